// k_pathtrace.hip.h — the per-path state machine of Raytracer.wgsl `main` + ray_color (:607-819) (start_sample,
// setup_surface, shade_bounce, finish_pixel) and two kernels that drive it: k_pathtrace (one pixel per lane) and
// k_pathtrace_persistent.  k_wf_shade (k_wavefront.hip.h) is the third driver.
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_PATHTRACE_HIP_H
#define MI355RT_K_PATHTRACE_HIP_H

namespace rtk {

// ======================================================================= per-path state machine
// One sample of the reference is a PathState that advances one bounce per shade_bounce() call.  The three kernel forms
// differ only in how they schedule paths and when they trace the rays a bounce asks for; traversal draws no random
// numbers, so per path the arithmetic, the RNG draw order and the order of f32 additions are those of ray_color (and of
// the oracle) in every form, and so are the pixels.

struct PathState {
  uint32_t pixel, rng, depth, sample;
  rt3 ro, rd, throughput, radiance, col;
  float prev_pdf;
  bool specular;
  // current surface
  float hit_t;
  uint32_t tri, inst;
  rt3 normal, geom_n, albedo;
  rt2 tex_uv;
};

// the state of a lane without a path: every field zero, specular = true (set field by field: `PathState p = {}` costs the
// global-memory persistent kernel 3 more VGPR spills in the product build)
__device__ __forceinline__ PathState idle_path() {
  PathState p;
  p.pixel = p.rng = p.depth = p.sample = 0u;
  p.ro = p.rd = p.throughput = p.radiance = p.col = p.normal = p.geom_n = p.albedo = rt3_splat(0.0f);
  p.prev_pdf = p.hit_t = 0.0f;
  p.specular = true;
  p.tri = p.inst = 0u;
  p.tex_uv = rt2_make(0.0f, 0.0f);
  return p;
}

// surface frame of the hit (tri, inst) for the ray (ro, rd): Raytracer.wgsl:738-779
// REC (the one-leaf forms of the persistent kernel): wrec holds the world record of every triangle (k_prepare_world_tris),
// and the geometric normal, which depends on (instance, triangle) alone, is read from it: the bits the expression below
// gives, made once per upload.  The texture coordinates are interpolated only when the scene has a texture layer:
// without one sample_tex returns 1 and never looks at them.
// PLAIN (k_pathtrace_persistent_plain): the host has seen every triangle of the scene fail both texture tests below
// (scene_facts.h), which are then not made.
template <bool REC = false, bool PLAIN = false>
__device__ __forceinline__ void setup_surface(const DevScene& S, PathState& p, bool from_gbuffer, float gx, float gy,
                                              uint32_t galbedo, const float4* wrec = nullptr) {
  InvRows m = load_inv_rows(S, p.inst);
  Bary b = barycentrics(S, p.tri, mul_point(m, p.ro), mul_dir(m, p.rd));
  const float4* ts = S.tri_shade + 8 * (size_t)p.tri;   // the hit's shading record: one 128-byte line
  float4 q4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q5 = q4, q6 = q4;
  if (!REC || !from_gbuffer) {   // the vertex normals: the G-buffer has the depth-0 normal already
    q4 = ts[4];
    q5 = ts[5];
    q6 = ts[6];
  }
  if (!REC || S.tex_layers != 0u) {   // wave-uniform
    const float4 q7 = ts[7];
    p.tex_uv = rt2_make(ts[4].w, ts[5].w) * b.w + rt2_make(ts[6].w, q7.x) * b.u + rt2_make(q7.y, q7.z) * b.v;
  }
  if (from_gbuffer) {
    p.hit_t = b.t;
    p.normal = unpack_normal(gx, gy);
    p.albedo = rt3_make(rt_from_unorm8(galbedo & 255u), rt_from_unorm8((galbedo >> 8) & 255u),
                        rt_from_unorm8((galbedo >> 16) & 255u));
  } else {
    rt3 ln = rt_normalize(xyz(q4) * b.w + xyz(q5) * b.u + xyz(q6) * b.v);
    p.normal = rt_normalize(normal_to_world(m, ln));
    float4 nd0 = ts[0], nd2 = ts[2];
    p.albedo = xyz(nd0);
    if (!PLAIN && nd2.x > -0.5f) p.albedo = p.albedo * sample_tex(S, p.tex_uv, rt_f2i32_sat(nd2.x));
    if (!PLAIN && nd2.z > -0.5f) {
      rt3 n_map = sample_tex(S, p.tex_uv, rt_f2i32_sat(nd2.z)) * 2.0f - rt3_splat(1.0f);
      rt3 T = rt_normalize(b.e1);
      rt3 B = rt_normalize(rt_cross(ln, T));
      rt3 ln_mapped = rt_normalize(T * n_map.x + B * n_map.y + ln * n_map.z);
      p.normal = rt_normalize(normal_to_world(m, ln_mapped));
    }
  }
  if constexpr (REC) {
    p.geom_n = xyz(wrec[2 * p.tri]);
  } else {
    p.geom_n = rt_normalize(normal_to_world(m, rt_normalize(rt_cross(b.e1, b.e2))));
  }
}

// the camera of the uniforms, read once per kernel
struct CameraBasis {
  rt3 o, ll, h, v;
  float lens;   // camera.origin.w: > 0 draws a thin-lens offset per sample
};
__device__ __forceinline__ CameraBasis camera_basis(const rt_scene_uniforms& U) {
  CameraBasis c;
  c.o = rt3_make(U.camera.origin[0], U.camera.origin[1], U.camera.origin[2]);
  c.ll = rt3_make(U.camera.lower_left[0], U.camera.lower_left[1], U.camera.lower_left[2]);
  c.h = rt3_make(U.camera.horizontal[0], U.camera.horizontal[1], U.camera.horizontal[2]);
  c.v = rt3_make(U.camera.vertical[0], U.camera.vertical[1], U.camera.vertical[2]);
  c.lens = U.camera.origin[3];
  return c;
}

// The arguments of the persistent kernel as they lie in its kernel-argument segment (the parameter list of
// k_pathtrace_persistent.hip.h, in order: keep the two in step), and the segment seen through an opaque copy of its address.
// A group of wave-uniform words read through it at the point of use is a scalar load served by the scalar cache, where the
// same words read from the parameter are loaded once before the loop and held in scalar registers the kernel does not
// have (it spills them to lanes of a VGPR and reads them back with a vector instruction each).
struct PtKernArgs {
  DevScene Sg;
  DevFrame F;
  rt_scene_uniforms U;
  uint32_t* ticket;
  uint32_t n_nodes_total, n_tris_total, n_inst_total, n_verts_total;
  const DevFrameSlot* slots;
  uint32_t n_slots;
  LdsPlan plan;
};
typedef const PtKernArgs __attribute__((address_space(4))) * rt_kernargs;
__device__ __forceinline__ rt_kernargs fresh_kernargs() {
  rt_kernargs k = (rt_kernargs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}
// camera_basis(U) of the kernel's U, read as new
__device__ __forceinline__ CameraBasis fresh_camera_basis() {
  const rt_kernargs k = fresh_kernargs();
  CameraBasis c;
  c.o = rt3_make(k->U.camera.origin[0], k->U.camera.origin[1], k->U.camera.origin[2]);
  c.ll = rt3_make(k->U.camera.lower_left[0], k->U.camera.lower_left[1], k->U.camera.lower_left[2]);
  c.h = rt3_make(k->U.camera.horizontal[0], k->U.camera.horizontal[1], k->U.camera.horizontal[2]);
  c.v = rt3_make(k->U.camera.vertical[0], k->U.camera.vertical[1], k->U.camera.vertical[2]);
  c.lens = k->U.camera.origin[3];
  return c;
}

// Start sample p.sample of pixel p.pixel = (x, y) in the frame `slot` (Raytracer.wgsl:798-809, :608-619): seed the RNG,
// make the camera ray, reset the path and take the depth-0 surface from the frame's G-buffer.  Returns false for a
// background pixel (or MAX_DEPTH = 0): the sample is black and ends at once.  LIVE: the caller has made that test on the
// pixel's G-buffer depth already (k_pathtrace_persistent hands out no other pixel); the depth is not read again and the
// sample always starts.  DEFER (the one-leaf forms of k_pathtrace_persistent): the surface frame is not made here; p.tri and
// p.inst are set, the pixel's packed normal and albedo are handed on in `gs`, and the caller's one surface pass of the trip
// calls setup_surface(.., from_gbuffer = true, ..) for the lane.
struct GbufSurface {
  float nx, ny;       // octahedral normal (normal_id.xy)
  uint32_t albedo;    // rgba8
};
template <bool LIVE = false, bool REC = false, bool DEFER = false>
__device__ __forceinline__ bool start_sample(const DevScene& S, const DevFrame& F, const rt_scene_uniforms& U,
                                             const CameraBasis& cam, const DevFrameSlot& slot, uint32_t x, uint32_t y,
                                             PathState& p, const float4* wrec = nullptr, GbufSurface* gs = nullptr) {
  p.rng = init_rng(p.pixel, slot.frame_count * F.spp + p.sample);
  rt3 off = rt3_splat(0.0f);
  if (cam.lens > 0.0f) {  // random_in_unit_disk (:201-205)
    float r = rt_sqrt(rand_pcg(p.rng));
    float theta = RT_TWO_PI * rand_pcg(p.rng);
    float st, ct;
    rt_sincos(theta, &st, &ct);
    rt3 rdk = cam.lens * rt3_make(r * ct, r * st, 0.0f);
    rt3 cu = rt3_make(U.camera.u[0], U.camera.u[1], U.camera.u[2]);
    rt3 cv = rt3_make(U.camera.v[0], U.camera.v[1], U.camera.v[2]);
    off = cu * rdk.x + cv * rdk.y;
  }
  float u = rt_div((float)x + 0.5f + slot.jitter_x * (float)U.width, (float)U.width);
  float v = 1.0f - rt_div((float)y + 0.5f + slot.jitter_y * (float)U.height, (float)U.height);
  p.rd = cam.ll + u * cam.h + v * cam.v - cam.o - off;
  p.ro = cam.o + off;
  p.throughput = rt3_splat(1.0f);
  p.radiance = rt3_splat(0.0f);
  p.prev_pdf = 0.0f;
  p.specular = true;
  p.depth = 0u;
  // the three G-buffer words of the pixel are requested together (they come from HBM: one round trip instead of depth
  // first, then the rest)
  const float gdepth = LIVE ? 0.0f : slot.depth[p.pixel];
  float4 g;
  uint32_t galbedo;
  if constexpr (DEFER) {
    // the plane pointers come out of the slot table in memory, so the compiler cannot tell their address space: named
    // global here, or each load is a flat one that waits on the LDS counter as well (ld_g, k_traverse.hip.h)
    const f4 gv = ld_g(reinterpret_cast<const f4*>(slot.normal_id), p.pixel);
    g = make_float4(gv.x, gv.y, gv.z, gv.w);
    galbedo = ld_g32(slot.albedo, p.pixel);
  } else {
    g = slot.normal_id[p.pixel];
    galbedo = slot.albedo[p.pixel];
  }
  if (LIVE || (!(gdepth >= 1.0f) && F.max_depth != 0u)) {
    p.tri = rt_f2u(g.z);
    p.inst = rt_f2u(g.w);
    if constexpr (DEFER) {
      gs->nx = g.x;
      gs->ny = g.y;
      gs->albedo = galbedo;
    } else {
      setup_surface<REC>(S, p, true, g.x, g.y, galbedo, wrec);
    }
    return true;
  }
  return false;
}

// One bounce of ray_color for a path whose surface frame is ready (Raytracer.wgsl:656-728): emissive / MIS, the
// three NEE draws and the pending NEE term, BSDF sampling, throughput, ray offset, Russian roulette, depth limit.
// The shadow ray and the extension ray it asks for are traced by the caller (megakernel trip or wavefront stage).
struct BounceOut {
  bool want_shadow, want_extend, nee_valid, ended;
  rt3 sh_o, sh_d, nee;
  float sh_tmax;
};
// REC: light_pdf and sample_light read the records of the one-leaf forms (setup_surface)
// PLAIN (k_pathtrace_persistent_plain): the host has seen (scene_facts.h) that every triangle's material word decodes to 0 or
// 3, that both texture tests below fail on every triangle and that a triangle with an emission longer than 1e-4 is a light:
// the material is taken as 3 or 0, the texture tests are not made and the emissive test is the material's alone.  What is
// left is evaluated as written, so a path gets the bits of the generic form.
template <bool REC = false, bool PLAIN = false>
__device__ __forceinline__ void shade_bounce(const DevScene& S, uint32_t light_count, uint32_t max_depth, PathState& p,
                                             BounceOut& o, const float4* wrec = nullptr) {
  o.want_shadow = o.want_extend = o.nee_valid = false;
  o.sh_o = o.sh_d = o.nee = rt3_splat(0.0f);
  o.sh_tmax = 0.0f;
  const float4* ts = S.tri_shade + 8 * (size_t)p.tri;
  float4 d0 = ts[0], d1 = ts[1], d2 = ts[2], d3 = ts[3];
  const uint32_t mat_word = rt_f2u32_sat(d0.w + 0.5f);
  const uint32_t mat_type = PLAIN ? (mat_word == 3u ? 3u : 0u) : mat_word;
  const rt3 hit_p = p.ro + p.rd * p.hit_t;
  p.normal = (rt_dot(p.rd, p.normal) < 0.0f) ? p.normal : -p.normal;
  p.geom_n = (rt_dot(p.rd, p.geom_n) < 0.0f) ? p.geom_n : -p.geom_n;
  float metallic = d1.x, roughness = d1.y;
  if (!PLAIN && d2.y > -0.5f) {
    rt3 mr = sample_tex(S, p.tex_uv, rt_f2i32_sat(d2.y));
    metallic *= mr.z;
    roughness *= mr.y;
  }
  roughness = rt_max(roughness, 0.005f);
  rt3 emissive = xyz(d3);
  if (!PLAIN && d2.w > -0.5f) emissive = emissive * sample_tex(S, p.tex_uv, rt_f2i32_sat(d2.w));
  const rt3 f0 = rt_mix3(rt3_splat(0.04f), p.albedo, metallic);

  bool ended = false;
  if (mat_type == 3u || (!PLAIN && rt_length(emissive) > 1e-4f)) {
    rt3 em_val = (mat_type == 3u) ? p.albedo : emissive;
    if (p.specular) {
      p.radiance = p.radiance + p.throughput * em_val;
    } else {
      p.radiance = p.radiance + p.throughput * em_val *
                                    power_heuristic(p.prev_pdf, REC ? light_pdf_rec(wrec, light_count, p.tri, p.hit_t, p.rd)
                                                                    : light_pdf(S, light_count, p.tri, p.inst, p.hit_t, p.rd));
    }
    if (mat_type == 3u) ended = true;
  }
  if (!ended) {
    if (mat_type != 2u) {  // NEE: the 3 draws happen here, the shadow ray is traced below
      LightSample ls = REC ? sample_light_rec(S, light_count, hit_p, p.rng) : sample_light(S, light_count, hit_p, p.rng);
      if (ls.pdf > 0.0f) {
        rt3 bsdf_val = rt3_splat(0.0f);
        float bsdf_pdf = 0.0f;
        if (mat_type == 0u) {
          bsdf_val = rt_div_pi3(p.albedo);
          bsdf_pdf = rt_div_pi(rt_max(rt_dot(p.normal, ls.dir), 0.0f));
        } else if (mat_type == 1u) {
          bsdf_val = eval_ggx(p.normal, -p.rd, ls.dir, roughness, f0);
          rt3 H = rt_normalize(-p.rd + ls.dir);
          bsdf_pdf = rt_div(ggx_d(rt_dot(p.normal, H), roughness * roughness) * rt_max(rt_dot(p.normal, H), 0.0f),
                            4.0f * rt_max(rt_dot(-p.rd, H), 0.0f));
        }
        o.want_shadow = true;  // the reference traces the shadow ray before looking at bsdf_pdf
        o.sh_o = hit_p + p.geom_n * 1e-4f;
        o.sh_d = ls.dir;
        o.sh_tmax = ls.dist - 2e-4f;
        o.nee_valid = bsdf_pdf > 0.0f;
        if (o.nee_valid) {
          o.nee = rt_div3z(p.throughput * bsdf_val * ls.L * power_heuristic(ls.pdf, bsdf_pdf) *
                               rt_max(rt_dot(p.normal, ls.dir), 0.0f), ls.pdf);
        }
      }
    }
    Scatter sc;
    if (mat_type == 0u) {
      sc = sample_diffuse(p.normal, p.albedo, p.rng);
    } else if (mat_type == 1u) {
      sc = sample_ggx(p.normal, -p.rd, roughness, f0, p.rng);
    } else {
      sc = sample_dielectric(p.rd, p.normal, d1.z, p.albedo, p.rng);
    }
    if (mat_type != 2u && rt_dot(sc.dir, p.geom_n) <= 0.0f) {
      sc.pdf = 0.0f;
      sc.throughput = rt3_splat(0.0f);
    }
    if (sc.pdf <= 0.0f || rt_length(sc.throughput) <= 0.0f) {
      ended = true;
    } else {
      p.throughput = p.throughput * sc.throughput;
      rt3 offset_n = (rt_dot(sc.dir, p.geom_n) > 0.0f) ? p.geom_n : -p.geom_n;
      p.ro = hit_p + offset_n * 1e-4f;
      p.rd = sc.dir;
      p.prev_pdf = sc.pdf;
      p.specular = sc.specular;
      if (p.depth > 3u) {
        float pr = rt_max(p.throughput.x, rt_max(p.throughput.y, p.throughput.z));
        if (rand_pcg(p.rng) > pr) {
          ended = true;
        } else {
          p.throughput = rt_div3z(p.throughput, pr);
        }
      }
      if (!ended) {
        if (p.depth < max_depth - 1u) {
          o.want_extend = true;
        } else {
          ended = true;  // depth limit: the loop condition ends the path after this bounce
        }
      }
    }
  }
  o.ended = ended;
}

// The pixel's last sample is done (Raytracer.wgsl:811-818): average the samples, then accumulate, or park the colour of
// frame `item_slot` of a batch in frame_col (F.frame_col is set for batched and wavefront dispatches, whose frames
// k_accumulate_frames adds in order).  Unbatched, slots[0] is the frame.
__device__ __forceinline__ void finish_pixel(const DevFrame& F, const rt_scene_uniforms& U, const DevFrameSlot* slots,
                                             uint32_t item_slot, uint32_t pixel, rt3 col) {
  if (F.spp != 1u) col = rt_div3z(col, (float)F.spp);   // x / 1 = x, bit for bit
  if (F.frame_col) {
    F.frame_col[(size_t)item_slot * ((size_t)U.width * U.height) + pixel] = make_float4(col.x, col.y, col.z, 1.0f);
  } else {
    float4 acc = make_float4(col.x, col.y, col.z, 1.0f);
    if (slots[0].frame_count > 1u) {
      float4 prev = F.accum[pixel];
      acc = make_float4(prev.x + col.x, prev.y + col.y, prev.z + col.z, prev.w + 1.0f);
    }
    F.accum[pixel] = acc;
  }
}
// finish_pixel of a pixel whose samples were all background: their sum is +0 and so is its average, +0 / SPP for every
// SPP >= 1 (rt_set_pipeline refuses 0), so no division is made
__device__ __forceinline__ void finish_black_pixel(const DevFrame& F, const rt_scene_uniforms& U, const DevFrameSlot* slots,
                                                   uint32_t item_slot, uint32_t pixel) {
  DevFrame f = F;
  f.spp = 1u;
  finish_pixel(f, U, slots, item_slot, pixel, rt3_splat(0.0f));
}

// ======================================================================= path tracer, one pixel per lane
// Raytracer.wgsl `main` (:791-819) as written: a lane runs its pixel's samples one after another and traces the rays of
// each bounce at once with the per-lane walk (k_intersect.hip.h).  Kept for A/B timing (kernel variant 0); unbatched only.
template <bool DETAIL>
__global__ __launch_bounds__(64) void k_pathtrace(DevScene S, DevFrame F, rt_scene_uniforms U,
                                                  const DevFrameSlot* __restrict__ slots) {
  uint32_t x, y;
  bool live = tile_pixel(U, x, y) && owns_row(F, y);
  LaneCounters c = {0, 0, 0, 0, 0, 0};
  if (live) {
    const CameraBasis cam = camera_basis(U);
    const DevFrameSlot slot = slots[0];
    PathState p = idle_path();
    p.pixel = y * U.width + x;
    for (p.sample = 0u; p.sample < F.spp; p.sample++) {
      bool alive = start_sample(S, F, U, cam, slot, x, y, p);
      while (alive) {
        if (DETAIL) c.shaded++;
        BounceOut bo;
        shade_bounce(S, U.light_count, F.max_depth, p, bo);
        if (bo.want_shadow) {
          c.shadow++;
          const bool occluded = trace_any<DETAIL>(S, U.blas_base_idx, bo.sh_o, bo.sh_d, RT_T_MIN, bo.sh_tmax, c);
          if (!occluded && bo.nee_valid) p.radiance = p.radiance + bo.nee;
        }
        alive = bo.want_extend;
        if (alive) {
          c.extension++;
          const Hit hit = trace_closest<DETAIL>(S, U.blas_base_idx, p.ro, p.rd, RT_T_MIN, RT_T_MAX, c);
          alive = hit.inst >= 0;   // a miss ends the path
          if (alive) {
            p.hit_t = hit.t;
            p.tri = (uint32_t)hit.tri;
            p.inst = (uint32_t)hit.inst;
            setup_surface(S, p, false, 0.0f, 0.0f, 0u);
            p.depth++;
          }
        }
      }
      p.col = p.col + p.radiance;
    }
    finish_pixel(F, U, slots, 0u, p.pixel, p.col);
  }
  flush_counters<DETAIL>(c, F.counters, blockIdx.x);
}

// ============================================================ path tracer, persistent form
// k_pathtrace_persistent: the production path-trace kernel.
//
//  * persistent waves: the grid is sized to the resident wave count; each wave pulls 8x8 pixel
//    tiles from a global ticket counter until the image is exhausted (one ray per lane);
//  * path regeneration: a lane whose path ended (light hit, miss, absorbed, Russian roulette,
//    depth limit) takes the next pixel of its wave's current tile, found with a ballot/mbcnt prefix
//    over the idle mask, so the 64 lanes stay busy instead of waiting for the longest path; a pixel
//    whose G-buffer holds background is finished there (colour +0) and the lane takes the next one, so
//    that no trip carries a lane with nothing to trace;
//  * per trip every live lane executes exactly one bounce: shade -> (NEE shadow ray) -> scatter ->
//    (extension ray), so the wave runs the two traversals and the shading code converged;
//  * traversal data (nodes, triangle records, instance records) is staged once per workgroup in LDS
//    when it fits (LDS = true); larger scenes read the same records through L1/L2;
//  * TLAS and BLAS are walked by ONE loop with an in-instance flag, so lanes in different
//    instances / levels share the node fetch + slab test.
// Only the scheduling differs from k_pathtrace, which cannot change any pixel because paths are independent.

// (the wave-level walk itself — TravMem, trav_step, tri_flush, traverse() — is in k_traverse.hip.h)

// Stage the whole scene (traversal records + shading arrays), exactly the slots launch_plan.h scene_lds_slots counts, in its
// order, from slot rec0 of the workgroup's LDS on: M reads every traversal record from LDS, and S (a copy of Sg on entry)
// gets the LDS addresses of the arrays shading reads.  The caller's __syncthreads() follows.  (k_pathtrace_persistent keeps
// a register-tuned copy of this for its LEAN / ONE_INST forms, which stage less: launch_plan.h one_leaf_lds_slots.)
__device__ __forceinline__ void stage_whole_scene(TravMem& M, DevScene& S, f4* s_scene, uint32_t rec0, const DevScene& Sg,
                                                  uint32_t n_nodes, uint32_t n_tris, uint32_t n_inst, uint32_t n_verts) {
  uint32_t slot = rec0;
  auto stage = [&](const void* src, size_t n) {
    f4* base = s_scene + slot;
    lds_stage(base, src, n);
    slot += (uint32_t)n;
    return base;
  };
  M.gnodes = M.gtri = M.ginst = nullptr;
  M.groot = nullptr;
  M.k_lds = n_nodes;
  M.t_min = RT_T_MIN;
  M.l_nodes = slot;
  S.tnodes = reinterpret_cast<const float4*>(stage(Sg.tnodes, (size_t)2 * n_nodes));
  M.l_tri = slot;
  S.tri_geom = reinterpret_cast<const float4*>(stage(Sg.tri_geom, (size_t)RT_TRI_STRIDE * n_tris));
  M.l_inst = slot;
  S.inst_trav = reinterpret_cast<const float4*>(stage(Sg.inst_trav, (size_t)4 * n_inst));
  M.l_root = slot;
  stage(Sg.inst_root, ((size_t)n_inst + 3) / 4);
  S.tri_shade = reinterpret_cast<const float4*>(stage(Sg.tri_shade, (size_t)8 * n_tris));
  S.topo = reinterpret_cast<const float4*>(stage(Sg.topo, (size_t)5 * n_tris));
  S.pos = reinterpret_cast<const float4*>(stage(Sg.pos, n_verts));
  // uv (8 B/vertex) and lights (8 B each): the device buffers are allocated with >= 16-byte slack
  S.uv = reinterpret_cast<const float2*>(stage(Sg.uv, ((size_t)n_verts + 1) / 2));
  S.inst = reinterpret_cast<const float4*>(stage(Sg.inst, (size_t)9 * n_inst));
  S.lights = reinterpret_cast<const uint2*>(stage(Sg.lights, ((size_t)Sg.n_lights + 1) / 2));
  S.light_rec = reinterpret_cast<const float4*>(stage(Sg.light_rec, (size_t)4 * Sg.n_lights));
}

// Diagnostic build only (-DRT_CLOCK_STAMP, tools/clock_check.py): every workgroup of the persistent kernel stamps
// s_memtime / s_memrealtime around its work loop into this array, which nothing else reads; the in-kernel clock is
// delta(memtime) / delta(memrealtime) x 100 MHz.  In the product build no stamp executes.
#define RT_CLOCK_STAMP_SLOTS 4096
__device__ unsigned long long g_clock_stamps[2 * RT_CLOCK_STAMP_SLOTS];
// Diagnostic build only (-DRT_PT_STAMPS, tools/pt_sections.py): s_memtime cycles the persistent kernel's waves spend in
// the five sections of a trip (regenerate + start a sample, shade, shadow traversal, extension traversal + surface frame,
// finish), summed over all waves; [5] = trips, [6] = waves, [7] = the surface pass of the one-leaf forms, which is then in
// neither the first nor the fourth section.
__device__ unsigned long long g_pt_sections[8];

// Occupancy: the LDS-resident form is VALU-issue bound (3, 4, 5 waves/SIMD within 2 %), the global-memory form
// is latency bound and gains ~11 % from 6 waves/SIMD even with the spills that costs (measured on MI355X).
// Fill TravMem for the mixed mode and stage what the plan names (LdsPlan, lds_sizes.h; decided on the host, launch_plan.h
// plan_lds); returns the number of 16-byte slots used.
__device__ __forceinline__ uint32_t trav_stage_mixed(TravMem& M, f4* lds, uint32_t slot0, const DevScene& Sg, const LdsPlan& P,
                                                     uint32_t n_tris_total, uint32_t n_inst_total) {
  uint32_t slot = slot0;
  M.gnodes = reinterpret_cast<const f4*>(Sg.tnodes);
  M.gtri = reinterpret_cast<const f4*>(Sg.tri_geom);
  M.ginst = reinterpret_cast<const f4*>(Sg.inst_trav);
  M.groot = Sg.inst_root;
  M.k_lds = P.k_nodes;
  M.t_min = RT_T_MIN;
  M.l_nodes = slot;
  lds_stage(lds + slot, Sg.tnodes, (size_t)2 * P.k_nodes);
  slot += 2u * P.k_nodes;
  M.l_inst = M.l_root = M.l_tri = RT_LDS_NONE;
  if (P.stage_inst) {
    M.l_inst = slot;
    lds_stage(lds + slot, Sg.inst_trav, (size_t)4 * n_inst_total);
    slot += 4u * n_inst_total;
    M.l_root = slot;
    lds_stage(lds + slot, Sg.inst_root, ((size_t)n_inst_total + 3) / 4);   // the buffer has 16 bytes of slack
    slot += (n_inst_total + 3u) / 4u;
  }
  if (P.stage_tri) {
    M.l_tri = slot;
    lds_stage(lds + slot, Sg.tri_geom, (size_t)RT_TRI_STRIDE * n_tris_total);
    slot += (uint32_t)RT_TRI_STRIDE * n_tris_total;
  }
  return slot - slot0;
}

// Occupancy: the LDS-resident form is latency bound at 4 waves/SIMD (registers), the global-memory form gains ~11 %
// from 6 waves/SIMD even with the spills that costs (measured on MI355X).  The one-leaf-TLAS LDS form (ONE_INST, product
// build) fits 96 VGPRs without spills (LEAN below, tests/test_kernel_resources.py) and runs at 5 waves/SIMD: Cornell
// 38.6 -> 34.0 ms per image.  Five is also the LDS ceiling of Cornell (about 29.5 KB per workgroup); a
// one-leaf scene that stages more gets fewer workgroups from the host's occupancy query.  Its counting build stays at 4.
// Where three 512-thread workgroups fit the CU's LDS (Cornell: about 52 KB each, one staged scene per eight waves), the
// host runs the same product form of a batched dispatch as k_pathtrace_persistent_wide at RT_PT_WIDE_WAVES = 6 waves per
// SIMD.  At 80 VGPRs it still
// spills (64 B/lane of scratch, SLIM in k_pathtrace_persistent.hip.h, tests/test_kernel_resources_wide.py) and is faster
// all the same: Cornell 34.02 -> 33.15 ms per image.
#ifndef RT_PT_LDS_WAVES
#define RT_PT_LDS_WAVES 4      // waves per SIMD of the LDS-resident form (128 VGPRs)
#endif
#ifndef RT_PT_GLOBAL_WAVES
#define RT_PT_GLOBAL_WAVES 6   // workgroups of 4 waves per CU = waves per SIMD of the global-memory form (tools/SWEEPS.md)
#endif
#ifndef RT_PT_ONE_INST_WAVES
#define RT_PT_ONE_INST_WAVES 5 // waves per SIMD of the one-leaf-TLAS LDS form, product build (96 VGPRs)
#endif
#ifndef RT_PT_WIDE_WAVES
#define RT_PT_WIDE_WAVES 6     // waves per SIMD of the same form in 512-thread workgroups (80 VGPRs)
#endif
// a wave-uniform value taken as new at this point: nothing computed from it is hoisted out of the loop it is used in
__device__ __forceinline__ uint32_t rt_fresh(uint32_t v) {
  asm volatile("" : "+s"(v));
  return v;
}
__device__ __forceinline__ rt_scene_uniforms fresh_size(const rt_scene_uniforms& U) {
  rt_scene_uniforms u = U;
  u.width = rt_fresh(U.width);
  u.height = rt_fresh(U.height);
  return u;
}
__device__ __forceinline__ DevFrame fresh_stripes(const DevFrame& F) {
  DevFrame f = F;
  f.stripe_rows = rt_fresh(F.stripe_rows);
  f.stripe_count = rt_fresh(F.stripe_count);
  return f;
}
__device__ __forceinline__ DevFrame fresh_spp(const DevFrame& F) {
  DevFrame f = F;
  f.spp = rt_fresh(F.spp);
  return f;
}
// SLIM (k_pathtrace_persistent_wide): the lane's sample sum is parked in LDS behind the WAVES wave queues, in three planes
// of WAVES * 64 floats (RT_PT_COL_BYTES_PER_WAVE per wave, lds_sizes.h; launch_plan.h sizes the launch's LDS with it)
template <uint32_t WAVES>
__device__ __forceinline__ float* col_park_at(f4* lds) {
  return reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + WAVES * RT_WORK_BYTES_PER_WAVE) + threadIdx.x;
}
template <uint32_t WAVES>
__device__ __forceinline__ void col_park_clear(f4* lds) {
  float* park = col_park_at<WAVES>(lds);
  park[0] = park[WAVES * 64] = park[2 * WAVES * 64] = 0.0f;
}
template <uint32_t WAVES>
__device__ __forceinline__ rt3 col_park_add(f4* lds, rt3 radiance) {   // the sum + radiance, parked again and returned
  float* park = col_park_at<WAVES>(lds);
  const rt3 col = rt3_make(park[0], park[WAVES * 64], park[2 * WAVES * 64]) + radiance;
  park[0] = col.x;
  park[WAVES * 64] = col.y;
  park[2 * WAVES * 64] = col.z;
  return col;
}

// k_pathtrace_persistent: 256-thread workgroups, every form
#define RT_PT_KERNEL k_pathtrace_persistent
#define RT_PT_WAVES 4
#define RT_PT_SIMD_WAVES (LDS ? ((ONE_INST && !DETAIL) ? RT_PT_ONE_INST_WAVES : RT_PT_LDS_WAVES) : RT_PT_GLOBAL_WAVES)
#define RT_PT_PLAIN false
#define RT_PT_SWEEP false
#define RT_PT_SWEEP_PARAMS
#define RT_PT_SWEEP_ARG nullptr, 0u, false
#include "k_pathtrace_persistent.hip.h"
#undef RT_PT_KERNEL
#undef RT_PT_WAVES
#undef RT_PT_SIMD_WAVES
#undef RT_PT_PLAIN
#undef RT_PT_SWEEP
#undef RT_PT_SWEEP_PARAMS
#undef RT_PT_SWEEP_ARG

// k_pathtrace_persistent_wide: the one-leaf-TLAS LDS form of the product build (rt_api.hip instantiates <false, true, true>
// only) in 512-thread workgroups.  Eight waves share one staged scene, so that three workgroups of a small scene (24 waves,
// 6 per SIMD) fit the CU's LDS where six 256-thread ones would not.
#define RT_PT_KERNEL k_pathtrace_persistent_wide
#define RT_PT_WAVES 8
#define RT_PT_SIMD_WAVES RT_PT_WIDE_WAVES
#define RT_PT_PLAIN false
#define RT_PT_SWEEP false
#define RT_PT_SWEEP_PARAMS
#define RT_PT_SWEEP_ARG nullptr, 0u, false
#include "k_pathtrace_persistent.hip.h"
#undef RT_PT_KERNEL
#undef RT_PT_WAVES
#undef RT_PT_SIMD_WAVES
#undef RT_PT_PLAIN
#undef RT_PT_SWEEP
#undef RT_PT_SWEEP_PARAMS
#undef RT_PT_SWEEP_ARG

// k_pathtrace_persistent_plain: the wide form (<false, true, true> only, the same workgroups and LDS layout) for a scene in
// which the host has seen nothing but untextured Lambertian triangles and lights (scene_facts.h; launch_plan.h
// persistent_shape).  shade_bounce and setup_surface are compiled without the GGX and dielectric branches, the four texture
// fetches and the emissive length, whose conditions the generic form evaluates on every trip to skip them; with their
// registers gone the kernel holds its 80 VGPRs without scratch (tests/test_kernel_resources_plain.py).
#define RT_PT_KERNEL k_pathtrace_persistent_plain
#define RT_PT_WAVES 8
#define RT_PT_SIMD_WAVES RT_PT_WIDE_WAVES
#define RT_PT_PLAIN true
#define RT_PT_SWEEP false
#define RT_PT_SWEEP_PARAMS
#define RT_PT_SWEEP_ARG nullptr, 0u, false
#include "k_pathtrace_persistent.hip.h"
#undef RT_PT_KERNEL
#undef RT_PT_WAVES
#undef RT_PT_SIMD_WAVES
#undef RT_PT_PLAIN
#undef RT_PT_SWEEP
#undef RT_PT_SWEEP_PARAMS
#undef RT_PT_SWEEP_ARG

// k_pathtrace_sweep_wide, k_pathtrace_sweep_plain: the wide form and its plain twin (<false, true, true> only, the same
// workgroups and LDS layout) for a scene whose BLAS the host has found sweepable (scene_facts.h walk_facts; launch_plan.h
// persistent_shape): both walks of a trip test the BLAS leaves in wave lock-step (k_traverse.hip.h traverse_leaves).  They
// take two parameters more: the leaf records with the node records behind them, and a word of the number of leaves (bits 0-15),
// the number of nodes (bits 16-30) and bit 31, set when every walk is to take the node sweep.
#define RT_PT_SWEEP true
#define RT_PT_SWEEP_PARAMS , const float4* __restrict__ leaf_recs, uint32_t leaf_info
#define RT_PT_SWEEP_ARG leaf_recs, leaf_info & 0xffffu, (leaf_info >> 31) != 0u, (leaf_info >> 16) & 0x7fffu
#define RT_PT_WAVES 8
#define RT_PT_SIMD_WAVES RT_PT_WIDE_WAVES
#define RT_PT_KERNEL k_pathtrace_sweep_wide
#define RT_PT_PLAIN false
#include "k_pathtrace_persistent.hip.h"
#undef RT_PT_KERNEL
#undef RT_PT_PLAIN
#define RT_PT_KERNEL k_pathtrace_sweep_plain
#define RT_PT_PLAIN true
#include "k_pathtrace_persistent.hip.h"
#undef RT_PT_KERNEL
#undef RT_PT_PLAIN
#undef RT_PT_WAVES
#undef RT_PT_SIMD_WAVES
#undef RT_PT_SWEEP
#undef RT_PT_SWEEP_PARAMS
#undef RT_PT_SWEEP_ARG

}  // namespace rtk
#endif
