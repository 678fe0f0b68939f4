// k_radiance.hip.h — k_radiance_query: the radiance that arrives along a caller's rays (rt_trace_radiance, mi355rt.h).
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_RADIANCE_HIP_H
#define MI355RT_K_RADIANCE_HIP_H

namespace rtk {

// The fourth driver of the per-path state machine (setup_surface / shade_bounce, k_pathtrace.hip.h), beside k_pathtrace,
// k_pathtrace_persistent and k_wf_shade.  Its rays come from a flat array of rt_ray {o, t_max} {d, pad} instead of the
// camera and the G-buffer, and its result goes to a flat array of rt_radiance {r, g, b, t} instead of the accumulator.
// Sample s of ray i is ray_color (Raytracer.wgsl:607-783) with rng = init_rng(pad, seed * spp + s) and the depth-0 surface
// taken from the TRACED hit, the way every later depth takes it (:738-779, setup_surface(.., from_gbuffer = false, ..)):
// no G-buffer, no octahedral normal, no unorm8 albedo, no lens offset, no jitter.
//  * the first segment is the closest hit in (RT_T_MIN, the ray's t_max); it does not depend on the sample, so it is
//    traced once per ray and counts as one extension ray.  Its (t, tri, inst) is kept in three registers and the surface
//    frame is made again at the start of every sample, because shade_bounce flips the normals in place;
//  * every later segment uses RT_T_MIN / RT_T_MAX and the shadow rays are those of shade_bounce, as in a frame;
//  * rgb = (((0 + r_0) + r_1) + ...) in sample order, divided by spp as finish_pixel does (not at all for spp == 1);
//    t = the first segment's distance; a miss is {+0, +0, +0, the bits of the ray's t_max};
//  * max_depth == 0: the first segment is traced and t reported, nothing is shaded (shade_bounce would compute
//    max_depth - 1u).
// Scheduling is the persistent kernel's: persistent waves, a chunk of RT_RAD_CHUNK consecutive rays per atomic, idle lanes
// take the next unassigned ray of the wave's chunk (ballot / prefix count), and per trip every live lane executes one
// bounce, so the wave runs both traversals and the shading code converged, with ONE call site per walk: the extension
// walk also traces the first segments (per-lane t_max).  A lane keeps its ray for all spp samples.  Paths are
// independent and traversal draws no random number, so a result depends on (scene, ray, pad, seed, spp, max_depth) only.
// LDS = true: the whole scene is staged, traversal records and shading arrays (the persistent kernel's non-ONE_INST LDS
// form); otherwise trav_stage_mixed with the host's plan.  There is no one-leaf / world-record form yet.
#ifndef RT_RAD_CHUNK
#define RT_RAD_CHUNK 64u   // rays per atomic: the persistent kernel's 8 x 8 tile
#endif

struct RadianceArgs {
  const float4* rays;   // 2 per ray
  float4* out;          // 1 per ray: {r, g, b, t}
  uint32_t* head;       // chunk counter, zeroed by the host before the launch
  uint64_t* counters;   // RT_COUNTER_SHARDS x 6, the query's own (flush_counters)
  uint32_t n_rays, max_depth, spp, seed;
  uint32_t light_count, blas_base;
  uint32_t n_nodes, n_tris, n_inst, n_verts;
};

template <bool DETAIL, bool LDS>
__global__ __launch_bounds__(256, LDS ? RT_PT_LDS_WAVES : RT_PT_GLOBAL_WAVES)
void k_radiance_query(DevScene Sg, RadianceArgs A, LdsPlan plan) {
  constexpr uint32_t WAVES = 4;
  extern __shared__ f4 s_scene[];
  // per-wave triangle work queue at the start of LDS, staged scene after it
  const uint32_t wave = threadIdx.x >> 6;
  WaveWork WW;
  wave_work_at(WW, reinterpret_cast<char*>(s_scene) + wave * RT_WORK_BYTES_PER_WAVE);
  const uint32_t rec0 = (WAVES * RT_WORK_BYTES_PER_WAVE) / 16;
  TravMem M;
  DevScene S = Sg;
  if (LDS) {
    // the slots of scene_lds_slots, in the persistent kernel's order
    uint32_t slot = rec0;
    auto stage = [&](const void* src, size_t n) {
      f4* base = s_scene + slot;
      lds_stage(base, src, n);
      slot += (uint32_t)n;
      return base;
    };
    M.gnodes = M.gtri = M.ginst = nullptr;
    M.groot = nullptr;
    M.k_lds = A.n_nodes;
    M.t_min = RT_T_MIN;
    M.l_nodes = slot;
    f4* ln = stage(Sg.tnodes, (size_t)2 * A.n_nodes);
    M.l_tri = slot;
    f4* lt = stage(Sg.tri_geom, (size_t)RT_TRI_STRIDE * A.n_tris);
    M.l_inst = slot;
    f4* li = stage(Sg.inst_trav, (size_t)4 * A.n_inst);
    M.l_root = slot;
    stage(Sg.inst_root, ((size_t)A.n_inst + 3) / 4);
    S.tri_shade = reinterpret_cast<const float4*>(stage(Sg.tri_shade, (size_t)8 * A.n_tris));
    S.topo = reinterpret_cast<const float4*>(stage(Sg.topo, (size_t)5 * A.n_tris));
    S.pos = reinterpret_cast<const float4*>(stage(Sg.pos, A.n_verts));
    // uv (8 B/vertex) and lights (8 B each): the device buffers are allocated with >= 16-byte slack
    S.uv = reinterpret_cast<const float2*>(stage(Sg.uv, ((size_t)A.n_verts + 1) / 2));
    S.inst = reinterpret_cast<const float4*>(stage(Sg.inst, (size_t)9 * A.n_inst));
    S.lights = reinterpret_cast<const uint2*>(stage(Sg.lights, ((size_t)Sg.n_lights + 1) / 2));
    S.light_rec = reinterpret_cast<const float4*>(stage(Sg.light_rec, (size_t)4 * Sg.n_lights));
    __syncthreads();
    S.tnodes = reinterpret_cast<const float4*>(ln);
    S.tri_geom = reinterpret_cast<const float4*>(lt);
    S.inst_trav = reinterpret_cast<const float4*>(li);
  } else {
    trav_stage_mixed(M, s_scene, rec0, Sg, plan, A.n_tris, A.n_inst);
    __syncthreads();
  }
  constexpr int MODE = LDS ? RT_TRAV_LDS : RT_TRAV_MIXED;
  constexpr uint32_t NO_HIT = 0xffffffffu;   // first_inst of a ray whose first segment is not traced yet

  const uint32_t lane = threadIdx.x & 63u;
  // wave-uniform work cursor: rays [chunk_pos, chunk_end) of the wave's chunk are still unassigned
  uint32_t chunk_pos = 0u, chunk_end = 0u;
  bool work_left = true;

  PathState p = idle_path();   // p.pixel: the lane's ray; p.col: its sample sum
  bool have_ray = false;       // lane owns a ray whose samples are not all done
  bool alive = false;          // lane owns a running sample
  bool first_seg = false;      // ... whose ray (p.ro, p.rd; t_max in p.hit_t) is the first segment, still to be traced
  float first_t = 0.0f;        // the first segment's hit, kept for the ray's later samples
  uint32_t first_tri = 0u, first_inst = NO_HIT;
  // cnt_ext, cnt_shadow: rays of the whole wave, wave-uniform (scalar registers); the others count per lane
  uint32_t cnt_ext = 0, cnt_shadow = 0, cnt_nodes = 0, cnt_tris = 0, cnt_shaded = 0;

  for (;;) {
    // ------------------------------------------------------------ regenerate
    // (a) wave-wide: every lane without a ray takes the next unassigned one of the wave's chunk.  All lanes execute this
    //     loop (busy lanes with need = false) so that the wave-uniform cursor stays identical in every lane.
    {
      bool need = !have_ray;
      for (;;) {
        const unsigned long long mask = __ballot(need);
        if (mask == 0ull || !work_left) break;
        if (chunk_pos >= chunk_end) {
          const int leader = __builtin_ctzll(mask);
          uint32_t t = 0;
          if (lane == (uint32_t)leader) t = atomicAdd(A.head, 1u);
          t = __shfl(t, leader, 64);
          // n_rays < 2^31 (the host refuses more) and at most one overshoot per wave: t * RT_RAD_CHUNK stays below 2^32
          if (t >= (A.n_rays + RT_RAD_CHUNK - 1u) / RT_RAD_CHUNK) {
            work_left = false;
            break;
          }
          chunk_pos = t * RT_RAD_CHUNK;
          chunk_end = min(chunk_pos + RT_RAD_CHUNK, A.n_rays);
        }
        // rank of this lane among the needy lanes
        const uint32_t rank =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        const uint32_t idx = chunk_pos + rank;
        if (need && idx < chunk_end) {
          need = false;
          have_ray = true;
          p.pixel = idx;
          p.sample = 0u;
          p.col = rt3_splat(0.0f);
          first_inst = NO_HIT;
        }
        chunk_pos += (uint32_t)__builtin_popcountll(mask);   // past chunk_end: the chunk is used up
      }
    }
    // (b) start the next sample of the owned ray: the ray is read again from the array (the path has overwritten it), and
    //     the depth-0 surface comes from the kept first hit, or the first segment joins this trip's extension walk
    if (!alive && have_ray) {
      const float4 r0 = A.rays[2 * (size_t)p.pixel], r1 = A.rays[2 * (size_t)p.pixel + 1];
      p.rng = init_rng(rt_f2u(r1.w), A.seed * A.spp + p.sample);
      p.ro = xyz(r0);
      p.rd = xyz(r1);
      p.throughput = rt3_splat(1.0f);
      p.radiance = rt3_splat(0.0f);
      p.prev_pdf = 0.0f;
      p.specular = true;
      p.depth = 0u;
      alive = true;
      if (first_inst == NO_HIT) {
        first_seg = true;
        p.hit_t = r0.w;   // no surface yet: the slot carries the segment's t_max to the walk
      } else {
        p.hit_t = first_t;
        p.tri = first_tri;
        p.inst = first_inst;
        setup_surface(S, p, false, 0.0f, 0.0f, 0u);
      }
    }
    const bool running = alive && !first_seg;
    bool path_done = false;

    // ------------------------------------------------------------ shade one bounce
    bool want_shadow = false, want_extend = first_seg;
    bool nee_valid = false;
    rt3 sh_o = rt3_splat(0.0f), sh_d = rt3_splat(0.0f), nee = rt3_splat(0.0f);
    float sh_tmax = 0.0f;
    if (running) {
      if (DETAIL) cnt_shaded++;
      BounceOut bo;
      shade_bounce(S, A.light_count, A.max_depth, p, bo);
      want_shadow = bo.want_shadow;
      want_extend = bo.want_extend;
      nee_valid = bo.nee_valid;
      sh_o = bo.sh_o;
      sh_d = bo.sh_d;
      sh_tmax = bo.sh_tmax;
      nee = bo.nee;
      if (bo.ended) path_done = true;
    }

    // ------------------------------------------------------------ shadow rays (any hit)
    const unsigned long long shadow_mask = __ballot(want_shadow);
    if (shadow_mask != 0ull) {
      cnt_shadow += (uint32_t)__builtin_popcountll(shadow_mask);
      float t_;
      int32_t a_, b_;
      bool occluded;
      traverse<true, DETAIL, MODE>(M, s_scene, WW, A.blas_base, want_shadow, sh_o, sh_d, sh_tmax, t_, a_, b_, occluded, cnt_nodes,
                                   cnt_tris);
      if (want_shadow) {
        if (!occluded && nee_valid) p.radiance = p.radiance + nee;  // nothing is added when bsdf_pdf <= 0
      }
    }

    // ------------------------------------------------------------ extension rays and first segments (closest hit)
    bool ray_done = false;   // the ray ends without a sample: first segment missed, or max_depth == 0
    const unsigned long long extend_mask = __ballot(want_extend);
    if (extend_mask != 0ull) {
      cnt_ext += (uint32_t)__builtin_popcountll(extend_mask);
      float t_;
      int32_t tri_, inst_;
      bool any_;
      traverse<false, DETAIL, MODE>(M, s_scene, WW, A.blas_base, want_extend, p.ro, p.rd, first_seg ? p.hit_t : RT_T_MAX, t_, tri_,
                                    inst_, any_, cnt_nodes, cnt_tris);
      if (want_extend) {
        if (inst_ < 0) {
          if (first_seg) {
            first_t = t_;   // a miss hands the bound back: the bits of the ray's t_max
            ray_done = true;
          } else {
            path_done = true;
          }
        } else {
          p.hit_t = t_;
          p.tri = (uint32_t)tri_;
          p.inst = (uint32_t)inst_;
          if (first_seg) {
            first_t = t_;
            first_tri = (uint32_t)tri_;
            first_inst = (uint32_t)inst_;
            if (A.max_depth == 0u) ray_done = true;
          } else {
            p.depth++;
          }
          if (!ray_done) setup_surface(S, p, false, 0.0f, 0.0f, 0u);
        }
        first_seg = false;
      }
    }

    // ------------------------------------------------------------ sample / ray finished
    if (path_done) {
      alive = false;
      p.col = p.col + p.radiance;
      p.sample++;
      if (p.sample >= A.spp) {  // the ray's last sample
        if (A.spp != 1u) p.col = rt_div3z(p.col, (float)A.spp);   // finish_pixel's average
        ray_done = true;
      }
    }
    if (ray_done) {   // p.col is +0 when no sample ran
      alive = false;
      have_ray = false;
      A.out[p.pixel] = make_float4(p.col.x, p.col.y, p.col.z, first_t);
    }
    if (!work_left && __ballot(have_ray) == 0ull) break;
  }

  // counters: one flush per persistent wave
  LaneCounters c;
  c.primary = 0;
  c.extension = lane == 0u ? cnt_ext : 0u;   // the wave's count, once
  c.shadow = lane == 0u ? cnt_shadow : 0u;
  c.nodes = cnt_nodes;
  c.tris = cnt_tris;
  c.shaded = cnt_shaded;
  flush_counters<DETAIL>(c, A.counters, blockIdx.x * WAVES + wave);
}

}  // namespace rtk
#endif
