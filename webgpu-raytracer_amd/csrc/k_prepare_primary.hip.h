// k_prepare_primary.hip.h — upload-time re-layout kernels and k_primary_visibility (Rasterizer.wgsl:81-173 restated as a ray cast).
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_PREPARE_PRIMARY_HIP_H
#define MI355RT_K_PREPARE_PRIMARY_HIP_H

namespace rtk {

// =========================================================== upload-time re-layout
__global__ void k_prepare_tris(const float4* __restrict__ topo, const float4* __restrict__ pos,
                               float4* __restrict__ tri_geom, uint32_t n_tris, uint32_t n_verts) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_tris) return;
  float4 idx = topo[5 * i];
  uint32_t i0 = rt_f2u(idx.x), i1 = rt_f2u(idx.y), i2 = rt_f2u(idx.z);
  if (i0 >= n_verts) i0 = n_verts - 1;  // robust buffer access: clamp instead of faulting
  if (i1 >= n_verts) i1 = n_verts - 1;
  if (i2 >= n_verts) i2 = n_verts - 1;
  rt3 v0 = xyz(pos[i0]), v1 = xyz(pos[i1]), v2 = xyz(pos[i2]);
  rt3 e1 = v1 - v0, e2 = v2 - v0;
  tri_geom[RT_TRI_STRIDE * i + 0] = make_float4(v0.x, v0.y, v0.z, 0.0f);
  tri_geom[RT_TRI_STRIDE * i + 1] = make_float4(e1.x, e1.y, e1.z, 0.0f);
  tri_geom[RT_TRI_STRIDE * i + 2] = make_float4(e2.x, e2.y, e2.z, 0.0f);
}
// per-triangle shading record (device_scene.h): pure copies
__global__ void k_prepare_tri_shade(const float4* __restrict__ topo, const float4* __restrict__ nrm,
                                    const float2* __restrict__ uv, float4* __restrict__ tri_shade, uint32_t n_tris,
                                    uint32_t n_verts) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_tris) return;
  float4 idx = topo[5 * i];
  uint32_t i0 = rt_f2u(idx.x), i1 = rt_f2u(idx.y), i2 = rt_f2u(idx.z);
  if (i0 >= n_verts) i0 = n_verts - 1;  // robust buffer access: clamp instead of faulting
  if (i1 >= n_verts) i1 = n_verts - 1;
  if (i2 >= n_verts) i2 = n_verts - 1;
  const float4 n0 = nrm[i0], n1 = nrm[i1], n2 = nrm[i2];
  const float2 t0 = uv[i0], t1 = uv[i1], t2 = uv[i2];
  float4* dst = tri_shade + 8 * (size_t)i;
  dst[0] = topo[5 * i + 1];
  dst[1] = topo[5 * i + 2];
  dst[2] = topo[5 * i + 3];
  dst[3] = topo[5 * i + 4];
  dst[4] = make_float4(n0.x, n0.y, n0.z, t0.x);
  dst[5] = make_float4(n1.x, n1.y, n1.z, t0.y);
  dst[6] = make_float4(n2.x, n2.y, n2.z, t1.x);
  dst[7] = make_float4(t1.y, t2.x, t2.y, 0.0f);
}
__global__ void k_prepare_lights(DevScene S, float4* __restrict__ light_rec, uint32_t n, uint32_t n_tris,
                                 uint32_t n_inst) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint2 ref = S.lights[i];
  if (ref.y >= n_tris) ref.y = n_tris - 1;  // robust buffer access: clamp instead of faulting
  if (ref.x >= n_inst) ref.x = n_inst - 1;
  WorldTri w = world_triangle(S, ref.y, ref.x);
  rt3 edge1 = w.v1 - w.v0;
  rt3 edge2 = w.v2 - w.v0;
  rt3 cr = rt_cross(edge1, edge2);
  rt3 n_raw = rt_normalize(cr);
  float area = rt_length(cr) * 0.5f;
  light_rec[4 * i + 0] = make_float4(w.v0.x, w.v0.y, w.v0.z, area);
  light_rec[4 * i + 1] = make_float4(w.v1.x, w.v1.y, w.v1.z, n_raw.x);
  light_rec[4 * i + 2] = make_float4(w.v2.x, w.v2.y, w.v2.z, n_raw.y);
  light_rec[4 * i + 3] = make_float4(n_raw.z, rt_u2f(ref.y), 0.0f, 0.0f);
}
// Per-triangle world records of a scene whose TLAS is one node, a leaf: every hit is in the instance that node names, so
// what the kernels would compute per hit from (instance, triangle) alone is made here once per upload, by the very
// functions they call (the library is compiled without contraction and with correctly rounded division, square root and
// normalisation: the same expression on the same inputs gives the same bits in any kernel, NaN of a zero-area triangle
// included).
//   tri_world    2 x float4 / tri   {geom_n.xyz, light area} {light normal.xyz, 0}: setup_surface's geometric normal, and
//                area and unit normal of the world-space triangle as light_pdf computes them.  The host places them
//                behind the n_tris shading records, in the same buffer (tri_shade + 8 * n_tris)
//   tri_shade_w  8 x float4 / tri   the shading record with the three vertex normals taken to world space and normalised,
//                as k_primary_visibility does per pixel
// Runs after k_prepare_tris / k_prepare_tri_shade / k_prepare_instances and the node pass (it reads their outputs).
__global__ void k_prepare_world_tris(DevScene S, float4* __restrict__ tri_world, float4* __restrict__ tri_shade_w,
                                     uint32_t n_tris, uint32_t n_inst) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_tris) return;
  // the instance of the TLAS leaf (node 0), as traverse<.., ONE_INST> reads it: further instances may exist, unreferenced
  uint32_t inst = rt_f2u(S.tnodes[1].w) >> 3;
  if (inst >= n_inst) inst = n_inst - 1;  // robust buffer access: clamp instead of faulting
  const InvRows m = load_inv_rows(S, inst);
  const rt3 e1 = xyz(S.tri_geom[RT_TRI_STRIDE * i + 1]), e2 = xyz(S.tri_geom[RT_TRI_STRIDE * i + 2]);
  const rt3 geom_n = rt_normalize(normal_to_world(m, rt_normalize(rt_cross(e1, e2))));
  const WorldTri w = world_triangle(S, i, inst);   // light_pdf's first lines, as in k_prepare_lights
  const rt3 edge1 = w.v1 - w.v0;
  const rt3 edge2 = w.v2 - w.v0;
  const rt3 cr = rt_cross(edge1, edge2);
  const float area = rt_length(cr) * 0.5f;
  const rt3 normal = rt_normalize(cr);
  tri_world[2 * i + 0] = make_float4(geom_n.x, geom_n.y, geom_n.z, area);
  tri_world[2 * i + 1] = make_float4(normal.x, normal.y, normal.z, 0.0f);
  const float4* ts = S.tri_shade + 8 * (size_t)i;
  float4* dst = tri_shade_w + 8 * (size_t)i;
  for (int k = 0; k < 4; k++) dst[k] = ts[k];
  for (int k = 4; k < 7; k++) {
    const float4 q = ts[k];
    const rt3 wn = rt_normalize(normal_to_world(m, xyz(q)));
    dst[k] = make_float4(wn.x, wn.y, wn.z, q.w);
  }
  dst[7] = ts[7];
}
__global__ void k_prepare_instances(const float4* __restrict__ inst, float4* __restrict__ inst_trav, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 c0 = inst[9 * i + 4], c1 = inst[9 * i + 5], c2 = inst[9 * i + 6], c3 = inst[9 * i + 7];
  float4 meta = inst[9 * i + 8];
  inst_trav[4 * i + 0] = make_float4(c0.x, c1.x, c2.x, c3.x);
  inst_trav[4 * i + 1] = make_float4(c0.y, c1.y, c2.y, c3.y);
  inst_trav[4 * i + 2] = make_float4(c0.z, c1.z, c2.z, c3.z);
  inst_trav[4 * i + 3] = make_float4(meta.x, c0.w, c1.w, c2.w);
}

// ================================================================ primary visibility
// LDS = false: one wave (one 8x8 tile) per workgroup, records through L1 / L2.  LDS = true (small scenes): 256-thread
// workgroups, one wave per tile, and the records staged in LDS first — the walk is a chain of dependent fetches, and an LDS
// fetch returns in a fraction of an L1 hit's time.  The launch's dynamic LDS: launch_plan.h primary_lds_slots.
// TILES = true (an LDS form, k_primary_visibility_tiles): a wave casts `rounds` tiles one after the other, tile primary_tile(blockIdx.x, rounds, r, wave)
// in round r (lds_sizes.h), so that the staging, the barrier, everything that depends on the dispatch alone and the counter
// flush are paid once per wave, not once per tile.  It is the form of an unstriped dispatch of a one-leaf scene (the TLAS is
// one node, a leaf: launch_plan.h one_leaf_lds), which is what keeps it inside the registers of eight waves per SIMD: no
// TLAS loop around the walk of the one instance, none of the stripe tests and their reciprocals, and what is read once per
// wave lives in scalar registers: at most 96 of them (amdgpu_num_sgpr on k_primary_visibility_tiles alone), which is what
// eight waves per SIMD may have; left to itself the compiler takes 105 and the form runs at seven.  launch_plan.h
// primary_shape chooses the form and rounds, primary_grid_x the grid.
// Results do not depend on where these values live; the eighth wave does.  Both devices below were needed with the
// compiler of ROCm 7.2.0 (AMD clang 22.0.0git, roc-7.2.0) and are held by tests/test_kernel_resources_primary.py (VGPRs,
// SGPRs, spills, waves per SIMD): with another compiler, look there first.
//
// A value every lane of the wave holds alike, kept in a scalar register from here on.  `zero` is 0 in every lane in a way
// the compiler does not see through: it moves a readfirstlane of a value it can prove uniform back in front of the
// arithmetic that made it, which leaves the result in a vector register.
__device__ __forceinline__ float wave_uniform(float x, uint32_t zero = 0u) {
  return rt_u2f((uint32_t)__builtin_amdgcn_readfirstlane((int)(rt_f2u(x) | zero)));
}
__device__ __forceinline__ float4 wave_uniform(float4 q) {
  return make_float4(wave_uniform(q.x), wave_uniform(q.y), wave_uniform(q.z), wave_uniform(q.w));
}
template <bool DETAIL, bool LDS, bool TILES>
__device__ __forceinline__ void primary_visibility(DevScene Sg, DevFrame F, rt_scene_uniforms U, const DevFrameSlot* __restrict__ slots,
                                                   uint32_t n_tiles, uint32_t n_nodes_total, uint32_t n_tris_total,
                                                   uint32_t n_inst_total, const float4* __restrict__ tri_shade_w, uint32_t rounds) {
  static_assert(LDS || !TILES, "the form of many tiles per wave is an LDS form");
  // tri_shade_w (LDS form, one-leaf-TLAS scenes; else null): the shading records with world-space vertex normals
  // (k_prepare_world_tris), staged in place of tri_shade
  extern __shared__ float4 s_primary[];
  DevScene S = Sg;
  if (LDS) {
    float4* dst = s_primary;
    auto stage = [&](const void* src, size_t slots_n) {
      const float4* g = reinterpret_cast<const float4*>(src);
      float4* base = dst;
      for (uint32_t i = threadIdx.x; i < slots_n; i += 256) base[i] = g[i];
      dst += slots_n;
      return base;
    };
    S.nodes = stage(Sg.nodes, (size_t)2 * n_nodes_total);
    S.tri_geom = stage(Sg.tri_geom, (size_t)RT_TRI_STRIDE * n_tris_total);
    S.inst_trav = stage(Sg.inst_trav, (size_t)4 * n_inst_total);
    S.tri_shade = stage(tri_shade_w ? tri_shade_w : Sg.tri_shade, (size_t)8 * n_tris_total);
    __syncthreads();
  }
  const uint32_t wave = TILES ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : threadIdx.x >> 6;
  const uint32_t lane_id = threadIdx.x & 63u;
  const uint32_t n_rounds = TILES ? rounds : 1u;
  const uint32_t first_tile = LDS ? primary_tile(blockIdx.x, n_rounds, 0u, wave) : blockIdx.x;
  // batched dispatch: blockIdx.y selects the frame; its jitter and G-buffer planes come from the slot table
  if (slots) {
    const DevFrameSlot sl = slots[blockIdx.y];
    U.frame_count = sl.frame_count;
    U.jitter[0] = sl.jitter_x;
    U.jitter[1] = sl.jitter_y;
    F.albedo = sl.albedo;
    F.normal_id = sl.normal_id;
    F.depth = sl.depth;
  }
  // What depends on the dispatch and the frame alone: every lane computes it from kernel arguments and the slot.
  const rt3 eye = rt3_make(U.camera.origin[0], U.camera.origin[1], U.camera.origin[2]);
  const rt3 ll = rt3_make(U.camera.lower_left[0], U.camera.lower_left[1], U.camera.lower_left[2]);
  const rt3 hor = rt3_make(U.camera.horizontal[0], U.camera.horizontal[1], U.camera.horizontal[2]);
  const rt3 ver = rt3_make(U.camera.vertical[0], U.camera.vertical[1], U.camera.vertical[2]);
  const rt3 center = ll + hor * 0.5f + ver * 0.5f;
  float focal_length = rt_length(center - eye);
  const float z_near = 0.001f, z_far = 10000.0f;
  float t_near = z_near / focal_length, t_far = z_far / focal_length;
  float width_f = (float)U.width, height_f = (float)U.height;
  float jitter_x = U.jitter[0] * width_f, jitter_y = U.jitter[1] * height_f;
  TlasLeaf leaf = {};
  if (TILES) {
    const uint32_t zero = (threadIdx.x >> 6) ^ wave;
    focal_length = wave_uniform(focal_length, zero);
    t_near = wave_uniform(t_near, zero);
    t_far = wave_uniform(t_far, zero);
    width_f = wave_uniform(width_f, zero);
    height_f = wave_uniform(height_f, zero);
    jitter_x = wave_uniform(jitter_x, zero);
    jitter_y = wave_uniform(jitter_y, zero);
    if (U.blas_base_idx != 0u) {   // node 0, the TLAS leaf, and the rows of the one instance it names
      leaf.lo = wave_uniform(S.nodes[0]);
      leaf.hi = wave_uniform(S.nodes[1]);
      const InvRows m = load_inv_rows(S, rt_f2u(leaf.hi.w) >> 3);
      leaf.m.r0 = wave_uniform(m.r0);
      leaf.m.r1 = wave_uniform(m.r1);
      leaf.m.r2 = wave_uniform(m.r2);
      leaf.m.tail = wave_uniform(m.tail);
    }
  }
  uint32_t n_live = 0;   // TILES: pixels cast by this wave (wave-uniform)
  LaneCounters c = {0, 0, 0, 0, 0, 0};
  for (uint32_t r = 0; r < n_rounds; r++) {
    const uint32_t tile_id = first_tile + 4u * r;   // = primary_tile(blockIdx.x, n_rounds, r, wave)
    if (TILES && tile_id >= n_tiles) break;         // wave-uniform; the rounds after it lie higher still
    uint32_t x, y;
    bool live;
    if (!TILES && F.own_period) {
      // sharded render with tile-aligned stripes: blockIdx.x enumerates only the tiles of the rows this rank owns
      const uint32_t tiles_x = (U.width + 7u) / 8u;
      uint32_t trow = tile_id / tiles_x;
      trow = (trow / F.own_run) * F.own_period + F.own_first + (trow % F.own_run);
      x = (tile_id % tiles_x) * 8u + (lane_id & 7u);
      y = trow * 8u + (lane_id >> 3);
      live = x < U.width && y < U.height;
    } else {
      live = tile_pixel(U, tile_id, lane_id, x, y) && (TILES || owns_row(F, y));
    }
    live = live && tile_id < n_tiles;
    if (TILES)
      n_live += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(live));
    else if (live)
      c.primary = 1;
    if (!live) continue;
    const uint32_t p_idx = y * U.width + x;
    float u = ((float)x + 0.5f + jitter_x) / width_f;
    float v = 1.0f - ((float)y + 0.5f + jitter_y) / height_f;
    rt3 d = ll + u * hor + v * ver - eye;
    const HitUV hv = trace_closest_uv<DETAIL, TILES>(S, U.blas_base_idx, eye, d, t_near, t_far, c, leaf);
    const Hit hit = hv.hit;
    if (hit.inst < 0) {
      F.albedo[p_idx] = 0u;
      F.normal_id[p_idx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      F.depth[p_idx] = 1.0f;
    } else {
      // u and v of the accepted triangle test are the barycentrics of the hit (trace_closest_uv)
      const float b_u = hv.u, b_v = hv.v, b_w = 1.0f - hv.u - hv.v;
      const float4* ts = S.tri_shade + 8 * (size_t)hit.tri;
      const float4 d0 = ts[0], d2 = ts[2], q4 = ts[4], q5 = ts[5], q6 = ts[6], q7 = ts[7];
      rt3 wn0 = xyz(q4), wn1 = xyz(q5), wn2 = xyz(q6);
      if (!LDS || !tri_shade_w) {   // wave-uniform
        const InvRows m = TILES ? leaf.m : load_inv_rows(S, (uint32_t)hit.inst);
        wn0 = rt_normalize(normal_to_world(m, wn0));
        wn1 = rt_normalize(normal_to_world(m, wn1));
        wn2 = rt_normalize(normal_to_world(m, wn2));
      }
      rt3 n = rt_normalize(wn0 * b_w + wn1 * b_u + wn2 * b_v);
      rt2 pn = pack_normal(n);
      rt3 albedo = xyz(d0);
      if (d2.x > -0.5f) {
        rt2 tuv = rt2_make(q4.w, q5.w) * b_w + rt2_make(q6.w, q7.x) * b_u + rt2_make(q7.y, q7.z) * b_v;
        albedo = albedo * sample_tex(S, tuv, rt_f2i32_sat(d2.x));
      }
      F.albedo[p_idx] = rt_unorm8(albedo.x) | (rt_unorm8(albedo.y) << 8) | (rt_unorm8(albedo.z) << 16) | (255u << 24);
      F.normal_id[p_idx] = make_float4(pn.x, pn.y, rt_u2f((uint32_t)hit.tri), rt_u2f((uint32_t)hit.inst));
      float z_view = hit.t * focal_length;
      float z_clip = z_view * (z_far / (z_far - z_near)) - (z_far * z_near) / (z_far - z_near);
      F.depth[p_idx] = z_clip / z_view;
    }
  }
  if (TILES) c.primary = lane_id == 0u ? n_live : 0u;   // the wave's sum is what the flush adds
  flush_counters<DETAIL>(c, F.counters, first_tile + blockIdx.y * 977u);
}
// The forms of one tile per wave; `rounds` is not read.
template <bool DETAIL, bool LDS>
__global__ __launch_bounds__(LDS ? 256 : 64) void k_primary_visibility(DevScene Sg, DevFrame F, rt_scene_uniforms U,
                                                                       const DevFrameSlot* __restrict__ slots, uint32_t n_tiles,
                                                                       uint32_t n_nodes_total, uint32_t n_tris_total,
                                                                       uint32_t n_inst_total, uint32_t n_verts_total,
                                                                       const float4* __restrict__ tri_shade_w, uint32_t rounds) {
  primary_visibility<DETAIL, LDS, false>(Sg, F, U, slots, n_tiles, n_nodes_total, n_tris_total, n_inst_total, tri_shade_w, rounds);
}
// The form of many tiles per wave, alone under the cap of 96 scalar registers (above).
template <bool DETAIL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(96))) void k_primary_visibility_tiles(
    DevScene Sg, DevFrame F, rt_scene_uniforms U, const DevFrameSlot* __restrict__ slots, uint32_t n_tiles, uint32_t n_nodes_total,
    uint32_t n_tris_total, uint32_t n_inst_total, uint32_t n_verts_total, const float4* __restrict__ tri_shade_w, uint32_t rounds) {
  primary_visibility<DETAIL, true, true>(Sg, F, U, slots, n_tiles, n_nodes_total, n_tris_total, n_inst_total, tri_shade_w, rounds);
}

}  // namespace rtk
#endif
