// k_gather.hip.h — k_irradiance_gather: the cosine-weighted mean radiance that arrives at a caller's surface points
// (rt_gather_irradiance, mi355rt.h).
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_GATHER_HIP_H
#define MI355RT_K_GATHER_HIP_H

namespace rtk {

// The fifth driver of the per-path state machine (setup_surface / shade_bounce, k_pathtrace.hip.h), the twin of
// k_radiance_query (k_radiance.hip.h).  Its work item is a surface point, rt_gather_point {position, t_max} {normal, pad},
// and its result one rt_irradiance {r, g, b, hit_fraction} per point.  For sample s of point i, f = seed * spp + s:
//  * the direction is sample_diffuse(rt_normalize(normal), ., rng_d).dir with rng_d = init_rng(pad ^ 0x80000000u, f), a
//    stream of its own, and is not normalised again;
//  * the sample is what k_radiance_query returns for the ray {position, t_max, that direction, pad} with spp = 1 and
//    seed = f: rng = init_rng(pad, f), first segment = closest hit in (RT_T_MIN, t_max), depth-0 surface from the traced hit,
//    later segments RT_T_MIN / RT_T_MAX, shadow rays those of shade_bounce;
//  * rgb = (((0 + r_0) + r_1) + ...) in sample order, divided by spp as finish_pixel does (not at all for spp == 1): the
//    cosine-weighted mean incoming radiance, E / pi;  hit_fraction = rt_div(hits, spp), hits = the samples whose first
//    segment hit something;
//  * max_depth == 0: every first segment is still traced, nothing is shaded, rgb = +0 (1 - hit_fraction is ambient
//    occlusion of radius t_max).
// Every sample has a first segment of its own, so unlike the twin nothing of a first hit is kept: the point is read again at
// the start of every sample, the direction is made there, and the segment rides in that trip's extension walk with the
// point's t_max.  Each first segment counts as one extension ray, which makes the counters of a gather the sums of the
// counters of the radiance queries it is composed of.
// Scheduling is the twin's: persistent waves, a chunk of RT_RAD_CHUNK consecutive points per atomic, idle lanes take the
// next unassigned point of the wave's chunk (ballot / prefix count), one shade step, one any-hit walk and one closest-hit
// walk per trip with ONE call site per walk.  A lane keeps its point for all spp samples (few points with a very large spp
// fill few lanes: replicate the point with different pads and average).  A result depends on (scene, point, pad, seed,
// spp, max_depth) only.
// LDS = true: the whole scene is staged (the persistent kernel's non-ONE_INST LDS form); otherwise trav_stage_mixed with the
// host's plan.  There is no one-leaf / world-record form.
#define RT_GATHER_DIR_STREAM 0x80000000u   // pad ^ this = the stream id of a point's directions

struct GatherArgs {
  const float4* points; // 2 per point
  float4* out;          // 1 per point: {r, g, b, hit_fraction}
  uint32_t* head;       // chunk counter, zeroed by the host before the launch
  uint64_t* counters;   // RT_COUNTER_SHARDS x 6, the query's own (flush_counters)
  uint32_t n_points, max_depth, spp, seed;
  uint32_t light_count, blas_base;
  uint32_t n_nodes, n_tris, n_inst, n_verts;
};

template <bool DETAIL, bool LDS>
__global__ __launch_bounds__(256, LDS ? RT_PT_LDS_WAVES : RT_PT_GLOBAL_WAVES)
void k_irradiance_gather(DevScene Sg, GatherArgs A, LdsPlan plan) {
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
    // the slots of scene_lds_slots, in the persistent kernel's order (k_radiance_query's block)
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

  const uint32_t lane = threadIdx.x & 63u;
  // wave-uniform work cursor: points [chunk_pos, chunk_end) of the wave's chunk are still unassigned
  uint32_t chunk_pos = 0u, chunk_end = 0u;
  bool work_left = true;

  PathState p = idle_path();   // p.pixel: the lane's point; p.col: its sample sum
  bool have_point = false;     // lane owns a point whose samples are not all done
  bool alive = false;          // lane owns a running sample
  bool first_seg = false;      // ... whose ray (p.ro, p.rd; t_max in p.hit_t) is the first segment, still to be traced
  uint32_t hits = 0u;          // samples of the lane's point whose first segment hit something
  // cnt_ext, cnt_shadow: rays of the whole wave, wave-uniform (scalar registers); the others count per lane
  uint32_t cnt_ext = 0, cnt_shadow = 0, cnt_nodes = 0, cnt_tris = 0, cnt_shaded = 0;

  for (;;) {
    // ------------------------------------------------------------ regenerate
    // (a) wave-wide: every lane without a point takes the next unassigned one of the wave's chunk.  All lanes execute this
    //     loop (busy lanes with need = false) so that the wave-uniform cursor stays identical in every lane.
    {
      bool need = !have_point;
      for (;;) {
        const unsigned long long mask = __ballot(need);
        if (mask == 0ull || !work_left) break;
        if (chunk_pos >= chunk_end) {
          const int leader = __builtin_ctzll(mask);
          uint32_t t = 0;
          if (lane == (uint32_t)leader) t = atomicAdd(A.head, 1u);
          t = __shfl(t, leader, 64);
          // n_points < 2^31 (the host refuses more) and at most one overshoot per wave: t * RT_RAD_CHUNK stays below 2^32
          if (t >= (A.n_points + RT_RAD_CHUNK - 1u) / RT_RAD_CHUNK) {
            work_left = false;
            break;
          }
          chunk_pos = t * RT_RAD_CHUNK;
          chunk_end = min(chunk_pos + RT_RAD_CHUNK, A.n_points);
        }
        // rank of this lane among the needy lanes
        const uint32_t rank =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        const uint32_t idx = chunk_pos + rank;
        if (need && idx < chunk_end) {
          need = false;
          have_point = true;
          p.pixel = idx;
          p.sample = 0u;
          p.col = rt3_splat(0.0f);
          hits = 0u;
        }
        chunk_pos += (uint32_t)__builtin_popcountll(mask);   // past chunk_end: the chunk is used up
      }
    }
    // (b) start the next sample of the owned point: the point is read again from the array (the path has overwritten the
    //     ray), the direction is drawn from the point's direction stream, and the first segment joins this trip's extension
    //     walk
    if (!alive && have_point) {
      const float4 r0 = A.points[2 * (size_t)p.pixel], r1 = A.points[2 * (size_t)p.pixel + 1];
      const uint32_t pad = rt_f2u(r1.w), f = A.seed * A.spp + p.sample;
      uint32_t rng_d = init_rng(pad ^ RT_GATHER_DIR_STREAM, f);
      p.rng = init_rng(pad, f);
      p.ro = xyz(r0);
      p.rd = sample_diffuse(rt_normalize(xyz(r1)), rt3_splat(0.0f), rng_d).dir;
      p.throughput = rt3_splat(1.0f);
      p.radiance = rt3_splat(0.0f);
      p.prev_pdf = 0.0f;
      p.specular = true;
      p.depth = 0u;
      alive = true;
      first_seg = true;
      p.hit_t = r0.w;   // no surface yet: the slot carries the segment's t_max to the walk
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
          path_done = true;   // a missed first segment is a sample of +0
        } else {
          p.hit_t = t_;
          p.tri = (uint32_t)tri_;
          p.inst = (uint32_t)inst_;
          if (first_seg) {
            hits++;
            if (A.max_depth == 0u) path_done = true;   // nothing is shaded (shade_bounce would compute max_depth - 1u)
          } else {
            p.depth++;
          }
          if (!path_done) setup_surface(S, p, false, 0.0f, 0.0f, 0u);
        }
        first_seg = false;
      }
    }

    // ------------------------------------------------------------ sample / point finished
    if (path_done) {
      alive = false;
      p.col = p.col + p.radiance;
      p.sample++;
      if (p.sample >= A.spp) {  // the point's last sample
        if (A.spp != 1u) p.col = rt_div3z(p.col, (float)A.spp);   // finish_pixel's average
        have_point = false;
        A.out[p.pixel] = make_float4(p.col.x, p.col.y, p.col.z, rt_div((float)hits, (float)A.spp));
      }
    }
    if (!work_left && __ballot(have_point) == 0ull) break;
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
