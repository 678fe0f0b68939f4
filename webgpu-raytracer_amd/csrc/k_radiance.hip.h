// k_radiance.hip.h — path_query_loop: the persistent loop behind the path queries, and its first kind, k_radiance_query: the
// radiance that arrives along a caller's rays (rt_trace_radiance, mi355rt.h).  The second kind, k_irradiance_gather, is in
// k_gather.hip.h.
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_RADIANCE_HIP_H
#define MI355RT_K_RADIANCE_HIP_H

namespace rtk {

// ============================================================ the shared loop
// A path query drives the per-path state machine (setup_surface / shade_bounce, k_pathtrace.hip.h), as k_pathtrace,
// k_pathtrace_persistent and k_wf_shade do, over a caller's flat array of ITEMS, two float4 each {x, y, z, t_max}
// {x, y, z, pad} (rt_ray, rt_gather_point), and writes one float4 {r, g, b, w} per item.  Every item gets spp samples;
// sample s runs with rng = init_rng(pad, seed * spp + s), its first segment is the closest hit in (RT_T_MIN, the item's
// t_max) and counts as one extension ray, its depth-0 surface is taken from that TRACED hit the way every later depth takes
// it (Raytracer.wgsl:738-779, setup_surface(.., from_gbuffer = false, ..)): no G-buffer, no octahedral normal, no unorm8
// albedo, no lens offset, no jitter.  Every later segment uses RT_T_MIN / RT_T_MAX and the shadow rays are those of
// shade_bounce, as in a frame.  rgb = (((0 + r_0) + r_1) + ...) in sample order, divided by spp as finish_pixel does (not
// at all for spp == 1).  With max_depth == 0 the first segments are still traced and nothing is shaded (shade_bounce would
// compute max_depth - 1u).
// Scheduling is the persistent kernel's: persistent waves, a chunk of RT_RAD_CHUNK consecutive items per atomic, idle lanes
// take the next unassigned item of the wave's chunk (ballot / prefix count), and per trip every live lane executes one
// bounce, so the wave runs both traversals and the shading code converged, with ONE call site per walk: the extension
// walk also traces the first segments (per-lane t_max).  A lane keeps its item for all spp samples.  Paths are
// independent and traversal draws no random number, so a result depends on (scene, item, seed, spp, max_depth) only.
// LDS = true: the whole scene is staged, traversal records and shading arrays (stage_whole_scene: the persistent kernel's
// non-ONE_INST LDS form); otherwise trav_stage_mixed with the host's plan.  There is no one-leaf / world-record form yet.
//
// ITEM is the kind's policy (RadianceItem below, GatherItem in k_gather.hip.h), in the style of RayQueryIO.  It holds what a
// lane keeps of its item beside the PathState, and says only what differs between the kinds:
//   static constexpr bool FIRST_SEG_PER_SAMPLE
//                         a first segment that ends without a surface to shade (a miss, or a hit with max_depth == 0) ends
//                         the sample, which is then a sample of +0 (true), or ends the whole item, of which no sample has
//                         run (false)
//   void take()           the lane has taken a new item
//   bool start_sample(r1, pad, f, p)
//                         start sample f = seed * spp + s of the item whose second record is r1: set the direction p.rd, and
//                         either return true (the first segment is to be traced) or put a kept first hit into p.hit_t /
//                         p.tri / p.inst and return false
//   void first_hit(t, tri, inst), void first_miss(t)
//                         what the sample's first segment found; a miss hands the bound back (the bits of the item's t_max)
//   float w(spp)          the fourth word of the item's result
#ifndef RT_RAD_CHUNK
#define RT_RAD_CHUNK 64u   // items per atomic: the persistent kernel's 8 x 8 tile
#endif

struct PathQueryArgs {
  const float4* items;  // 2 per item
  float4* out;          // 1 per item: {r, g, b, ITEM::w}
  uint32_t* head;       // chunk counter, zeroed by the host before the launch
  uint64_t* counters;   // RT_COUNTER_SHARDS x 6, the query's own (flush_counters)
  uint32_t n_items, max_depth, spp, seed;
  uint32_t light_count, blas_base;
  uint32_t n_nodes, n_tris, n_inst, n_verts;
};

template <class ITEM, bool DETAIL, bool LDS>
__device__ __forceinline__ void path_query_loop(DevScene Sg, PathQueryArgs A, LdsPlan plan) {
  constexpr uint32_t WAVES = 4;
  extern __shared__ f4 s_scene[];
  // per-wave triangle work queue at the start of LDS, staged scene after it
  const uint32_t wave = threadIdx.x >> 6;
  WaveWork WW;
  wave_work_at(WW, reinterpret_cast<char*>(s_scene) + wave * RT_WORK_BYTES_PER_WAVE);
  const uint32_t rec0 = (WAVES * RT_WORK_BYTES_PER_WAVE) / 16;
  TravMem M;
  DevScene S = Sg;
  if (LDS)
    stage_whole_scene(M, S, s_scene, rec0, Sg, A.n_nodes, A.n_tris, A.n_inst, A.n_verts);
  else
    trav_stage_mixed(M, s_scene, rec0, Sg, plan, A.n_tris, A.n_inst);
  __syncthreads();
  constexpr int MODE = LDS ? RT_TRAV_LDS : RT_TRAV_MIXED;

  const uint32_t lane = threadIdx.x & 63u;
  // wave-uniform work cursor: items [chunk_pos, chunk_end) of the wave's chunk are still unassigned
  uint32_t chunk_pos = 0u, chunk_end = 0u;
  bool work_left = true;

  PathState p = idle_path();   // p.pixel: the lane's item; p.col: its sample sum
  ITEM item;
  bool have_item = false;      // lane owns an item whose samples are not all done
  bool alive = false;          // lane owns a running sample
  bool first_seg = false;      // ... whose ray (p.ro, p.rd; t_max in p.hit_t) is the first segment, still to be traced
  // cnt_ext, cnt_shadow: rays of the whole wave, wave-uniform (scalar registers); the others count per lane
  uint32_t cnt_ext = 0, cnt_shadow = 0, cnt_nodes = 0, cnt_tris = 0, cnt_shaded = 0;

  for (;;) {
    // ------------------------------------------------------------ regenerate
    // (a) wave-wide: every lane without an item takes the next unassigned one of the wave's chunk.  All lanes execute this
    //     loop (busy lanes with need = false) so that the wave-uniform cursor stays identical in every lane.
    {
      bool need = !have_item;
      for (;;) {
        const unsigned long long mask = __ballot(need);
        if (mask == 0ull || !work_left) break;
        if (chunk_pos >= chunk_end) {
          const int leader = __builtin_ctzll(mask);
          uint32_t t = 0;
          if (lane == (uint32_t)leader) t = atomicAdd(A.head, 1u);
          t = __shfl(t, leader, 64);
          // n_items < 2^31 (the host refuses more) and at most one overshoot per wave: t * RT_RAD_CHUNK stays below 2^32
          if (t >= (A.n_items + RT_RAD_CHUNK - 1u) / RT_RAD_CHUNK) {
            work_left = false;
            break;
          }
          chunk_pos = t * RT_RAD_CHUNK;
          chunk_end = min(chunk_pos + RT_RAD_CHUNK, A.n_items);
        }
        // rank of this lane among the needy lanes
        const uint32_t rank =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        const uint32_t idx = chunk_pos + rank;
        if (need && idx < chunk_end) {
          need = false;
          have_item = true;
          p.pixel = idx;
          p.sample = 0u;
          p.col = rt3_splat(0.0f);
          item.take();
        }
        chunk_pos += (uint32_t)__builtin_popcountll(mask);   // past chunk_end: the chunk is used up
      }
    }
    // (b) start the next sample of the owned item: the item is read again from the array (the path has overwritten the
    //     ray), and the depth-0 surface comes from a kept first hit, or the first segment joins this trip's extension walk
    if (!alive && have_item) {
      const float4 r0 = A.items[2 * (size_t)p.pixel], r1 = A.items[2 * (size_t)p.pixel + 1];
      const uint32_t pad = rt_f2u(r1.w), f = A.seed * A.spp + p.sample;
      p.rng = init_rng(pad, f);
      p.ro = xyz(r0);
      const bool trace_first = item.start_sample(r1, pad, f, p);
      p.throughput = rt3_splat(1.0f);
      p.radiance = rt3_splat(0.0f);
      p.prev_pdf = 0.0f;
      p.specular = true;
      p.depth = 0u;
      alive = true;
      if (trace_first) {
        first_seg = true;
        p.hit_t = r0.w;   // no surface yet: the slot carries the segment's t_max to the walk
      } else {
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
    bool item_done = false;   // the item ends in this trip
    // what a first segment ends when it leaves no surface to shade (a miss, or max_depth == 0): the sample or the item
    bool& unshaded = ITEM::FIRST_SEG_PER_SAMPLE ? path_done : item_done;
    const unsigned long long extend_mask = __ballot(want_extend);
    if (extend_mask != 0ull) {
      cnt_ext += (uint32_t)__builtin_popcountll(extend_mask);
      float t_;
      int32_t tri_, inst_;
      bool any_;
      traverse<false, DETAIL, MODE>(M, s_scene, WW, A.blas_base, want_extend, p.ro, p.rd, first_seg ? p.hit_t : RT_T_MAX, t_, tri_,
                                    inst_, any_, cnt_nodes, cnt_tris);
      if (want_extend) {   // (path_done is still false here: shade_bounce asks for an extension ray or ends the path)
        if (inst_ < 0) {
          if (first_seg) {
            item.first_miss(t_);
            unshaded = true;
          } else {
            path_done = true;
          }
        } else {
          p.hit_t = t_;
          p.tri = (uint32_t)tri_;
          p.inst = (uint32_t)inst_;
          if (first_seg) {
            item.first_hit(t_, (uint32_t)tri_, (uint32_t)inst_);
            if (A.max_depth == 0u) unshaded = true;
          } else {
            p.depth++;
          }
          if (!unshaded) setup_surface(S, p, false, 0.0f, 0.0f, 0u);
        }
        first_seg = false;
      }
    }

    // ------------------------------------------------------------ sample / item finished
    if (path_done) {
      alive = false;
      p.col = p.col + p.radiance;
      p.sample++;
      if (p.sample >= A.spp) {  // the item's last sample
        if (A.spp != 1u) p.col = rt_div3z(p.col, (float)A.spp);   // finish_pixel's average
        item_done = true;
      }
    }
    if (item_done) {   // p.col is +0 when no sample ran
      alive = false;
      have_item = false;
      A.out[p.pixel] = make_float4(p.col.x, p.col.y, p.col.z, item.w(A.spp));
    }
    if (!work_left && __ballot(have_item) == 0ull) break;
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

// ============================================================ radiance queries
// The item is a ray, rt_ray {o, t_max} {d, pad}, and the result an rt_radiance {r, g, b, t}.  Sample s of ray i is ray_color
// (Raytracer.wgsl:607-783) with rng = init_rng(pad, seed * spp + s) and the depth-0 surface taken from the TRACED hit:
//  * the first segment is the closest hit in (RT_T_MIN, the ray's t_max); it does not depend on the sample, so it is
//    traced once per ray and counts as one extension ray.  Its (t, tri, inst) is kept in three registers and the surface
//    frame is made again at the start of every sample, because shade_bounce flips the normals in place;
//  * every later segment uses RT_T_MIN / RT_T_MAX and the shadow rays are those of shade_bounce, as in a frame;
//  * rgb = (((0 + r_0) + r_1) + ...) in sample order, divided by spp as finish_pixel does (not at all for spp == 1);
//    t = the first segment's distance; a miss is {+0, +0, +0, the bits of the ray's t_max};
//  * max_depth == 0: the first segment is traced and t reported, nothing is shaded (shade_bounce would compute
//    max_depth - 1u).
// A result depends on (scene, ray, pad, seed, spp, max_depth) only.
struct RadianceItem {
  static constexpr bool FIRST_SEG_PER_SAMPLE = false;
  static constexpr uint32_t NO_HIT = 0xffffffffu;   // first_inst of a ray whose first segment is not traced yet
  float first_t = 0.0f;                             // the first segment's hit, kept for the ray's later samples
  uint32_t first_tri = 0u, first_inst = NO_HIT;
  __device__ __forceinline__ void take() { first_inst = NO_HIT; }
  __device__ __forceinline__ bool start_sample(const float4& r1, uint32_t, uint32_t, PathState& p) const {
    p.rd = xyz(r1);
    if (first_inst == NO_HIT) return true;
    p.hit_t = first_t;
    p.tri = first_tri;
    p.inst = first_inst;
    return false;
  }
  __device__ __forceinline__ void first_hit(float t, uint32_t tri, uint32_t inst) {
    first_t = t;
    first_tri = tri;
    first_inst = inst;
  }
  __device__ __forceinline__ void first_miss(float t) { first_t = t; }
  __device__ __forceinline__ float w(uint32_t) const { return first_t; }
};

template <bool DETAIL, bool LDS>
__global__ __launch_bounds__(256, LDS ? RT_PT_LDS_WAVES : RT_PT_GLOBAL_WAVES)
void k_radiance_query(DevScene Sg, PathQueryArgs A, LdsPlan plan) {
  path_query_loop<RadianceItem, DETAIL, LDS>(Sg, A, plan);
}

}  // namespace rtk
#endif
