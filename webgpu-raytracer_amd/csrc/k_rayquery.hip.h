// k_rayquery.hip.h — k_ray_query: ray casts against the uploaded scene for the host (rt_trace_rays, mi355rt.h).
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_RAYQUERY_HIP_H
#define MI355RT_K_RAYQUERY_HIP_H

namespace rtk {

// The trace kernels of the wavefront form with another ray source: persistent waves with ray-level regeneration
// (wf_trace_loop, k_wavefront.hip.h) over a caller's flat array of rt_ray {o, t_max} {d, -} — the queue record of the
// trace kernels — and a flat array of rt_ray_hit, one 16-byte result at the ray's own index.  The walks, the triangle
// flush and the staging are the ones the render kernels run (WfNodeWalk / WfPairWalk, tri_flush, trav_stage_mixed,
// pw_stage): nothing of them is restated here.  What differs from a render launch: t_max is per ray for closest-hit rays
// too, and t_min is the caller's (TravMem::t_min / PairMem::t_min).
// A wave takes RT_RQ_CHUNK consecutive rays per atomic and its lanes pull them in order, so a caller's coherent ray order
// (pixels of a row, texels of a bake) stays together in a wave.
// Termination for ANY bit pattern of a ray: the node walk only ever moves to a successor, which k_validate_scene has
// checked to be a larger index or the end mark, so it takes at most one step per node and instance; the pair walk's
// stack is finite and its stackless fall-back follows the same forward order.  A NaN or infinite component decides slab
// and triangle tests one way or the other, never the number of steps.
#ifndef RT_RQ_CHUNK
#define RT_RQ_CHUNK 128u   // rays per atomic: 1920 x 1080 rays are 16 200 chunks for at most 6 144 resident waves
#endif

struct RayQueryArgs {
  const float4* rays;   // 2 per ray
  uint4* out;           // 1 per ray: {bits(t), tri, inst, hit}
  uint32_t* head;       // chunk counter, zeroed by the host before the launch
  uint64_t* counters;   // RT_COUNTER_SHARDS x 6, the query's own (flush_counters)
  uint32_t n_rays, blas_base;
  float t_min;
  uint32_t n_recs, n_tris, n_inst;   // nodes (node walk) or pair records (pair walk), triangles, instances
};

template <bool ANY>
struct RayQueryIO;
struct RayQuerySrc {
  template <bool ANY>
  using IO = RayQueryIO<ANY>;
  const RayQueryArgs& A;
  __device__ __forceinline__ uint32_t blas_base() const { return A.blas_base; }
  __device__ __forceinline__ uint64_t* counters() const { return A.counters; }
};
template <bool ANY>
struct RayQueryIO {
  static constexpr uint32_t CHUNK = RT_RQ_CHUNK;
  const float4* rays;
  uint4* out;
  uint32_t n_rays;
  uint32_t* head;
  __device__ __forceinline__ explicit RayQueryIO(const RayQuerySrc& src) : rays(src.A.rays), out(src.A.out), n_rays(src.A.n_rays), head(src.A.head) {}
  __device__ __forceinline__ bool valid(uint32_t) const { return true; }
  __device__ __forceinline__ float4 ray0(uint32_t qi) const { return rays[2 * qi]; }       // {o, t_max}
  __device__ __forceinline__ float4 ray1(uint32_t qi) const { return rays[2 * qi + 1]; }   // {d, -}
  static __device__ __forceinline__ float t_max(float4 r0) { return r0.w; }
  // closest hit: the walk's bound is the ray's t_max until a hit replaces it, so a miss hands the caller's bits back
  template <class WALK>
  __device__ __forceinline__ void store(uint32_t slot, const typename WALK::Lane& s) const {
    if (ANY) {
      // (rt_opaque: the two constants are made here, where the store needs them; hoisted out of the trace loop they
      // occupy two registers through the whole walk, which the RAYREG counting form does not have)
      const uint32_t none = rt_f2u(rt_opaque(rt_u2f(0xffffffffu)));
      out[slot] = make_uint4(rt_f2u(rt_opaque(0.0f)), none, none, WALK::occluded(s) ? 1u : 0u);
    } else
      out[slot] = make_uint4(rt_f2u(s.closest), (uint32_t)s.best_tri, (uint32_t)s.best_inst, s.best_tri != -1 ? 1u : 0u);
  }
};

// FORM: the five forms of the 256-thread trace kernels, RT_RQ_* of lds_sizes.h (launch_plan.h trace_shape picks as it does for
// k_wf_trace / k_wf_trace_pairs)

// Waves per SIMD asked of the compiler: those of the wavefront kernel of the same form — except the plain mixed node walk
// without counting, where k_wf_trace comes out at 72 VGPRs (7 waves) under a bound of 6 and the per-ray t_max of a
// closest-hit query costs this kernel a 73rd: asked for 7, it fits 72 without a spill
// (tests/test_kernel_resources_ray_query.py).
template <bool DETAIL, int FORM>
constexpr int rq_waves() {
  return (FORM == RT_RQ_NODE_LDS || FORM == RT_RQ_PAIR_LDS) ? 4
         : FORM >= RT_RQ_PAIR_LDS                           ? RT_WF_WAVES
         : (FORM == RT_RQ_NODE_MIXED && !DETAIL)            ? RT_WF_NODE_WAVES + 1
                                                            : RT_WF_NODE_WAVES;
}
template <bool ANY, bool DETAIL, int FORM>
__global__ __launch_bounds__(256, (rq_waves<DETAIL, FORM>()))
void k_ray_query(DevScene Sg, RayQueryArgs A, LdsPlan nplan, PairPlan pplan) {
  extern __shared__ f4 s_scene[];
  constexpr bool PAIRS = FORM >= RT_RQ_PAIR_LDS, LDS = FORM == RT_RQ_NODE_LDS || FORM == RT_RQ_PAIR_LDS;
  WaveWork W;
  if constexpr (PAIRS) {
    wave_work_at(W, reinterpret_cast<char*>(s_scene) + (threadIdx.x >> 6) * RT_PW_BYTES_PER_WAVE);
    const uint32_t rec0 = (4 * RT_PW_BYTES_PER_WAVE) / 16;
    PairMem M;
    PairPlan plan = pplan;
    if (LDS) plan.stage_pairs = plan.stage_inst = plan.stage_tri = 1u;
    pw_stage(M, s_scene, rec0, Sg, plan, A.n_recs, A.n_tris, A.n_inst, A.t_min);
    __syncthreads();
    wf_trace_loop<WfPairWalk<ANY, DETAIL, LDS>, 256>(M, s_scene, W, RayQuerySrc{A});
  } else {
    wave_work_at(W, reinterpret_cast<char*>(s_scene) + (threadIdx.x >> 6) * RT_WORK_BYTES_PER_WAVE);
    const uint32_t rec0 = (4 * RT_WORK_BYTES_PER_WAVE) / 16;
    TravMem M;
    LdsPlan plan = nplan;
    if (LDS) {
      plan.k_nodes = A.n_recs;
      plan.stage_inst = plan.stage_tri = 1u;
    }
    trav_stage_mixed(M, s_scene, rec0, Sg, plan, A.n_tris, A.n_inst);
    M.t_min = A.t_min;
    __syncthreads();
    constexpr int MODE = LDS ? RT_TRAV_LDS : (FORM == RT_RQ_NODE_RAYREG ? RT_TRAV_MIXED_RAYREG : RT_TRAV_MIXED);
    wf_trace_loop<WfNodeWalk<ANY, DETAIL, MODE>, 256>(M, s_scene, W, RayQuerySrc{A});
  }
}

}  // namespace rtk
#endif
