// k_gather.hip.h — k_irradiance_gather: the cosine-weighted mean radiance that arrives at a caller's surface points
// (rt_gather_irradiance, mi355rt.h).
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_GATHER_HIP_H
#define MI355RT_K_GATHER_HIP_H

namespace rtk {

// The second kind of path query: path_query_loop (k_radiance.hip.h) with the policy GatherItem.  Its work item is a surface
// point, rt_gather_point {position, t_max} {normal, pad}, and its result one rt_irradiance {r, g, b, hit_fraction} per point.
// For sample s of point i, f = seed * spp + s:
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
// Every sample has a first segment of its own, so unlike RadianceItem nothing of a first hit is kept: the point is read again
// at the start of every sample, the direction is made there, and the segment rides in that trip's extension walk with the
// point's t_max.  Each first segment counts as one extension ray, which makes the counters of a gather the sums of the
// counters of the radiance queries it is composed of.
// A lane keeps its point for all spp samples (few points with a very large spp fill few lanes: replicate the point with
// different pads and average).  A result depends on (scene, point, pad, seed, spp, max_depth) only.
#define RT_GATHER_DIR_STREAM 0x80000000u   // pad ^ this = the stream id of a point's directions

struct GatherItem {
  static constexpr bool FIRST_SEG_PER_SAMPLE = true;   // a missed first segment is a sample of +0
  uint32_t hits = 0u;                                  // samples of the lane's point whose first segment hit something
  __device__ __forceinline__ void take() { hits = 0u; }
  __device__ __forceinline__ bool start_sample(const float4& r1, uint32_t pad, uint32_t f, PathState& p) const {
    uint32_t rng_d = init_rng(pad ^ RT_GATHER_DIR_STREAM, f);
    p.rd = sample_diffuse(rt_normalize(xyz(r1)), rt3_splat(0.0f), rng_d).dir;
    return true;
  }
  __device__ __forceinline__ void first_hit(float, uint32_t, uint32_t) { hits++; }
  __device__ __forceinline__ void first_miss(float) {}
  __device__ __forceinline__ float w(uint32_t spp) const { return rt_div((float)hits, (float)spp); }
};

template <bool DETAIL, bool LDS>
__global__ __launch_bounds__(256, LDS ? RT_PT_LDS_WAVES : RT_PT_GLOBAL_WAVES)
void k_irradiance_gather(DevScene Sg, PathQueryArgs A, LdsPlan plan) {
  path_query_loop<GatherItem, DETAIL, LDS>(Sg, A, plan);
}

}  // namespace rtk
#endif
