// k_directional.hip.h — k_dir_rays and k_dir_project: the two kernels a directional gather (rt_gather_directional, mi355rt.h)
// puts around k_radiance_query, and k_dir_scatter: the way of its results back into the four layers of an atlas
// (rt_bake_atlas_directional).
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_DIRECTIONAL_HIP_H
#define MI355RT_K_DIRECTIONAL_HIP_H

namespace rtk {

// A directional gather is the probe gather's composition (k_probe.hip.h) at surface points: twelve accumulators across
// shade_bounce fit beside a PathState no better than 27 do, so the unit of path work is the (point, sample) pair:
//   k_dir_rays        one rt_ray per (point, sample) of the batch
//   k_radiance_query  as it stands, on those rays with spp = 1 and seed = 0
//   k_dir_project     one wave per point: the samples onto the four real spherical harmonics of bands 0 .. 1, summed in the
//                     probe rule's fixed tree
// For sample s of point i, f = seed * spp + s (u32):
//  * the direction is the probe rule's for (pad, f), probe_direction, mirrored into the hemisphere of the point's normal N as
//    given: c = (d0.x * N.x + d0.y * N.y) + d0.z * N.z, d = c < 0 ? -d0 : d0 (a NaN does not flip); not normalised again;
//  * the sample is what k_radiance_query returns for the ray {position, t_max, d, pad} with spp = 1 and seed = f, which
//    THE PAD IDENTITY of k_probe.hip.h turns into seed = 0 on pad' = pad + f * 719393u.
#define RT_DIR_SH_COEFFS 4

__device__ __forceinline__ rt3 dir_direction(uint32_t pad, uint32_t f, float nx, float ny, float nz) {
  const rt3 d0 = probe_direction(pad, f);
  const float c = (d0.x * nx + d0.y * ny) + d0.z * nz;
  return (c < 0.0f) ? rt3_make(-d0.x, -d0.y, -d0.z) : d0;
}

// One thread per (point, sample) of the batch: item g = i * spp + s.  points: 2 float4 per point; rays: 2 float4 per item.
// n_items = points of the batch * spp <= RT_DIRECTIONAL_BATCH_SAMPLES (the host cuts the call), so g stays far below 2^32.
__global__ __launch_bounds__(256)
void k_dir_rays(const float4* __restrict__ points, float4* __restrict__ rays, uint32_t n_items, uint32_t spp, uint32_t seed) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n_items) return;
  const uint32_t i = g / spp, s = g - i * spp;
  const uint32_t f = seed * spp + s;
  const float4 r0 = points[2 * (size_t)i];
  const float4 r1 = points[2 * (size_t)i + 1];
  const uint32_t pad = rt_f2u(r1.w);
  const rt3 d = dir_direction(pad, f, r1.x, r1.y, r1.z);
  rays[2 * (size_t)g] = r0;
  rays[2 * (size_t)g + 1] = make_float4(d.x, d.y, d.z, rt_u2f(pad + f * 719393u));
}

// One wave per point (four per workgroup).  Lane l strides over the samples l, l + 64, ...: it makes the direction again
// from the rng and the point's normal (so only the 16-byte radiance is read), and adds radiance[c] * Y_k(d) to its 12
// partial sums, each ((+0 + term(l)) + term(l + 64)) + ...  Then six butterfly steps m = 32 .. 1, P[l] = P[l] + P[l ^ m] in
// all lanes at once, and lane 0 holds the sum the rule names; it divides, scales by 2 pi and stores the 64 bytes as four
// vector stores, row k {sh[k].rgb, hit_fraction} being the texel of atlas layer k.  A sample is a hit iff t < t_max (false
// for NaN).
__global__ __launch_bounds__(256)
void k_dir_project(const float4* __restrict__ points, const float4* __restrict__ radiance, float4* __restrict__ out,
                   uint32_t n_points, uint32_t spp, uint32_t seed) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);   // wave-uniform
  if (i >= n_points) return;
  const float t_max = points[2 * (size_t)i].w;
  const float4 r1 = points[2 * (size_t)i + 1];
  const uint32_t pad = rt_f2u(r1.w);
  const float4* rad = radiance + (size_t)i * spp;
  float acc[RT_DIR_SH_COEFFS][3];
#pragma unroll
  for (int k = 0; k < RT_DIR_SH_COEFFS; k++) acc[k][0] = acc[k][1] = acc[k][2] = 0.0f;
  uint32_t hits = 0u;
  for (uint32_t s = lane; s < spp; s += 64u) {
    const rt3 d = dir_direction(pad, seed * spp + s, r1.x, r1.y, r1.z);
    const float4 L = rad[s];
    if (L.w < t_max) hits++;
    float Y[RT_DIR_SH_COEFFS];
    Y[0] = 0.282094792f;
    Y[1] = 0.488602512f * d.y;
    Y[2] = 0.488602512f * d.z;
    Y[3] = 0.488602512f * d.x;
#pragma unroll
    for (int k = 0; k < RT_DIR_SH_COEFFS; k++) {
      acc[k][0] = acc[k][0] + L.x * Y[k];
      acc[k][1] = acc[k][1] + L.y * Y[k];
      acc[k][2] = acc[k][2] + L.z * Y[k];
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int k = 0; k < RT_DIR_SH_COEFFS; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) acc[k][c] = acc[k][c] + __shfl_xor(acc[k][c], m, 64);
    hits += __shfl_xor(hits, m, 64);
  }
  if (lane == 0u) {
    const float n = (float)spp;
    const float hf = rt_div((float)hits, n);
    float4* o = out + 4 * (size_t)i;
#pragma unroll
    for (int k = 0; k < RT_DIR_SH_COEFFS; k++)
      o[k] = make_float4(rt_div(acc[k][0], n) * RT_TWO_PI, rt_div(acc[k][1], n) * RT_TWO_PI, rt_div(acc[k][2], n) * RT_TWO_PI, hf);
  }
}

// The way back into a layer-major atlas of four layers: layer k of texel texels[j] = row k of results[j], every uncovered
// texel of every layer {+0, +0, +0, -1}.  The owner map is an atlas bake's (u64, all ones = uncovered).  As in bake_scatter
// the two groups of stores of a thread go to different kinds of texel, and every texel is written by exactly one thread.
struct DirScatterArgs {
  const unsigned long long* owner;   // n_texels
  const uint32_t* texels;            // n, each below n_texels and covered
  const float4* results;             // n rt_directional: 4 float4 each
  float4* layers;                    // 4 * n_texels
  uint32_t n_texels, n;
};
__global__ __launch_bounds__(256) void k_dir_scatter(DirScatterArgs A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < A.n_texels && A.owner[i] == ~0ull) {
#pragma unroll
    for (int k = 0; k < RT_DIR_SH_COEFFS; k++) A.layers[(size_t)k * A.n_texels + i] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
  }
  if (i < A.n) {
    const uint32_t t = A.texels[i];
#pragma unroll
    for (int k = 0; k < RT_DIR_SH_COEFFS; k++) A.layers[(size_t)k * A.n_texels + t] = A.results[4 * (size_t)i + k];
  }
}

}  // namespace rtk
#endif
