// k_probe.hip.h — k_probe_rays and k_probe_project: the two kernels a probe gather (rt_gather_probes, mi355rt.h) puts around
// k_radiance_query.
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_PROBE_HIP_H
#define MI355RT_K_PROBE_HIP_H

namespace rtk {

// A probe gather is a composition, not a third policy of path_query_loop: a lane of that loop keeps its item for all spp
// samples, and a probe grid is few items with very many samples (4 096 probes fill 64 waves); 27 accumulators across
// shade_bounce do not fit beside a PathState either.  So the unit of path work is the (probe, sample) pair:
//   k_probe_rays      one rt_ray per (probe, sample) of the batch
//   k_radiance_query  as it stands, on those rays with spp = 1 and seed = 0
//   k_probe_project   one wave per probe: the samples onto the nine real spherical harmonics of bands 0 .. 2, summed in a
//                     fixed tree
// For sample s of probe i, f = seed * spp + s (u32):
//  * the direction is uniform on the sphere from a stream of its own, rng_d = init_rng(pad ^ RT_GATHER_DIR_STREAM, f) (the
//    gather's stream id): z = 1 - 2 u1, r = sqrt(max(0, 1 - z z)), (sin, cos) of 2 pi u2, d = (r cos, r sin, z); it is not
//    normalised again;
//  * the sample is what k_radiance_query returns for the ray {position, t_max, d, pad} with spp = 1 and seed = f.
// THE PAD IDENTITY.  init_rng(a, b) hashes a + b * 719393u (k_common.hip.h), so init_rng(pad + f * 719393u, 0) ==
// init_rng(pad, f): k_probe_rays writes pad' = pad + f * 719393u (u32) into the ray, and the radiance query at seed = 0, spp
// = 1 on pad' runs every path with exactly init_rng(pad, f).  One launch thereby carries a different f per item and
// path_query_loop is untouched.
#define RT_PROBE_SH_COEFFS 9
#define RT_PROBE_FOUR_PI 12.566370614f

__device__ __forceinline__ rt3 probe_direction(uint32_t pad, uint32_t f) {
  uint32_t rng_d = init_rng(pad ^ RT_GATHER_DIR_STREAM, f);
  const float u1 = rand_pcg(rng_d);
  const float u2 = rand_pcg(rng_d);
  const float z = 1.0f - 2.0f * u1;
  const float r = rt_sqrt(rt_max(0.0f, 1.0f - z * z));
  float sp, cp;
  rt_sincos(RT_TWO_PI * u2, &sp, &cp);
  return rt3_make(r * cp, r * sp, z);
}

// One thread per (probe, sample) of the batch: item g = i * spp + s.  probes: 2 float4 per probe; rays: 2 float4 per item.
// n_items = probes of the batch * spp <= RT_PROBE_BATCH_SAMPLES (the host cuts the call), so g stays far below 2^32.
__global__ __launch_bounds__(256)
void k_probe_rays(const float4* __restrict__ probes, float4* __restrict__ rays, uint32_t n_items, uint32_t spp, uint32_t seed) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n_items) return;
  const uint32_t i = g / spp, s = g - i * spp;
  const uint32_t f = seed * spp + s;
  const float4 r0 = probes[2 * (size_t)i];
  const uint32_t pad = rt_f2u(probes[2 * (size_t)i + 1].w);
  const rt3 d = probe_direction(pad, f);
  rays[2 * (size_t)g] = r0;
  rays[2 * (size_t)g + 1] = make_float4(d.x, d.y, d.z, rt_u2f(pad + f * 719393u));
}

// One wave per probe (four per workgroup).  Lane l strides over the samples l, l + 64, ...: it makes the direction again
// from the rng (so only the 16-byte radiance is read), and adds radiance[c] * Y_k(d) to its 27 partial sums, each ((+0 +
// term(l)) + term(l + 64)) + ...  Then six butterfly steps m = 32 .. 1, P[l] = P[l] + P[l ^ m] in all lanes at once, and
// lane 0 holds the sum the rule names; it divides, scales by 4 pi and stores the 112 bytes as seven vector stores.  A sample
// is a hit iff t < t_max (false for NaN).
__global__ __launch_bounds__(256)
void k_probe_project(const float4* __restrict__ probes, const float4* __restrict__ radiance, float4* __restrict__ out,
                     uint32_t n_probes, uint32_t spp, uint32_t seed) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);   // wave-uniform
  if (i >= n_probes) return;
  const float t_max = probes[2 * (size_t)i].w;
  const uint32_t pad = rt_f2u(probes[2 * (size_t)i + 1].w);
  const float4* rad = radiance + (size_t)i * spp;
  float acc[RT_PROBE_SH_COEFFS][3];
#pragma unroll
  for (int k = 0; k < RT_PROBE_SH_COEFFS; k++) acc[k][0] = acc[k][1] = acc[k][2] = 0.0f;
  uint32_t hits = 0u;
  for (uint32_t s = lane; s < spp; s += 64u) {
    const rt3 d = probe_direction(pad, seed * spp + s);
    const float4 L = rad[s];
    if (L.w < t_max) hits++;
    float Y[RT_PROBE_SH_COEFFS];
    Y[0] = 0.282094792f;
    Y[1] = 0.488602512f * d.y;
    Y[2] = 0.488602512f * d.z;
    Y[3] = 0.488602512f * d.x;
    Y[4] = 1.092548431f * (d.x * d.y);
    Y[5] = 1.092548431f * (d.y * d.z);
    Y[6] = 0.315391565f * (3.0f * (d.z * d.z) - 1.0f);
    Y[7] = 1.092548431f * (d.x * d.z);
    Y[8] = 0.546274215f * (d.x * d.x - d.y * d.y);
#pragma unroll
    for (int k = 0; k < RT_PROBE_SH_COEFFS; k++) {
      acc[k][0] = acc[k][0] + L.x * Y[k];
      acc[k][1] = acc[k][1] + L.y * Y[k];
      acc[k][2] = acc[k][2] + L.z * Y[k];
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int k = 0; k < RT_PROBE_SH_COEFFS; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) acc[k][c] = acc[k][c] + __shfl_xor(acc[k][c], m, 64);
    hits += __shfl_xor(hits, m, 64);
  }
  if (lane == 0u) {
    const float n = (float)spp;
    float w[28];
#pragma unroll
    for (int k = 0; k < RT_PROBE_SH_COEFFS; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) w[3 * k + c] = rt_div(acc[k][c], n) * RT_PROBE_FOUR_PI;
    w[27] = rt_div((float)hits, n);
    float4* o = out + 7 * (size_t)i;
#pragma unroll
    for (int j = 0; j < 7; j++) o[j] = make_float4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
  }
}

}  // namespace rtk
#endif
