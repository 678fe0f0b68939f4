// k_reflection_sample.hip.h — the kernel of the reflection sampler (rt_sample_reflection, mi355rt.h "THE REFLECTION SAMPLE
// RULE"): k_reflection_sample<PARALLAX> reads baked chains (k_reflection.hip.h) at a caller's queries {position, probe}
// {direction, roughness}: the direction, bent to where it leaves the probe's box in the PARALLAX form, is packed once; each of
// the two levels around the roughness gives four taps, folded across the octahedral seam; the two bilinear values are mixed
// by the fraction of the level.
// Not part of the kernel set of csrc/kernels.hip.h: the sampler needs no scene and none of the other kernels, and is compiled
// in a translation unit of its own (reflection_sample.hip, which includes mi355rt_math.h ahead of this header).
#ifndef MI355RT_K_REFLECTION_SAMPLE_HIP_H
#define MI355RT_K_REFLECTION_SAMPLE_HIP_H

#include "reflection_sample.h"

namespace rtk {

// pack of THE REFLECTION RULE (pack_normal of k_shading.hip.h, restated: that header belongs to the scene's kernels)
__device__ __forceinline__ rt2 reflection_sample_pack(rt3 v) {
  const float s = rt_rcp(rt_abs(v.x) + rt_abs(v.y) + rt_abs(v.z));
  const rt2 p = rt2_make(v.x * s, v.y * s);
  if (v.z < 0.0f)
    return rt2_make((1.0f - rt_abs(p.y)) * (p.x >= 0.0f ? 1.0f : -1.0f), (1.0f - rt_abs(p.x)) * (p.y >= 0.0f ? 1.0f : -1.0f));
  return p;
}

// one axis of the fetch: the left tap in -1 .. S - 1 and the weight of its neighbour, in [0, 1) whatever q is
__device__ __forceinline__ int reflection_sample_axis(float q, float fS, float* f) {
  float u = (q * 0.5f + 0.5f) * fS - 0.5f;
  if (!(u >= -0.5f)) u = -0.5f;   // NaN too
  u = rt_min(u, fS - 0.5f);
  const float fl = rt_floor(u);
  *f = u - fl;
  return (int)fl;
}

// The fold of a tap (i, j) in -1 .. S across the octahedral seam, x first, then y; -> texel index j * S + i.  It is
// visibility_wrap (k_volume_visibility.hip.h) without a branch: a coordinate in -1 .. S that is outside folds to the nearest
// one inside, -1 to 0 and S to S - 1, which is a clamp, and the other coordinate is mirrored.
__device__ __forceinline__ uint32_t reflection_sample_fold(int i, int j, int S) {
  const int ci = min(max(i, 0), S - 1);
  j = (ci != i) ? S - 1 - j : j;
  const int cj = min(max(j, 0), S - 1);
  const int fi = (cj != j) ? S - 1 - ci : ci;
  return (uint32_t)(cj * S + fi);
}

// the four folded taps of a level of side 1 << S_log2 around q and their weights w00, w10, w01, w11
struct ReflectionTaps {
  uint32_t t[4];
  float w[4];
};
__device__ __forceinline__ ReflectionTaps reflection_sample_taps(rt2 q, uint32_t S_log2) {
  const int S = 1 << S_log2;
  const float fS = (float)S;
  float fx, fy;
  const int i0 = reflection_sample_axis(q.x, fS, &fx), j0 = reflection_sample_axis(q.y, fS, &fy);
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  ReflectionTaps T;
  T.t[0] = reflection_sample_fold(i0, j0, S);
  T.t[1] = reflection_sample_fold(i0 + 1, j0, S);
  T.t[2] = reflection_sample_fold(i0, j0 + 1, S);
  T.t[3] = reflection_sample_fold(i0 + 1, j0 + 1, S);
  T.w[0] = gx * gy;
  T.w[1] = fx * gy;
  T.w[2] = gx * fy;
  T.w[3] = fx * fy;
  return T;
}

// A term of weight exactly zero is left out: +0 in its place leaves the sum as it is, because a sum that began at +0 never
// is -0 - and the texel, whatever it holds, is dropped.
__device__ __forceinline__ float reflection_sample_term(float w, float v) { return (w == 0.0f) ? 0.0f : w * v; }
__device__ __forceinline__ float4 reflection_sample_value(const float (&w)[4], const float4 (&v)[4]) {
  float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    a.x = a.x + reflection_sample_term(w[k], v[k].x);
    a.y = a.y + reflection_sample_term(w[k], v[k].y);
    a.z = a.z + reflection_sample_term(w[k], v[k].z);
    a.w = a.w + reflection_sample_term(w[k], v[k].w);
  }
  return a;
}

// One thread per query, 256-thread workgroups.  The two 16-byte loads of the query come first; the PARALLAX form then loads
// the probe's position and the two halves of its box - the plain form holds none of that code.  The eight texel loads, four
// per level, are all issued before the first is used: a tap or a level of weight zero is still loaded, from the legal index
// the fold gives it, and dropped.  One 16-byte store.  No LDS, no atomics.  A query whose probe index is outside the array
// loads nothing more and stores four +0.
template <bool PARALLAX>
__global__ __launch_bounds__(256)
void k_reflection_sample(ReflectionSampleArgs A) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= A.n) return;
  float4 q0 = A.queries[2 * (size_t)g];
  float4 q1 = A.queries[2 * (size_t)g + 1];
  // both loads are issued here, whole and aligned: not cut down to the words a form reads, the second not sunk behind the branch
  asm volatile("" : "+v"(q0.x), "+v"(q0.y), "+v"(q0.z), "+v"(q0.w), "+v"(q1.x), "+v"(q1.y), "+v"(q1.z), "+v"(q1.w));
  const uint32_t p = rt_f2u(q0.w);
  if (p >= A.n_probes) {
    A.out[g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  rt3 d = rt3_make(q1.x, q1.y, q1.z);
  if (PARALLAX) {
    const float4 c = A.probes[2 * (size_t)p];
    const float4 lo = A.boxes[2 * (size_t)p];
    const float4 hi = A.boxes[2 * (size_t)p + 1];
    const bool inside = lo.x <= q0.x && q0.x <= hi.x && lo.y <= q0.y && q0.y <= hi.y && lo.z <= q0.z && q0.z <= hi.z;
    if (inside) {
      // the quotient of an axis that does not move is worked out on a numerator of no meaning and dropped
      const float tx = (d.x > 0.0f || d.x < 0.0f) ? rt_div((d.x > 0.0f ? hi.x : lo.x) - q0.x, d.x) : __builtin_inff();
      const float ty = (d.y > 0.0f || d.y < 0.0f) ? rt_div((d.y > 0.0f ? hi.y : lo.y) - q0.y, d.y) : __builtin_inff();
      const float tz = (d.z > 0.0f || d.z < 0.0f) ? rt_div((d.z > 0.0f ? hi.z : lo.z) - q0.z, d.z) : __builtin_inff();
      const float t = rt_min(rt_min(tx, ty), tz);
      if (t < __builtin_inff()) {
        const rt3 h = rt3_make(q0.x + d.x * t, q0.y + d.y * t, q0.z + d.z * t);
        d = rt3_make(h.x - c.x, h.y - c.y, h.z - c.z);
      }
    }
  }
  // the level
  float r = q1.w;
  if (!(r > 0.0f)) r = 0.0f;   // NaN too
  r = rt_min(r, 1.0f);
  const float xl = r * (float)(A.levels - 1u);
  const uint32_t m0 = min((uint32_t)xl, A.levels - 2u);
  const float gm = xl - (float)m0;
  const float wa = 1.0f - gm, wb = gm;
  // level m of side S_m = size >> m lies at the texel (4 / 3) (size^2 - S_m^2) of its chain, level m + 1 right behind it
  const uint32_t S0_log2 = A.size_log2 - m0;
  const uint32_t map = 1u << (2u * A.size_log2), side2 = 1u << (2u * S0_log2);
  const float4* __restrict__ level0 = A.chains + (size_t)p * A.chain + (4u * (map - side2)) / 3u;
  const float4* __restrict__ level1 = level0 + side2;
  const rt2 q = reflection_sample_pack(d);
  const ReflectionTaps Ta = reflection_sample_taps(q, S0_log2), Tb = reflection_sample_taps(q, S0_log2 - 1u);
  float4 va[4], vb[4];
#pragma unroll
  for (int k = 0; k < 4; k++) va[k] = level0[Ta.t[k]];
#pragma unroll
  for (int k = 0; k < 4; k++) vb[k] = level1[Tb.t[k]];
  const float4 a = reflection_sample_value(Ta.w, va), b = reflection_sample_value(Tb.w, vb);
  A.out[g] = make_float4((0.0f + reflection_sample_term(wa, a.x)) + reflection_sample_term(wb, b.x),
                         (0.0f + reflection_sample_term(wa, a.y)) + reflection_sample_term(wb, b.y),
                         (0.0f + reflection_sample_term(wa, a.z)) + reflection_sample_term(wb, b.z),
                         (0.0f + reflection_sample_term(wa, a.w)) + reflection_sample_term(wb, b.w));
}

}  // namespace rtk
#endif
