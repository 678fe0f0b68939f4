// k_reflection.hip.h — the kernels of reflection probes (rt_capture_reflection / rt_filter_reflection / rt_bake_reflection,
// mi355rt.h "THE REFLECTION RULE"): k_reflection_rays and k_reflection_texels go around k_radiance_query as k_probe_rays and
// k_probe_project do, with the (texel, sample) pair as the unit of path work; k_reflection_filter makes one level of the
// GGX-filtered chain from level 0; k_reflection_copy puts packed maps into level 0 of their chains.
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_REFLECTION_HIP_H
#define MI355RT_K_REFLECTION_HIP_H

namespace rtk {

// A map is size * size texels, size = 1 << size_log2; the texels of the n probes of a call are numbered T = p * size^2 + t,
// below 2^31 (the host refuses more).  A batch is the texels [first, first + n_texels) of that numbering, whatever probes
// they belong to: item g = tl * spt + s of a batch is sample s of texel first + tl.
__device__ __forceinline__ rt3 reflection_direction(uint32_t pad_t, uint32_t f, uint32_t i, uint32_t j, float fsize) {
  uint32_t rng_d = init_rng(pad_t ^ RT_GATHER_DIR_STREAM, f);
  const float jx = rand_pcg(rng_d);
  const float jy = rand_pcg(rng_d);
  const float px = rt_div((float)i + jx, fsize) * 2.0f - 1.0f;
  const float py = rt_div((float)j + jy, fsize) * 2.0f - 1.0f;
  return unpack_normal(px, py);
}

// One thread per (texel, sample) of the batch.  probes: 2 float4 per probe; rays: 2 float4 per item, with the pad identity
// of k_probe.hip.h: pad' = pad_t + f * 719393u, traced at seed = 0, spp = 1.  n_items = n_texels * spt <=
// RT_PROBE_BATCH_SAMPLES.
__global__ __launch_bounds__(256)
void k_reflection_rays(const float4* __restrict__ probes, float4* __restrict__ rays, uint32_t n_items, uint32_t spt, uint32_t seed,
                       uint32_t first, uint32_t size_log2) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n_items) return;
  const uint32_t tl = g / spt, s = g - tl * spt;
  const uint32_t T = first + tl;
  const uint32_t p = T >> (2u * size_log2), t = T & ((1u << (2u * size_log2)) - 1u);
  const uint32_t i = t & ((1u << size_log2) - 1u), j = t >> size_log2;
  const uint32_t f = seed * spt + s;
  const float4 r0 = probes[2 * (size_t)p];
  const uint32_t pad_t = rt_f2u(probes[2 * (size_t)p + 1].w) + t;
  const rt3 d = reflection_direction(pad_t, f, i, j, (float)(1u << size_log2));
  rays[2 * (size_t)g] = r0;
  rays[2 * (size_t)g + 1] = make_float4(d.x, d.y, d.z, rt_u2f(pad_t + f * 719393u));
}

// One thread per texel of the batch: the mean of its spt samples in sample order and the share of them that hit, as one
// 16-byte store to texel t of probe p's map at out + p * out_stride (out_stride = size^2 for packed maps, chain_texels for a
// bake).  A sample is a hit iff t < t_max (false for NaN).
__global__ __launch_bounds__(256)
void k_reflection_texels(const float4* __restrict__ probes, const float4* __restrict__ radiance, float4* __restrict__ out,
                         uint32_t n_texels, uint32_t spt, uint32_t first, uint32_t size_log2, uint32_t out_stride) {
  const uint32_t tl = blockIdx.x * 256u + threadIdx.x;
  if (tl >= n_texels) return;
  const uint32_t T = first + tl;
  const uint32_t p = T >> (2u * size_log2), t = T & ((1u << (2u * size_log2)) - 1u);
  const float t_max = probes[2 * (size_t)p].w;
  const float4* rad = radiance + (size_t)tl * spt;
  rt3 col = rt3_splat(0.0f);
  uint32_t hits = 0u;
  for (uint32_t s = 0u; s < spt; s++) {
    const float4 L = rad[s];
    col = col + rt3_make(L.x, L.y, L.z);
    if (L.w < t_max) hits++;
  }
  if (spt != 1u) col = rt_div3z(col, (float)spt);   // finish_pixel's average
  out[(size_t)p * out_stride + t] = make_float4(col.x, col.y, col.z, rt_div((float)hits, (float)spt));
}

// n packed maps into level 0 of n chains, one thread per texel, word for word.
__global__ __launch_bounds__(256)
void k_reflection_copy(const float4* __restrict__ maps, float4* __restrict__ chains, uint32_t n_texels, uint32_t size_log2,
                       uint32_t chain) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= n_texels) return;
  const uint32_t p = g >> (2u * size_log2), t = g & ((1u << (2u * size_log2)) - 1u);
  chains[(size_t)p * chain + t] = maps[g];
}

// ---- the filter: one level of all n chains per launch.
// One wave per output texel at a time, persistent over the n * S^2 texels of the level.  Lane l owns the samples l, l + 64,
// ... as in k_probe_project.  The half vector, the reflected direction l_t in the tangent frame and the weight w = l_t.z
// depend on (level, sample) only: a lane works them out ONCE, before its first texel, and keeps the three words per sample
// in registers (NS_MAX samples per lane, a template parameter so that the array never leaves the register file; the host
// picks the smallest build that holds filter_samples / 64).  sum_w is the same for every texel of the level and is summed
// once, by the rule's tree.  Per texel and sample only to_world, pack_normal, the two indices and one 16-byte load remain; the
// samples go in groups of RT_REFLECTION_GROUP whose loads are all issued before the first is used.  The four colour sums are
// the rule's tree: the lane's partial in ascending sample order from +0, six butterfly steps; lane 0 divides and stores the
// 16 bytes.  A sample with !(w > 0), or beyond filter_samples in a build that holds more, contributes +0: it reads whatever
// texel its clamped index names and drops what it read.  (A partial never is -0, so adding +0 leaves it as it is.)  No LDS, no atomics.
// Level 0 is not staged in LDS: at size <= 64 it is at most 64 KiB and stays in the vector L1 / L2 of the CUs that gather from
// it, and an LDS copy per workgroup would cap a CU at two workgroups and add a fill per workgroup that the smallest levels
// (16 texels) could never pay back.
#define RT_REFLECTION_GROUP 4
struct ReflectionFilterArgs {
  const float4* src;        // level 0 of probe p at src + p * src_stride
  float4* out;              // the level of probe p at out + p * chain + offset
  uint32_t src_stride, chain, offset;   // in texels
  uint32_t n;               // probes; n * chain < 2^31
  uint32_t size_log2;       // of level 0
  uint32_t level, levels;   // 1 <= level < levels
  uint32_t K;               // filter_samples, a multiple of 64, <= 64 * NS_MAX
};

// (level, sample) -> l_t; w = l_t.z
__device__ __forceinline__ rt3 reflection_lobe(float a, uint32_t s, uint32_t K) {
  const float ux = rt_div((float)s + 0.5f, (float)K);
  const float uy = (float)(__brev(s) >> 8) * 0x1p-24f;
  const float phi = RT_TWO_PI * ux;
  const float cos_theta = rt_sqrt(rt_max(0.0f, rt_div(1.0f - uy, 1.0f + (a * a - 1.0f) * uy)));
  const float sin_theta = rt_sqrt(rt_max(0.0f, 1.0f - cos_theta * cos_theta));
  float sp, cp;
  rt_sincos(phi, &sp, &cp);
  const rt3 h = rt3_make(sin_theta * cp, sin_theta * sp, cos_theta);
  return rt3_make(2.0f * (h.z * h.x), 2.0f * (h.z * h.y), 2.0f * (h.z * h.z) - 1.0f);
}

// texel of level 0 that the world direction l falls into: always inside the map
__device__ __forceinline__ uint32_t reflection_source(rt3 l, uint32_t size, uint32_t size_log2) {
  const rt2 q = pack_normal(l);
  const float fsize = (float)size;
  float ux = (q.x * 0.5f + 0.5f) * fsize;
  float uy = (q.y * 0.5f + 0.5f) * fsize;
  if (!(ux > 0.0f)) ux = 0.0f;   // NaN too
  if (!(uy > 0.0f)) uy = 0.0f;
  const uint32_t ix = min(rt_f2u32_sat(rt_floor(ux)), size - 1u);
  const uint32_t iy = min(rt_f2u32_sat(rt_floor(uy)), size - 1u);
  return (iy << size_log2) + ix;
}

__device__ __forceinline__ float reflection_wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
  return v;
}

template <int NS_MAX>
__global__ __launch_bounds__(256)
void k_reflection_filter(ReflectionFilterArgs A) {
  static_assert(NS_MAX % RT_REFLECTION_GROUP == 0, "whole groups");
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t size = 1u << A.size_log2;
  const uint32_t S_log2 = A.size_log2 - A.level, S = 1u << S_log2;
  const uint32_t ns = A.K >> 6;                                  // samples per lane, wave-uniform
  const float a = rt_div((float)A.level, (float)(A.levels - 1u));
  float lx[NS_MAX], ly[NS_MAX], lz[NS_MAX];
  float pw = 0.0f;
#pragma unroll
  for (int k = 0; k < NS_MAX; k++) {
    lx[k] = ly[k] = lz[k] = 0.0f;
    if ((uint32_t)k < ns) {
      const rt3 lt = reflection_lobe(a, lane + 64u * (uint32_t)k, A.K);
      lx[k] = lt.x;
      ly[k] = lt.y;
      lz[k] = lt.z;
      pw = pw + (lt.z > 0.0f ? lt.z : 0.0f);
    }
  }
  const float sum_w = reflection_wave_sum(pw);
  const bool any = sum_w > 0.0f;
  const float den = any ? sum_w : 1.0f;

  const uint32_t total = A.n << (2u * S_log2);                   // texels of this level in the call, < 2^31
  const uint32_t n_waves = gridDim.x * 4u;
  for (uint32_t e = blockIdx.x * 4u + (threadIdx.x >> 6); e < total; e += n_waves) {   // wave-uniform
    const uint32_t p = e >> (2u * S_log2), t = e & ((1u << (2u * S_log2)) - 1u);
    const uint32_t i = t & (S - 1u), j = t >> S_log2;
    const float cx = rt_div((float)i + 0.5f, (float)S) * 2.0f - 1.0f;
    const float cy = rt_div((float)j + 0.5f, (float)S) * 2.0f - 1.0f;
    const Onb onb = build_onb(unpack_normal(cx, cy));
    const float4* __restrict__ src = A.src + (size_t)p * A.src_stride;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k0 = 0; k0 < NS_MAX; k0 += RT_REFLECTION_GROUP) {
      if ((uint32_t)k0 < ns) {
        float4 v[RT_REFLECTION_GROUP];
#pragma unroll
        for (int q = 0; q < RT_REFLECTION_GROUP; q++) {
          const int k = k0 + q;   // a sample that contributes nothing still reads some texel of the map: the index is clamped
          v[q] = src[reflection_source(to_world(onb, rt3_make(lx[k], ly[k], lz[k])), size, A.size_log2)];
        }
#pragma unroll
        for (int q = 0; q < RT_REFLECTION_GROUP; q++) {
          const int k = k0 + q;
          float w = lz[k];
          asm volatile("" : "+v"(w));   // the comparison stays here: hoisted out of the texel loop, its 64 lane masks would
          const bool valid = w > 0.0f;  // overflow the scalar registers
          acc[0] = acc[0] + (valid ? w * v[q].x : 0.0f);
          acc[1] = acc[1] + (valid ? w * v[q].y : 0.0f);
          acc[2] = acc[2] + (valid ? w * v[q].z : 0.0f);
          acc[3] = acc[3] + (valid ? w * v[q].w : 0.0f);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 4; c++) acc[c] = reflection_wave_sum(acc[c]);
    if (lane == 0u)
      A.out[(size_t)p * A.chain + A.offset + t] =
          any ? make_float4(rt_div(acc[0], den), rt_div(acc[1], den), rt_div(acc[2], den), rt_div(acc[3], den))
              : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
}

}  // namespace rtk
#endif
