// k_block_scan.hip.h — the block-level count, rank and prefix sum of the kernels that lay a scene out on the device (BLAS
// builder, node and pair re-layout, world update, lightmap point pass, atlas dilation), and the one-workgroup scan kernel
// between their count and rank launches.  Needs nothing of the project: tests/model/scan_check.hip includes it alone.
//
// At every call site ALL T threads of the workgroup call the primitive (threads out of range pass false / 0) and none
// returns before it.  Scratch is the caller's, so that two calls share LDS only where the caller says so.  The rank and the
// scans start with a barrier: the scratch may still be read by the previous call, so calls in a loop, or two in a row on
// the same scratch, are safe.
#ifndef MI355RT_K_BLOCK_SCAN_HIP_H
#define MI355RT_K_BLOCK_SCAN_HIP_H

namespace rtk {

// exclusive prefix sum of a flag over the T threads of the block; returns this thread's rank and the block total
// (s_wave: T / 64 words)
template <int T>
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t* s_wave, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const uint32_t in_wave = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  __syncthreads();  // s_wave may still be read by the previous call
  if (lane == 0u) s_wave[wave] = (uint32_t)__builtin_popcountll(m);
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t w = 0; w < (uint32_t)(T / 64); w++) {
    const uint32_t v = s_wave[w];
    before += w < wave ? v : 0u;
    all += v;
  }
  total = all;
  return before + in_wave;
}

// The number of set flags among the T threads of the block, in every thread (s_wave: T / 64 words).  The exception to the
// leading barrier: every caller counts once per kernel, and a barrier in front would be all a count kernel pays beyond its
// one.  A caller that has used s_wave before puts a barrier of its own in front.
template <int T>
__device__ __forceinline__ uint32_t block_count(bool flag, uint32_t* s_wave) {
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = (uint32_t)__builtin_popcountll(m);
  __syncthreads();
  uint32_t all = 0;
  for (uint32_t w = 0; w < (uint32_t)(T / 64); w++) all += s_wave[w];
  return all;
}

// Hillis-Steele inclusive prefix sum of v over the T threads of the block; s[T - 1] is the block total afterwards
// (s: T values)
template <int T, class V>
__device__ __forceinline__ V block_scan_inclusive(V v, V* s) {
  const uint32_t tid = threadIdx.x;
  __syncthreads();  // s may still be read by the previous call
  s[tid] = v;
  __syncthreads();
  for (uint32_t off = 1u; off < (uint32_t)T; off <<= 1) {
    const V w = tid >= off ? s[tid - off] : (V)0;
    __syncthreads();
    s[tid] += w;
    __syncthreads();
  }
  return s[tid];
}

// One workgroup of T threads: a[0 .. n) becomes its exclusive prefix sums in place, *total their sum (total may be null,
// and may be a + n); s[T - 1] holds the sum afterwards as well.  Every thread sums a contiguous run of ceil(n / T) elements,
// one pass over the T run sums follows, then the write-back: for n <= T that is one element per thread.  (s: T values)
template <int T, class V>
__device__ __forceinline__ void array_scan_exclusive(V* a, uint32_t n, V* total, V* s) {
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (n + (uint32_t)T - 1u) / (uint32_t)T;
  const uint32_t b0 = tid * per < n ? tid * per : n, b1 = b0 + per < n ? b0 + per : n;
  V sum = 0;
  for (uint32_t b = b0; b < b1; b++) sum += a[b];
  V run = block_scan_inclusive<T>(sum, s) - sum;   // the sum of the elements before b0
  for (uint32_t b = b0; b < b1; b++) {
    const V v = a[b];
    a[b] = run;
    run += v;
  }
  if (total && tid == (uint32_t)T - 1u) *total = s[tid];
}

// a[0 .. n) of u32 counts -> their exclusive prefix in place, the grand total to *total when it is given
__global__ __launch_bounds__(1024) void k_scan_counts(uint32_t* a, uint32_t n, uint32_t* total) {
  __shared__ uint32_t s[1024];
  array_scan_exclusive<1024>(a, n, total, s);
}

}  // namespace rtk
#endif
