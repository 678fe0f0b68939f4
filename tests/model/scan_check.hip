// scan_check.hip — the block primitives of csrc/k_block_scan.hip.h by themselves, each behind a trivial kernel.
// A small library of its own, built by tests/test_gpu_scan.py with the product's compiler flags; the test compares what
// comes back with numpy, exactly.  Test infrastructure outside the product library: nothing else of the renderer is
// included, linked or touched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_block_scan.hip.h"

enum { SCAN_RANK = 0, SCAN_INCLUSIVE = 1, SCAN_ARRAY_U32 = 2, SCAN_ARRAY_U64 = 3 };
enum { TOTAL_SEPARATE = 0, TOTAL_BEHIND = 1, TOTAL_NULL = 2 };

// flag then !flag on the same s_wave, as bvhb::k_big_plan ranks its large and its small nodes; threads past n pass false
// out: rank of flag [n], rank of !flag [n], then per block {total of flag, total of !flag, count of flag, count of !flag}
template <int T>
__global__ __launch_bounds__(T) void k_rank_check(const uint32_t* flag, uint32_t n, uint32_t* out) {
  __shared__ uint32_t s_wave[T / 64];
  const uint32_t i = blockIdx.x * (uint32_t)T + threadIdx.x;
  const bool in = i < n, f = in && flag[i] != 0u;
  uint32_t total_f, total_nf;
  const uint32_t rank_f = rtk::block_rank<T>(f, s_wave, total_f);
  const uint32_t rank_nf = rtk::block_rank<T>(in && !f, s_wave, total_nf);
  __syncthreads();   // block_count has no leading barrier of its own: s_wave was just read by block_rank
  const uint32_t count_f = rtk::block_count<T>(f, s_wave);
  __syncthreads();
  const uint32_t count_nf = rtk::block_count<T>(in && !f, s_wave);
  if (in) {
    out[i] = rank_f;
    out[n + i] = rank_nf;
  }
  if (threadIdx.x == (uint32_t)T - 1u) {
    uint32_t* b = out + 2 * (size_t)n + 4 * (size_t)blockIdx.x;
    b[0] = total_f;
    b[1] = total_nf;
    b[2] = count_f;
    b[3] = count_nf;
  }
}

// one block, twice in a row on the same scratch.  in: 2 T values; out: 2 T inclusive sums, then s[T - 1] after either call
template <int T>
__global__ __launch_bounds__(T) void k_inclusive_check(const uint32_t* in, uint32_t* out) {
  __shared__ uint32_t s[T];
  const uint32_t t = threadIdx.x;
  const uint32_t r0 = rtk::block_scan_inclusive<T>(in[t], s);
  const uint32_t t0 = s[T - 1];
  const uint32_t r1 = rtk::block_scan_inclusive<T>(in[T + t], s);
  const uint32_t t1 = s[T - 1];
  out[t] = r0;
  out[T + t] = r1;
  if (t == 0u) {
    out[2 * T] = t0;
    out[2 * T + 1] = t1;
  }
}

__global__ __launch_bounds__(1024) void k_array_u64_check(unsigned long long* a, uint32_t n, unsigned long long* total) {
  __shared__ unsigned long long s[1024];
  rtk::array_scan_exclusive<1024>(a, n, total, s);
}

template <class V>
static hipError_t array_check(uint32_t n, int total_mode, const void* in, void* out) {
  // device buffer: a[0 .. n), the word behind the array, a separate word; the caller fills all n + 2
  V* d = nullptr;
  const size_t bytes = ((size_t)n + 2) * sizeof(V);
  hipError_t e = hipMalloc((void**)&d, bytes);
  if (e != hipSuccess) return e;
  e = hipMemcpy(d, in, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    V* total = total_mode == TOTAL_SEPARATE ? d + n + 1 : (total_mode == TOTAL_BEHIND ? d + n : nullptr);
    if (sizeof(V) == 4) hipLaunchKernelGGL(rtk::k_scan_counts, dim3(1), dim3(1024), 0, 0, (uint32_t*)d, n, (uint32_t*)total);
    else hipLaunchKernelGGL(k_array_u64_check, dim3(1), dim3(1024), 0, 0, (unsigned long long*)d, n, (unsigned long long*)total);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost);   // on the null stream: after the kernel
  (void)hipFree(d);
  return e;
}

// One entry for the four checks, on device 0; returns 0, the first HIP error code, or -1 for arguments it does not know.
//   SCAN_RANK       threads 256 | 1024; in: n u32 flags; out: 2 n + 4 ceil(n / threads) u32 (k_rank_check)
//   SCAN_INCLUSIVE  threads 256 | 1024; in: 2 threads u32; out: 2 threads + 2 u32 (k_inclusive_check)
//   SCAN_ARRAY_*    in and out: n + 2 elements (the array, the word behind it, a separate word); total_mode says which of
//                   the two receives the sum, or neither
extern "C" int scan_check(int op, int threads, int total_mode, uint32_t n, const void* in, void* out) {
  if (!in || !out) return -1;
  hipError_t e = hipSetDevice(0);
  if (e != hipSuccess) return (int)e;
  if (op == SCAN_ARRAY_U32 || op == SCAN_ARRAY_U64) {
    if (total_mode < TOTAL_SEPARATE || total_mode > TOTAL_NULL) return -1;
    return (int)(op == SCAN_ARRAY_U32 ? array_check<uint32_t>(n, total_mode, in, out)
                                      : array_check<unsigned long long>(n, total_mode, in, out));
  }
  if ((op != SCAN_RANK && op != SCAN_INCLUSIVE) || (threads != 256 && threads != 1024)) return -1;
  const uint32_t T = (uint32_t)threads;
  const uint32_t blocks = op == SCAN_RANK ? (n + T - 1u) / T : 1u;
  if (op == SCAN_RANK && n == 0u) return -1;
  const size_t n_in = op == SCAN_RANK ? (size_t)n : 2 * (size_t)T;
  const size_t n_out = op == SCAN_RANK ? 2 * (size_t)n + 4 * (size_t)blocks : 2 * (size_t)T + 2;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  e = hipMalloc((void**)&d_in, n_in * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, n_out * 4);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, n_in * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0xff, n_out * 4);
  if (e == hipSuccess) {
    if (op == SCAN_RANK && T == 256u) hipLaunchKernelGGL(k_rank_check<256>, dim3(blocks), dim3(256), 0, 0, d_in, n, d_out);
    else if (op == SCAN_RANK) hipLaunchKernelGGL(k_rank_check<1024>, dim3(blocks), dim3(1024), 0, 0, d_in, n, d_out);
    else if (T == 256u) hipLaunchKernelGGL(k_inclusive_check<256>, dim3(1), dim3(256), 0, 0, d_in, d_out);
    else hipLaunchKernelGGL(k_inclusive_check<1024>, dim3(1), dim3(1024), 0, 0, d_in, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d_out, n_out * 4, hipMemcpyDeviceToHost);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return (int)e;
}
