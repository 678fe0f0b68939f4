// math_check.hip — the DEVICE compilation of include/mi355rt_math.h over the input sets of math_inputs.h, as checksums.
// A small library of its own, built by tests/math_util.py with the product's compiler flags; tests/test_gpu_math.py
// compares its checksums with those of the host compilation (tests/model/math_ref.cpp).  Test infrastructure outside the
// product library: nothing of the renderer is linked or touched.
//
// The headers come in the order of csrc/device_scene.h: k_ieee.hip.h first, so that a device compilation routes
// rt_div / rt_rcp / rt_sqrt / ... of the math header to the short sequences exactly as the kernels' does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "k_ieee.hip.h"
#include "mi355rt_math.h"
// the kernels' RNG: k_common.hip.h is part of the kernel set and needs the scene types before it
#include "device_scene.h"
#include "k_common.hip.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define MATH_INIT_RNG(pixel, frame) rtk::init_rng(pixel, frame)
#define MATH_RAND_PCG(state) rtk::rand_pcg(state)
#endif
#include "math_ops.h"

struct math_report {
  unsigned long long n, in_domain, checksum;
  unsigned int value[MATH_MAX_RESULTS];   // the result words of index `first`
};

__device__ __forceinline__ unsigned long long math_wave_sum(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

template <int OP>
__global__ __launch_bounds__(256) void k_math_check(unsigned long long first, unsigned long long count, math_report* rep) {
  unsigned long long n_in = 0, sum = 0;
  const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
  // every lane runs the same number of trips (the functions hold wave-uniform branches); lanes past the end idle
  const unsigned long long trips = (count + stride - 1ull) / stride;
  const unsigned long long R = (unsigned long long)math_results(OP);
  for (unsigned long long t = 0; t < trips; t++) {
    const unsigned long long k = t * stride + (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (k >= count) continue;
    const unsigned long long i = first + k;
    uint32_t w[MATH_MAX_RESULTS] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    const int nres = math_eval<OP>(i, w, nullptr, nullptr);
    if (nres > 0) {
      n_in += 1ull;
#pragma unroll
      for (int c = 0; c < MATH_MAX_RESULTS; c++)
        if (c < nres) sum += math_mix(OP, w[c], R * i + (unsigned long long)c);
    }
    if (k == 0ull) {
#pragma unroll
      for (int c = 0; c < MATH_MAX_RESULTS; c++) rep->value[c] = w[c];
    }
  }
  n_in = math_wave_sum(n_in);
  sum = math_wave_sum(sum);
  if ((threadIdx.x & 63u) == 0u) {
    atomicAdd(&rep->in_domain, n_in);
    atomicAdd(&rep->checksum, sum);
  }
}

typedef void (*math_kernel)(unsigned long long, unsigned long long, math_report*);
static math_kernel math_kernel_of(int op) {
  switch (op) {
#define MATH_X(name, r) case MATH_OP_##name: return k_math_check<MATH_OP_##name>;
    MATH_OPS(MATH_X)
#undef MATH_X
  }
  return nullptr;
}

// The checksum of op over indices [first, first + count) on device 0.  Returns 0, or the HIP error code (-1: unknown op).
extern "C" int math_check(int op, uint64_t first, uint64_t count, math_report* out) {
  if (!out) return -1;
  std::memset(out, 0, sizeof(*out));
  const math_kernel kern = math_kernel_of(op);
  if (!kern) return -1;
  if (count == 0) return 0;
  hipError_t e = hipSetDevice(0);
  if (e != hipSuccess) return (int)e;
  int cus = 0;
  e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  if (e != hipSuccess) return (int)e;
  if (cus < 1) cus = 1;
  hipStream_t stream = nullptr;
  e = hipStreamCreate(&stream);
  if (e != hipSuccess) return (int)e;
  math_report* d = nullptr;
  e = hipMalloc((void**)&d, sizeof(math_report));
  if (e == hipSuccess) {
    e = hipMemsetAsync(d, 0, sizeof(math_report), stream);
    const uint64_t want = (count + 255) / 256, cap = (uint64_t)cus * 32u;
    const dim3 grid((uint32_t)(want < cap ? want : cap)), block(256);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(kern, grid, block, 0, stream, (unsigned long long)first, (unsigned long long)count, d);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, sizeof(*out), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d);
  }
  (void)hipStreamDestroy(stream);
  if (e != hipSuccess) return (int)e;
  out->n = count;
  return 0;
}
