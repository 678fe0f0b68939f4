// reflection_sample.h — what the host API (rt_api.hip) and the reflection sampler's translation unit (reflection_sample.hip)
// share: the kernel's argument record and its launcher.  The sampler is a translation unit of its own - it needs nothing of the
// scene, the path tracer or the other kernels, only mi355rt_math.h - linked into the same library.
#ifndef MI355RT_REFLECTION_SAMPLE_H
#define MI355RT_REFLECTION_SAMPLE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtk {

struct ReflectionSampleArgs {
  const float4* chains;     // n_probes chains of `chain` texels, as a bake lays them out
  const float4* probes;     // PARALLAX: n_probes rt_probe, 2 float4 each (the position is read); else not read
  const float4* boxes;      // PARALLAX: n_probes rt_reflection_box, 2 float4 each; else not read
  const float4* queries;    // n rt_reflection_query, 2 float4 each
  float4* out;              // n texels
  uint32_t n;               // 1 .. 2^31 - 1
  uint32_t n_probes;        // n_probes * chain < 2^31
  uint32_t chain;           // texels of a chain
  uint32_t size_log2;       // of level 0
  uint32_t levels;          // 2 .. 8, (1 << size_log2) >> (levels - 1) >= 4
};

// k_reflection_sample<parallax> over the A.n queries, 256-thread workgroups, on `stream`; -> hipGetLastError() of the launch
hipError_t launch_reflection_sample(const ReflectionSampleArgs& A, bool parallax, hipStream_t stream);

}  // namespace rtk
#endif
