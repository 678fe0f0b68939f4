// reflection_sample.hip — the reflection sampler's translation unit: k_reflection_sample<PARALLAX> (k_reflection_sample.hip.h)
// and its launcher, built with the library's flags and linked into libmi355rt.so beside rt_api.hip, which holds the entries
// (rt_sample_reflection, rt_sample_reflection_device) and their checks.
#include "reflection_sample.h"

#include "k_ieee.hip.h"   // before the math header: the device build's correctly rounded rcp / div sequences
#include "../../include/mi355rt_math.h"
#include "k_reflection_sample.hip.h"

namespace rtk {

hipError_t launch_reflection_sample(const ReflectionSampleArgs& A, bool parallax, hipStream_t stream) {
  const dim3 blocks((A.n + 255u) / 256u);
  if (parallax)
    hipLaunchKernelGGL(k_reflection_sample<true>, blocks, dim3(256), 0, stream, A);
  else
    hipLaunchKernelGGL(k_reflection_sample<false>, blocks, dim3(256), 0, stream, A);
  return hipGetLastError();
}

}  // namespace rtk
