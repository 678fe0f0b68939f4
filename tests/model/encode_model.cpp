// encode_model.cpp — the host side of the two functions k_encode_atlas applies per texel (rt_rgbe8 and rt_f32_to_f16 of
// include/mi355rt_math.h), over arrays, so that tests/test_encode_model.py can hold the very source the device compiles to
// the numpy restatement of the encoding rule (tests/encode_util.py).  Built by encode_util.host_lib().
#include <cstdint>

#include "mi355rt_math.h"

extern "C" {

// n texels {r, g, b, w} -> n RGBE8 words
void encode_host_rgbe8(const float* atlas, uint32_t n, uint32_t* out) {
  for (uint32_t i = 0; i < n; i++) out[i] = rt_rgbe8(atlas[4 * i], atlas[4 * i + 1], atlas[4 * i + 2], atlas[4 * i + 3]);
}

// n floats -> n half bit patterns
void encode_host_f16(const float* in, uint32_t n, uint16_t* out) {
  for (uint32_t i = 0; i < n; i++) out[i] = rt_f32_to_f16(in[i]);
}

}
