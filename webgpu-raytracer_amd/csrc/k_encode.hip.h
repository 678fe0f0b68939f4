// k_encode.hip.h — k_encode_atlas: a 16-byte-per-texel f32 atlas into the texel format a renderer loads, half floats or the
// shared-exponent word of a Radiance .hdr pixel (rt_encode_atlas and the last stage of rt_bake_atlas_lightmap, mi355rt.h
// "lightmaps").
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_ENCODE_HIP_H
#define MI355RT_K_ENCODE_HIP_H

namespace rtk {

// One thread per texel, 256 per workgroup: one 16-byte load, then one 8-byte store (RT_LIGHTMAP_F16: four rt_f32_to_f16, w
// included) or one 4-byte store (RT_LIGHTMAP_RGBE8: rt_rgbe8 of mi355rt_math.h, integer exponent work, one exact multiply per
// channel).  The format is a kernel argument, hence wave-uniform.  A streaming kernel: no LDS, no atomics, and texel i of `out`
// depends on texel i of `in` alone.  RT_LIGHTMAP_F32 is a copy and never comes here: the host copies.
struct EncodeArgs {
  const uint4* in;          // n texels {r, g, b, w}
  void* out;                // n uint2 (F16) or n uint32_t (RGBE8); not `in`
  uint32_t n;               // W * H <= 2^24
  uint32_t format;          // RT_LIGHTMAP_F16 or RT_LIGHTMAP_RGBE8
};

__global__ __launch_bounds__(256)
void k_encode_atlas(EncodeArgs A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= A.n) return;
  const uint4 t = A.in[i];
  const float r = __uint_as_float(t.x), g = __uint_as_float(t.y), b = __uint_as_float(t.z), w = __uint_as_float(t.w);
  if (A.format == RT_LIGHTMAP_F16) {
    uint2 h;
    h.x = (uint32_t)rt_f32_to_f16(r) | ((uint32_t)rt_f32_to_f16(g) << 16);
    h.y = (uint32_t)rt_f32_to_f16(b) | ((uint32_t)rt_f32_to_f16(w) << 16);
    ((uint2*)A.out)[i] = h;
  } else {
    ((uint32_t*)A.out)[i] = rt_rgbe8(r, g, b, w);
  }
}

}  // namespace rtk
#endif
