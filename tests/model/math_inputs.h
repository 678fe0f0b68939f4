// math_inputs.h — the input sets of the math-header check, as plain C++ for BOTH sides: tests/model/math_check.hip
// enumerates them on the GPU and tests/model/math_ref.cpp on the host, each through its own compilation of
// include/mi355rt_math.h (math_ops.h applies the functions).  tests/test_gpu_math.py compares the two by checksum.
//
// An op has an index space [0, math_count(op)).  Index i gives operand words; the op produces R = math_results(op)
// result words, and word c enters the checksum as math_mix(op, bits, R * i + c) (NaN results as one canonical NaN).
// An index outside the op's domain contributes nothing on either side.  Consecutive indices share an exponent class,
// so the wave-uniform guards of k_ieee.hip.h see whole waves on one side, as in the renderer.
//
//   unary (sincos .. abs_sat)   i = the f32 bit pattern, all 2^32.  sincos: biased exponent <= 157 only (|x| < 2^31:
//                               where `(int)kf` of rt_sincos is defined; beyond it the host is undefined behaviour)
//   f16_to_f32                  all 2^16 halves;  pow2i: n = i - 126, i in [0, 254)
//   min max                     2^8 exponent classes (rt_ieee_div_operands) x 2^20 hashed mantissa samples, then every
//                               ordered pair of the 17 special values
//   clamp mix                   the same classes with a hashed third operand, then every ordered TRIPLE of the specials
//   pow                         16 rows that reach each early return of rt_pow, then 512 general pairs
//   vec3 / mat4 group           2^24 samples with biased exponents 107 .. 147, then 2^20 with the exponents of
//                               rt_ieee_exp_tab (zero / denormal .. inf / NaN), 4096 samples per exponent pair
//   rgbe8                       2^8 exponents of the largest channel x 2^16 samples
//   resize_coord                15 source sizes x every destination texel of 1024
//   bilinear_u8                 2^24 hashed quads
//   init_rng, rand_pcg          the kernels' RNG (csrc/k_common.hip.h, device only): 2^20 (pixel, frame) pairs, and every one
//                               of the 2^32 states (results: the float and the state left behind).  The host side of these
//                               two is not this directory's: the reference renderer's own functions, through its library
#ifndef MI355RT_TESTS_MATH_INPUTS_H
#define MI355RT_TESTS_MATH_INPUTS_H
#include <stdint.h>

#include "../../webgpu-raytracer_amd/csrc/k_ieee_inputs.h"   // rt_ieee_hash32 / exp_tab / mantissa / div_operands / canon / mix

#define MATH_HD RT_IEEE_HD

//        name            results
#define MATH_OPS(X)       \
  X(sincos, 2)            \
  X(exp, 1)               \
  X(log, 1)               \
  X(pow22, 1)             \
  X(floor, 1)             \
  X(f2u32_sat, 1)         \
  X(f2i32_sat, 1)         \
  X(f32_to_f16, 1)        \
  X(unorm8, 1)            \
  X(abs_sat, 2)           \
  X(f16_to_f32, 1)        \
  X(pow2i, 1)             \
  X(min, 1)               \
  X(max, 1)               \
  X(clamp, 1)             \
  X(mix, 1)               \
  X(pow, 1)               \
  X(dot, 1)               \
  X(cross, 3)             \
  X(length, 1)            \
  X(normalize, 3)         \
  X(reflect, 3)           \
  X(refract, 3)           \
  X(mix3, 3)              \
  X(minmax3, 6)           \
  X(clamp3, 3)            \
  X(div3s, 3)             \
  X(div3z, 3)             \
  X(rcp3, 3)              \
  X(div_pi3, 3)           \
  X(div33, 3)             \
  X(mat_mul_point, 3)     \
  X(mat_mul_dir, 3)       \
  X(vec_mul_mat_dir, 3)   \
  X(rgbe8, 1)             \
  X(resize_coord, 3)      \
  X(bilinear_u8, 1)       \
  X(init_rng, 1)          \
  X(rand_pcg, 2)

enum {
#define MATH_X(name, r) MATH_OP_##name,
  MATH_OPS(MATH_X)
#undef MATH_X
  MATH_OP_COUNT
};
enum { MATH_MAX_RESULTS = 8, MATH_MAX_OPERANDS = 28 };

MATH_HD int math_results(int op) {
  switch (op) {
#define MATH_X(name, r) case MATH_OP_##name: return r;
    MATH_OPS(MATH_X)
#undef MATH_X
  }
  return 0;
}

// Float results enter the checksum with NaNs as one canonical NaN (rt_ieee_mix); integer results enter as they are (a
// packed word such as rt_rgbe8's may look like a NaN and must not be folded).
MATH_HD int math_result_is_float(int op) {
  return !(op == MATH_OP_f2u32_sat || op == MATH_OP_f2i32_sat || op == MATH_OP_f32_to_f16 || op == MATH_OP_unorm8 || op == MATH_OP_rgbe8 ||
           op == MATH_OP_resize_coord || op == MATH_OP_bilinear_u8 || op == MATH_OP_init_rng || op == MATH_OP_rand_pcg);
}
MATH_HD uint64_t math_mix(int op, uint32_t bits, uint64_t k) { return math_result_is_float(op) ? rt_ieee_mix(bits, k) : (uint64_t)bits * (2u * k + 1u); }

#define MATH_POW22_Y 0.4545454680919647216796875f   // f32(1 / 2.2), the post pass's exponent

// ---------------------------------------------------------------------------------------------- the special values
enum { MATH_N_SPECIAL = 17, MATH_GENERAL_BITS = 28, MATH_POW_TABLE = 16, MATH_POW_GENERAL = 512,
       MATH_VEC_NARROW_BITS = 24, MATH_VEC_WIDE_BITS = 20, MATH_N_RESIZE_SRC = 15 };
MATH_HD uint32_t math_special(uint32_t k) {
  const uint32_t t[MATH_N_SPECIAL] = {
      0x00000000u, 0x80000000u,   // +-0
      0x00000001u, 0x80000001u,   // +- the smallest denormal
      0x007fffffu, 0x807fffffu,   // +- the largest denormal
      0x00800000u, 0x80800000u,   // +-2^-126
      0x3f800000u, 0xbf800000u,   // +-1
      0x7f7fffffu, 0xff7fffffu,   // +- the largest finite
      0x7f800000u, 0xff800000u,   // +-inf
      0x7fc00000u, 0xffc00000u,   // qNaN, -qNaN
      0x7fa00000u};               // sNaN
  return t[k % MATH_N_SPECIAL];
}

MATH_HD uint64_t math_count(int op) {
  const uint64_t general = 1ull << MATH_GENERAL_BITS;
  switch (op) {
    case MATH_OP_f16_to_f32: return 1ull << 16;
    case MATH_OP_pow2i: return 254;
    case MATH_OP_min: case MATH_OP_max: return general + MATH_N_SPECIAL * MATH_N_SPECIAL;
    case MATH_OP_clamp: case MATH_OP_mix: return general + MATH_N_SPECIAL * MATH_N_SPECIAL * MATH_N_SPECIAL;
    case MATH_OP_pow: return MATH_POW_TABLE + MATH_POW_GENERAL;
    case MATH_OP_rgbe8: case MATH_OP_bilinear_u8: return 1ull << 24;
    case MATH_OP_resize_coord: return (uint64_t)MATH_N_RESIZE_SRC * 1024u;
    case MATH_OP_init_rng: return 1ull << 20;
    default: break;
  }
  if (op >= MATH_OP_dot && op <= MATH_OP_vec_mul_mat_dir) return (1ull << MATH_VEC_NARROW_BITS) + (1ull << MATH_VEC_WIDE_BITS);
  return 1ull << 32;   // the unary ops
}

// word j of sample i: one 32-bit hash per (sample, slot)
MATH_HD uint32_t math_word(uint64_t i, uint32_t j) { return rt_ieee_hash32((uint32_t)i * 0x9e3779b1u + j * 0x85ebca6bu + 0x27d4eb2fu); }
// a float in [0, 1): no arithmetic, so the operand is the same word wherever it is made.  2^-k * [1, 2) for a hashed k
MATH_HD uint32_t math_unit_bits(uint32_t h) {
  const uint32_t k = 1u + ((h >> 23) & 7u);
  if ((h >> 26) == 0u) return 0u;                     // 1 in 64: exactly 0
  if ((h >> 26) == 1u) return 0x3f800000u;            // 1 in 64: exactly 1
  return ((127u - k) << 23) | (h & 0x7fffffu);
}

// -------------------------------------------------------------------------------------- two and three scalar operands
// general part: class e = i >> 20 (16 x 16 exponents), sample m = i & 0xfffff; then the specials block
MATH_HD void math_scalar_operands(int op, uint64_t i, uint32_t* a, uint32_t* b, uint32_t* c) {
  const uint64_t general = 1ull << MATH_GENERAL_BITS;
  if (i >= general) {
    const uint32_t k = (uint32_t)(i - general);
    *a = math_special(k % MATH_N_SPECIAL);
    *b = math_special((k / MATH_N_SPECIAL) % MATH_N_SPECIAL);
    *c = math_special((k / (MATH_N_SPECIAL * MATH_N_SPECIAL)) % MATH_N_SPECIAL);
    return;
  }
  const uint32_t e = (uint32_t)(i >> 20) & 255u, m = (uint32_t)i & 0xfffffu;
  rt_ieee_div_operands(((uint64_t)e << 24) | m, a, b);
  const uint32_t h = math_word(i, 1u);
  if (op == MATH_OP_mix && (m & 1u) == 0u) {
    *c = math_unit_bits(h);                           // half of mix's samples: t in [0, 1]
  } else {
    // the third operand near one of the other two in magnitude (so a clamp really clamps), or anywhere at all
    const uint32_t near = (h & 4u) ? *a : *b;
    const uint32_t ex = (h & 8u) ? rt_ieee_exp_tab(h >> 28) : ((near >> 23) & 255u);
    *c = ((h & 1u) << 31) | (ex << 23) | rt_ieee_mantissa(m, 0x2545f491u);
  }
  if ((op == MATH_OP_min || op == MATH_OP_max) && (m & 15u) == 5u) *b = (*b & 0x80000000u) | (*a & 0x7fffffffu);   // |a| == |b|
}

// pow(x, y): rows 0 .. 15 reach each early return of rt_pow, then hashed pairs
MATH_HD void math_pow_operands(uint64_t i, uint32_t* x, uint32_t* y) {
  const uint32_t ys[4] = {0x40000000u /* 2 */, 0x00000000u, 0x80000000u, 0xbfc00000u /* -1.5 */};
  const uint32_t y1[8] = {0x00000000u, 0x3ee8ba2fu, 0xc0400000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0x00000001u, 0x3f800000u};
  if (i < 4u) { *x = 0x00000000u; *y = ys[i]; return; }
  if (i < 8u) { *x = 0x80000000u; *y = ys[i - 4u]; return; }
  if (i < MATH_POW_TABLE) { *x = 0x3f800000u; *y = y1[i - 8u]; return; }
  const uint32_t h = math_word(i, 0u), g = math_word(i, 1u);
  // x: mostly positive around 1 (2^-20 .. 2^20), some anywhere; y: |y| in 2^-4 .. 2^4, some anywhere
  const uint32_t ex = (h & 15u) == 0u ? rt_ieee_exp_tab(h >> 28) : 107u + (h >> 8) % 41u;
  const uint32_t ey = (g & 15u) == 0u ? rt_ieee_exp_tab(g >> 28) : 123u + (g >> 8) % 9u;
  *x = (((h >> 4) & 15u) == 0u ? 0x80000000u : 0u) | (ex << 23) | (math_word(i, 2u) & 0x7fffffu);
  *y = ((g >> 4) << 31) | (ey << 23) | (math_word(i, 3u) & 0x7fffffu);
}

// ------------------------------------------------------------------------------------------------ vec3 / mat4 group
// 0 .. 2^24: every component a hashed mantissa with a biased exponent in 107 .. 147 (a block of 4096 samples shares a base
// exponent; components sit within +-2 of it).  Then 2^20: 256 exponent pairs (rt_ieee_exp_tab) x 4096 samples; words
// 0 .. 8 take the first exponent of the pair, the rest the second.
MATH_HD uint32_t math_vec_word(uint64_t i, uint32_t j) {
  const uint64_t narrow = 1ull << MATH_VEC_NARROW_BITS;
  const uint32_t h = math_word(i, 16u + j);
  uint32_t ex;
  if (i < narrow) {
    const uint32_t base = 109u + (uint32_t)(i >> 12) % 37u;      // 109 .. 145
    ex = base + (h >> 24) % 5u - 2u;                              // 107 .. 147
  } else {
    const uint32_t cls = (uint32_t)((i - narrow) >> 12) & 255u;
    ex = rt_ieee_exp_tab(j < 9u ? cls >> 4 : cls & 15u);
  }
  return ((h & 1u) << 31) | (ex << 23) | rt_ieee_mantissa(((h >> 4) & 15u) == 0u ? (h >> 9) & 4095u : 4096u + (h >> 1), 0x9e3779b9u + j);
}
// a vector close to unit length: an exact-ish unit triple, permuted and signed, its low mantissa bits perturbed
MATH_HD void math_unit_vec(uint64_t i, uint32_t slot, uint32_t v[3]) {
  const uint32_t t[8][3] = {
      {0x3f800000u, 0x00000000u, 0x00000000u},   // 1 0 0
      {0x3f19999au, 0x3f4ccccdu, 0x00000000u},   // .6 .8 0
      {0x3f2aaaabu, 0x3f2aaaabu, 0x3eaaaaabu},   // 2/3 2/3 1/3
      {0x3e6c4ec5u, 0x3e9d89d9u, 0x3f6c4ec5u},   // 3/13 4/13 12/13
      {0x3eb851ecu, 0x3ef5c28fu, 0x3f4ccccdu},   // .36 .48 .8
      {0x3e924925u, 0x3edb6db7u, 0x3f5b6db7u},   // 2/7 3/7 6/7
      {0x3de38e39u, 0x3ee38e39u, 0x3f638e39u},   // 1/9 4/9 8/9
      {0x3f13cd3au, 0x3f13cd3au, 0x3f13cd3au}};  // 1/sqrt(3) each
  const uint32_t h = math_word(i, 48u + slot);
  const uint32_t k = h & 7u, rot = (h >> 3) % 3u;
  for (uint32_t c = 0; c < 3u; c++) {
    const uint32_t w = t[k][(c + rot) % 3u];
    const uint32_t flip = (w & 0x7fffffffu) ? ((h >> (8u + 10u * c)) & 0x3ffu) : 0u;   // keep exact zeros
    v[c] = (w ^ flip) | (((h >> (5u + c)) & 1u) << 31);
  }
}
// eta in [0.4, 2.5]: positive floats order as their bits do
MATH_HD uint32_t math_eta_bits(uint64_t i) { return 0x3ecccccdu + math_word(i, 60u) % (0x40200000u - 0x3ecccccdu + 1u); }

// ------------------------------------------------------------------------------------------------------------ rgbe8
// class e = i >> 16: the biased exponent of the largest channel, 0 .. 255 (below 32 encodes as 0; 254 and 255 meet the
// `top` clamp).  The other channels lie up to 11 binades below, or are negative, zero or NaN.  w == -1 in 1 of 16.
MATH_HD void math_rgbe_operands(uint64_t i, uint32_t ch[3], uint32_t* w) {
  const uint32_t e = (uint32_t)(i >> 16) & 255u;
  const uint32_t h = math_word(i, 0u), g = math_word(i, 1u);
  const uint32_t big = h % 3u;
  for (uint32_t c = 0; c < 3u; c++) {
    const uint32_t hc = math_word(i, 2u + c);
    const uint32_t drop = c == big ? 0u : (hc >> 24) % 12u;
    const uint32_t ex = e > drop ? e - drop : 0u;
    uint32_t bits = (ex << 23) | rt_ieee_mantissa(((uint32_t)i & 0xffffu) < 64u ? (hc >> 9) & 4095u : 4096u + (hc >> 1), 0x7f4a7c15u + c);
    const uint32_t kind = (hc >> 3) & 31u;
    if (c != big || (g & 15u) == 1u) {                // the largest channel stays a plain positive number in 15 of 16
      if (kind < 4u) bits |= 0x80000000u;             // negative
      else if (kind == 4u) bits = 0u;                 // +0
      else if (kind == 5u) bits = 0x80000000u;        // -0
      else if (kind == 6u) bits = 0x7fc00000u | (hc & 0x80000000u);   // NaN
    }
    ch[c] = bits;
  }
  const uint32_t wsel = (g >> 4) & 15u;
  // -1 (the "no texel" mark), the two neighbours of -1, NaN, and otherwise 1
  *w = wsel == 0u ? 0xbf800000u : (wsel == 1u ? 0xbf800001u - ((g >> 8) & 2u) : (wsel == 2u ? 0x7fc00000u : 0x3f800000u));
}

// ----------------------------------------------------------------------------------------------------- texture resize
MATH_HD uint32_t math_resize_src(uint32_t k) {   // 32768: the largest size rt_upload_texture_image accepts
  const uint32_t t[MATH_N_RESIZE_SRC] = {1u, 2u, 3u, 7u, 31u, 300u, 517u, 640u, 1023u, 1024u, 1025u, 1500u, 2048u, 4096u, 32768u};
  return t[k % MATH_N_RESIZE_SRC];
}
// a quad of bytes c[4]; weight selectors: kind 0 = a rt_resize_coord output for (d, src), 1 = 0, 2 = the largest f32 below 1
MATH_HD void math_bilinear_operands(uint64_t i, uint32_t c[4], uint32_t sel[2][3]) {
  const uint32_t h = math_word(i, 0u), m = (uint32_t)i & 63u;
  for (uint32_t k = 0; k < 4u; k++) c[k] = m == 0u ? 0u : (m == 1u ? 255u : (h >> (8u * k)) & 255u);
  for (uint32_t a = 0; a < 2u; a++) {
    const uint32_t g = math_word(i, 1u + a);
    const uint32_t kind = (g & 15u) == 0u ? 1u : ((g & 15u) == 1u ? 2u : 0u);
    sel[a][0] = kind;
    sel[a][1] = (g >> 4) & 1023u;                 // d
    sel[a][2] = math_resize_src(g >> 14);         // src
  }
}

// ------------------------------------------------------------------------------------------------------------- RNG
// (pixel, frame): pixels of images up to 8192 x 8192 and the first few in order; frames small, large, and any 32-bit word
MATH_HD void math_rng_operands(uint64_t i, uint32_t* pixel, uint32_t* frame) {
  const uint32_t h = math_word(i, 0u), g = math_word(i, 1u);
  *pixel = ((uint32_t)i & 3u) == 0u ? (uint32_t)i >> 2 : (((uint32_t)i & 3u) == 1u ? h : h % (8192u * 8192u));
  *frame = ((uint32_t)i & 12u) == 0u ? (uint32_t)i >> 4 : (((uint32_t)i & 12u) == 4u ? g : g % 100000u);
}

#endif
