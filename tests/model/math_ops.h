// math_ops.h — applies the functions of include/mi355rt_math.h to the operands of math_inputs.h.  Included AFTER the
// math header by both sides of the check (tests/model/math_check.hip for gfx950, tests/model/math_ref.cpp for the host),
// so each side calls its own compilation of the header; nothing here does arithmetic of its own.
//
// math_eval<OP>(i, w, opnd, n_opnd): the result words of index i into w[], returns how many (0: i is outside the op's
// domain).  opnd (may be null): the operand words, for the report of a mismatch.
//
// init_rng / rand_pcg are not functions of the math header: the includer names them (MATH_INIT_RNG(pixel, frame),
// MATH_RAND_PCG(state lvalue)) — math_check.hip the kernels' own of csrc/k_common.hip.h.  Where they are not named, as on
// the host, the two ops produce nothing.
#ifndef MI355RT_TESTS_MATH_OPS_H
#define MI355RT_TESTS_MATH_OPS_H

#include "math_inputs.h"

#define MATH_OPND(k, v)            \
  do {                             \
    if (opnd) opnd[k] = (v);       \
    if (n_opnd && *n_opnd < (k) + 1) *n_opnd = (k) + 1; \
  } while (0)

MATH_HD rt3 math_rt3(const uint32_t v[3]) { return rt3_make(rt_u2f(v[0]), rt_u2f(v[1]), rt_u2f(v[2])); }
MATH_HD void math_put3(uint32_t* w, rt3 v) { w[0] = rt_f2u(v.x); w[1] = rt_f2u(v.y); w[2] = rt_f2u(v.z); }

template <int OP>
MATH_HD int math_eval(uint64_t i, uint32_t w[MATH_MAX_RESULTS], uint32_t* opnd, int* n_opnd) {
  if (n_opnd) *n_opnd = 0;
  if (i >= math_count(OP)) return 0;
  // ------------------------------------------------------------------------------------------------ one operand
  if (OP <= MATH_OP_abs_sat) {
    const uint32_t u = (uint32_t)i;
    const float x = rt_u2f(u);
    MATH_OPND(0, u);
    if (OP == MATH_OP_sincos) {
      if (((u >> 23) & 255u) > 157u) return 0;
      float s, c;
      rt_sincos(x, &s, &c);
      w[0] = rt_f2u(s); w[1] = rt_f2u(c);
    } else if (OP == MATH_OP_exp) w[0] = rt_f2u(rt_exp(x));
    else if (OP == MATH_OP_log) w[0] = rt_f2u(rt_log(x));
    else if (OP == MATH_OP_pow22) w[0] = rt_f2u(rt_pow(x, MATH_POW22_Y));
    else if (OP == MATH_OP_floor) w[0] = rt_f2u(rt_floor(x));
    else if (OP == MATH_OP_f2u32_sat) w[0] = rt_f2u32_sat(x);
    else if (OP == MATH_OP_f2i32_sat) w[0] = (uint32_t)rt_f2i32_sat(x);
    else if (OP == MATH_OP_f32_to_f16) w[0] = rt_f32_to_f16(x);
    else if (OP == MATH_OP_unorm8) w[0] = rt_unorm8(x);
    else { w[0] = rt_f2u(rt_abs(x)); w[1] = rt_f2u(rt_saturate(x)); }
    return math_results(OP);
  }
  if (OP == MATH_OP_f16_to_f32) {
    MATH_OPND(0, (uint32_t)i);
    w[0] = rt_f2u(rt_f16_to_f32((uint16_t)i));
    return 1;
  }
  if (OP == MATH_OP_pow2i) {
    MATH_OPND(0, (uint32_t)((int)i - 126));
    w[0] = rt_f2u(rt_pow2i((int)i - 126));
    return 1;
  }
  // --------------------------------------------------------------------------------------- two / three scalars
  if (OP == MATH_OP_min || OP == MATH_OP_max || OP == MATH_OP_clamp || OP == MATH_OP_mix) {
    uint32_t a, b, c;
    math_scalar_operands(OP, i, &a, &b, &c);
    MATH_OPND(0, a); MATH_OPND(1, b);
    if (OP == MATH_OP_min) w[0] = rt_f2u(rt_min(rt_u2f(a), rt_u2f(b)));
    else if (OP == MATH_OP_max) w[0] = rt_f2u(rt_max(rt_u2f(a), rt_u2f(b)));
    else {
      MATH_OPND(2, c);
      w[0] = rt_f2u(OP == MATH_OP_clamp ? rt_clamp(rt_u2f(a), rt_u2f(b), rt_u2f(c)) : rt_mix(rt_u2f(a), rt_u2f(b), rt_u2f(c)));
    }
    return 1;
  }
  if (OP == MATH_OP_pow) {
    uint32_t x, y;
    math_pow_operands(i, &x, &y);
    MATH_OPND(0, x); MATH_OPND(1, y);
    w[0] = rt_f2u(rt_pow(rt_u2f(x), rt_u2f(y)));
    return 1;
  }
  // ---------------------------------------------------------------------------------------------- vec3 / mat4
  if (OP >= MATH_OP_dot && OP <= MATH_OP_vec_mul_mat_dir) {
    const bool narrow = i < (1ull << MATH_VEC_NARROW_BITS);
    uint32_t av[3], bv[3], cv[3];
    for (uint32_t c = 0; c < 3u; c++) { av[c] = math_vec_word(i, c); bv[c] = math_vec_word(i, 9u + c); cv[c] = math_vec_word(i, 12u + c); }
    if (OP == MATH_OP_div3z && ((uint32_t)i & 7u) == 3u) { const uint32_t h = math_word(i, 61u); av[(h >> 4) % 3u] = (h & 1u) << 31; }
    if (OP == MATH_OP_refract) {
      if (narrow) math_unit_vec(i, 0u, av);
      math_unit_vec(i, 1u, bv);
    }
    if (OP == MATH_OP_reflect && ((uint32_t)i & 1u) == 0u) math_unit_vec(i, 1u, bv);
    for (int c = 0; c < 3; c++) MATH_OPND(c, av[c]);
    const rt3 a = math_rt3(av), b = math_rt3(bv);
    if (OP == MATH_OP_dot || OP == MATH_OP_cross || OP == MATH_OP_reflect || OP == MATH_OP_minmax3 || OP == MATH_OP_div33) {
      for (int c = 0; c < 3; c++) MATH_OPND(3 + c, bv[c]);
      if (OP == MATH_OP_dot) w[0] = rt_f2u(rt_dot(a, b));
      else if (OP == MATH_OP_cross) math_put3(w, rt_cross(a, b));
      else if (OP == MATH_OP_reflect) math_put3(w, rt_reflect(a, b));
      else if (OP == MATH_OP_div33) math_put3(w, a / b);
      else { math_put3(w, rt_min3(a, b)); math_put3(w + 3, rt_max3(a, b)); }
    } else if (OP == MATH_OP_length) w[0] = rt_f2u(rt_length(a));
    else if (OP == MATH_OP_normalize) math_put3(w, rt_normalize(a));
    else if (OP == MATH_OP_rcp3) math_put3(w, rt_rcp3(a));
    else if (OP == MATH_OP_div_pi3) math_put3(w, rt_div_pi3(a));
    else if (OP == MATH_OP_refract) {
      const uint32_t eta = math_eta_bits(i);
      for (int c = 0; c < 3; c++) MATH_OPND(3 + c, bv[c]);
      MATH_OPND(6, eta);
      math_put3(w, rt_refract(a, b, rt_u2f(eta)));
    } else if (OP == MATH_OP_mix3) {
      const uint32_t t = ((uint32_t)i & 1u) ? math_vec_word(i, 15u) : math_unit_bits(math_word(i, 62u));
      for (int c = 0; c < 3; c++) MATH_OPND(3 + c, bv[c]);
      MATH_OPND(6, t);
      math_put3(w, rt_mix3(a, b, rt_u2f(t)));
    } else if (OP == MATH_OP_clamp3) {
      for (int c = 0; c < 3; c++) { MATH_OPND(3 + c, bv[c]); MATH_OPND(6 + c, cv[c]); }
      math_put3(w, rt_clamp3(a, b, math_rt3(cv)));
    } else if (OP == MATH_OP_div3s || OP == MATH_OP_div3z) {
      MATH_OPND(3, bv[0]);
      math_put3(w, OP == MATH_OP_div3s ? a / rt_u2f(bv[0]) : rt_div3z(a, rt_u2f(bv[0])));
    } else {
      float m[16];
      for (uint32_t k = 0; k < 16u; k++) {
        const uint32_t mw = math_vec_word(i, 9u + k);
        MATH_OPND(3 + (int)k, mw);
        m[k] = rt_u2f(mw);
      }
      math_put3(w, OP == MATH_OP_mat_mul_point ? rt_mat_mul_point(m, a) : (OP == MATH_OP_mat_mul_dir ? rt_mat_mul_dir(m, a) : rt_vec_mul_mat_dir(a, m)));
    }
    return math_results(OP);
  }
  if (OP == MATH_OP_rgbe8) {
    uint32_t ch[3], ww;
    math_rgbe_operands(i, ch, &ww);
    for (int c = 0; c < 3; c++) MATH_OPND(c, ch[c]);
    MATH_OPND(3, ww);
    w[0] = rt_rgbe8(rt_u2f(ch[0]), rt_u2f(ch[1]), rt_u2f(ch[2]), rt_u2f(ww));
    return 1;
  }
  if (OP == MATH_OP_resize_coord) {
    const uint32_t d = (uint32_t)i & 1023u, src = math_resize_src((uint32_t)(i >> 10));
    MATH_OPND(0, d); MATH_OPND(1, src);
    uint32_t i0, i1;
    const float f = rt_resize_coord(d, src, 1024u, &i0, &i1);
    w[0] = i0; w[1] = i1; w[2] = rt_f2u(f);
    return 3;
  }
  if (OP == MATH_OP_bilinear_u8) {
    uint32_t c[4], sel[2][3];
    math_bilinear_operands(i, c, sel);
    float f[2];
    for (int a = 0; a < 2; a++) {
      uint32_t i0, i1;
      f[a] = sel[a][0] == 1u ? 0.0f : (sel[a][0] == 2u ? rt_u2f(0x3f7fffffu) : rt_resize_coord(sel[a][1], sel[a][2], 1024u, &i0, &i1));
    }
    for (int k = 0; k < 4; k++) MATH_OPND(k, c[k]);
    MATH_OPND(4, rt_f2u(f[0])); MATH_OPND(5, rt_f2u(f[1]));
    w[0] = rt_bilinear_u8(c[0], c[1], c[2], c[3], f[0], f[1]);
    return 1;
  }
#if defined(MATH_INIT_RNG) && defined(MATH_RAND_PCG)
  if (OP == MATH_OP_init_rng) {
    uint32_t pixel, frame;
    math_rng_operands(i, &pixel, &frame);
    MATH_OPND(0, pixel); MATH_OPND(1, frame);
    w[0] = MATH_INIT_RNG(pixel, frame);
    return 1;
  }
  if (OP == MATH_OP_rand_pcg) {
    uint32_t state = (uint32_t)i;
    MATH_OPND(0, state);
    w[0] = rt_f2u(MATH_RAND_PCG(state));
    w[1] = state;
    return 2;
  }
#endif
  return 0;
}

#endif
