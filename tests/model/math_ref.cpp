// math_ref.cpp — the HOST compilation of include/mi355rt_math.h over the input sets of math_inputs.h: the checksums
// tests/test_gpu_math.py compares with the device's (tests/model/math_check.hip), and the exhaustive accuracy sweeps of
// tests/test_math_model.py against double-precision libm.  Test infrastructure; plain C++ with std::thread.
// Built with -O2 -ffp-contract=off -fno-fast-math (tests/math_util.py).  -DMATH_REF_MAIN adds a main() that prints every
// op's checksum over the reduced enumeration (the stand-alone program the undefined-behaviour sanitizer runs).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include "../../include/mi355rt_math.h"

#include "math_ops.h"

typedef int (*eval_fn)(uint64_t, uint32_t*, uint32_t*, int*);
static eval_fn eval_of(int op) {
  switch (op) {
#define MATH_X(name, r) case MATH_OP_##name: return math_eval<MATH_OP_##name>;
    MATH_OPS(MATH_X)
#undef MATH_X
  }
  return nullptr;
}
static const char* const k_names[] = {
#define MATH_X(name, r) #name,
    MATH_OPS(MATH_X)
#undef MATH_X
};

template <int OP>
static void range_sum(uint64_t lo, uint64_t hi, uint64_t* sum, uint64_t* n_in) {
  const uint64_t R = (uint64_t)math_results(OP);
  uint64_t s = 0, n = 0;
  for (uint64_t i = lo; i < hi; i++) {
    uint32_t w[MATH_MAX_RESULTS];
    const int nres = math_eval<OP>(i, w, nullptr, nullptr);
    n += nres > 0;
    for (int c = 0; c < nres; c++) s += math_mix(OP, w[c], R * i + (uint64_t)c);
  }
  *sum += s;
  *n_in += n;
}
typedef void (*range_fn)(uint64_t, uint64_t, uint64_t*, uint64_t*);
static range_fn range_of(int op) {
  switch (op) {
#define MATH_X(name, r) case MATH_OP_##name: return range_sum<MATH_OP_##name>;
    MATH_OPS(MATH_X)
#undef MATH_X
  }
  return nullptr;
}

template <class F>
static void parallel(uint64_t first, uint64_t count, int threads, F body) {   // body(thread, lo, hi)
  if (threads < 1) threads = 1;
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; t++)
    pool.emplace_back([=]() {
      // 128-bit products: count may be 2^32 and threads 16
      const uint64_t lo = first + (uint64_t)((unsigned __int128)count * (unsigned)t / (unsigned)threads);
      const uint64_t hi = first + (uint64_t)((unsigned __int128)count * (unsigned)(t + 1) / (unsigned)threads);
      body(t, lo, hi);
    });
  for (auto& th : pool) th.join();
}

static void sweep(int op, uint64_t first, uint64_t count, int threads, uint64_t* sum, uint64_t* n_in) {
  *sum = *n_in = 0;
  const range_fn fn = range_of(op);
  if (!fn || count == 0) return;
  if (threads < 1) threads = 1;
  std::vector<uint64_t> s((size_t)threads, 0), n((size_t)threads, 0);
  parallel(first, count, threads, [&](int t, uint64_t lo, uint64_t hi) { fn(lo, hi, &s[(size_t)t], &n[(size_t)t]); });
  for (int t = 0; t < threads; t++) { *sum += s[(size_t)t]; *n_in += n[(size_t)t]; }
}

extern "C" {
int math_ref_op_count(void) { return MATH_OP_COUNT; }
const char* math_ref_op_name(int op) { return op >= 0 && op < MATH_OP_COUNT ? k_names[op] : ""; }
int math_ref_op_results(int op) { return math_results(op); }
uint64_t math_ref_op_size(int op) { return op >= 0 && op < MATH_OP_COUNT ? math_count(op) : 0; }

uint64_t math_ref_checksum(int op, uint64_t first, uint64_t count, int threads) {
  uint64_t s, n;
  sweep(op, first, count, threads, &s, &n);
  return s;
}
uint64_t math_ref_in_domain(int op, uint64_t first, uint64_t count, int threads) {
  uint64_t s, n;
  sweep(op, first, count, threads, &s, &n);
  return n;
}
void math_ref_sweep(int op, uint64_t first, uint64_t count, int threads, uint64_t* checksum, uint64_t* in_domain) {   // both in one pass
  sweep(op, first, count, threads, checksum, in_domain);
}
// the (pixel, frame) operands of init_rng samples [first, first + count): its host side is the reference renderer's library
void math_ref_rng_pairs(uint64_t first, uint64_t count, uint32_t* pixel_out, uint32_t* frame_out) {
  for (uint64_t k = 0; k < count; k++) math_rng_operands(first + k, &pixel_out[k], &frame_out[k]);
}
// the result words of index i (returns how many; 0: outside the domain) and, if asked for, its operand words
int math_ref_value(int op, uint64_t i, uint32_t* words_out) {
  const eval_fn fn = eval_of(op);
  return fn ? fn(i, words_out, nullptr, nullptr) : 0;
}
int math_ref_operands(int op, uint64_t i, uint32_t* operands_out) {
  const eval_fn fn = eval_of(op);
  uint32_t w[MATH_MAX_RESULTS];
  int n = 0;
  if (fn) fn(i, w, operands_out, &n);
  return n;
}
}

// ------------------------------------------------------------------------------------------- the reduced enumeration
// Every exponent class of every op with about 2^12 samples each: what the compiler-agreement, sanitizer and contraction
// tests run.  j -> an index of the full enumeration.
static uint64_t reduced_count(int op) {
  const uint64_t n = math_count(op);
  if (n == (1ull << 32)) return 512ull << 12;                                       // 2 signs x 256 exponents x 4096 mantissas
  if (op >= MATH_OP_min && op <= MATH_OP_mix) return (256ull << 12) + (n - (1ull << MATH_GENERAL_BITS));
  if (op >= MATH_OP_dot && op <= MATH_OP_vec_mul_mat_dir) return (1ull << 20) + (1ull << MATH_VEC_WIDE_BITS);
  if (op == MATH_OP_rgbe8) return 256ull << 12;
  if (op == MATH_OP_bilinear_u8) return 1ull << 20;
  return n;
}
static uint64_t reduced_index(int op, uint64_t j) {
  const uint64_t n = math_count(op);
  if (n == (1ull << 32)) {
    const uint32_t s = (uint32_t)j & 4095u;
    const uint32_t mant = s < 16u ? s : (s < 32u ? 0x7fffffu - (s - 16u) : rt_ieee_hash32((uint32_t)j) & 0x7fffffu);
    return ((j >> 12) << 23) | mant;
  }
  if (op >= MATH_OP_min && op <= MATH_OP_mix) {
    if (j >= (256ull << 12)) return (1ull << MATH_GENERAL_BITS) + (j - (256ull << 12));
    const uint64_t s = j & 4095u;
    return ((j >> 12) << 20) | (s < 1024u ? s * 4u : s * 255u);   // the corner mantissas (m < 4096) and beyond
  }
  if (op >= MATH_OP_dot && op <= MATH_OP_vec_mul_mat_dir) return j < (1ull << 20) ? j * 16u + (j & 15u) : (1ull << MATH_VEC_NARROW_BITS) + (j - (1ull << 20));
  if (op == MATH_OP_rgbe8) return ((j >> 12) << 16) | ((j & 4095u) * 16u + (j & 15u));
  if (op == MATH_OP_bilinear_u8) return j * 16u + (j & 15u);
  return j;
}
extern "C" uint64_t math_ref_reduced_checksum(int op, int threads) {
  const eval_fn fn = eval_of(op);
  if (!fn) return 0;
  if (threads < 1) threads = 1;
  const uint64_t R = (uint64_t)math_results(op);
  std::vector<uint64_t> part((size_t)threads, 0);
  parallel(0, reduced_count(op), threads, [&](int t, uint64_t lo, uint64_t hi) {
    uint64_t s = 0;
    for (uint64_t j = lo; j < hi; j++) {
      const uint64_t i = reduced_index(op, j);
      uint32_t w[MATH_MAX_RESULTS];
      const int nres = fn(i, w, nullptr, nullptr);
      for (int c = 0; c < nres; c++) s += math_mix(op, w[c], R * i + (uint64_t)c);
    }
    part[(size_t)t] = s;
  });
  uint64_t s = 0;
  for (uint64_t p : part) s += p;
  return s;
}

// ------------------------------------------------------------------------------------ which paths the inputs reach
// out[8], by op:  refract  {k < 0, k >= 0, NaN k}                       rgbe8  {non-zero result, w == -1, exponent < 32, top clamp}
//                 min/max  {general samples with a < b, with a > b, general samples, specials}
//                 pow      {x = 0 y > 0, x = 0 y = 0, x = 0 y < 0, x = 1, general}
extern "C" void math_ref_stats(int op, uint64_t first, uint64_t count, uint64_t out[8]) {
  for (int k = 0; k < 8; k++) out[k] = 0;
  const eval_fn fn = eval_of(op);
  if (!fn) return;
  for (uint64_t i = first; i < first + count; i++) {
    uint32_t w[MATH_MAX_RESULTS], o[MATH_MAX_OPERANDS];
    int n = 0;
    if (fn(i, w, o, &n) == 0) continue;
    if (op == MATH_OP_refract) {
      const rt3 iv = rt3_make(rt_u2f(o[0]), rt_u2f(o[1]), rt_u2f(o[2])), nv = rt3_make(rt_u2f(o[3]), rt_u2f(o[4]), rt_u2f(o[5]));
      const float eta = rt_u2f(o[6]), ni = rt_dot(nv, iv);
      const float k = 1.0f - eta * eta * (1.0f - ni * ni);
      out[k < 0.0f ? 0 : (k >= 0.0f ? 1 : 2)]++;
    } else if (op == MATH_OP_rgbe8) {
      const float top = 1.70141173319264429906e38f;
      float mx = 0.0f;
      bool clamped = false;
      for (int c = 0; c < 3; c++) {
        const float v = rt_u2f(o[c]);
        if (v > 0.0f) { clamped |= !(v < top); mx = v > mx ? v : mx; }
      }
      const bool off = rt_u2f(o[3]) == -1.0f;
      out[0] += w[0] != 0u;
      out[1] += off;
      out[2] += !off && (rt_f2u(mx < top ? mx : top) >> 23) < 32u;
      out[3] += !off && clamped;
    } else if (op == MATH_OP_min || op == MATH_OP_max) {
      if (i < (1ull << MATH_GENERAL_BITS)) {
        out[0] += rt_u2f(o[0]) < rt_u2f(o[1]);
        out[1] += rt_u2f(o[0]) > rt_u2f(o[1]);
        out[2]++;
      } else {
        out[3]++;
      }
    } else if (op == MATH_OP_pow) {
      const float x = rt_u2f(o[0]), y = rt_u2f(o[1]);
      out[x == 0.0f ? (y > 0.0f ? 0 : (y == 0.0f ? 1 : 2)) : (x == 1.0f ? 3 : 4)]++;
    }
  }
}

// ------------------------------------------------------------------------------------------- accuracy against libm
// fn over the f32 bit patterns [first, first + count):
//   0 sin  1 cos  4 pow(x, 1/2.2): max |f - libm| (absolute)         2 exp  3 log: max |f - libm| / ulp(libm), where
//   ulp(v) = 2^(floor(log2 |v|) - 23), the f32 spacing in v's binade (2^-149 below 2^-126)
//   5 unorm8(pow(x, 1/2.2)) against floor(255 pow + 0.5) in double: out_max = number of disagreements, out_aux = the
//     largest difference in codes
//   6 rt_f32_to_f16 / 7 rt_f16_to_f32 against the F16C instructions: out_max = number of differences (any NaN = any NaN)
// out_arg: the input bits where the maximum (or the first difference) occurs.  Returns 0, -1 for an unknown fn, -2 if fn
// needs F16C and this build has none.
enum { ACC_SIN = 0, ACC_COS = 1, ACC_EXP = 2, ACC_LOG = 3, ACC_POW = 4, ACC_UNORM8_POW = 5, ACC_F32_TO_F16 = 6, ACC_F16_TO_F32 = 7 };

static double ulp_of(double v) {
  v = std::fabs(v);
  if (!(v >= 1.1754943508222875e-38)) return std::ldexp(1.0, -149);
  int e;
  std::frexp(v, &e);   // v = m 2^e, m in [0.5, 1)
  return std::ldexp(1.0, e - 1 - 23);
}
#if defined(__x86_64__)
__attribute__((target("f16c"))) static uint16_t hw_f32_to_f16(float f) { return (uint16_t)_cvtss_sh(f, _MM_FROUND_TO_NEAREST_INT); }
__attribute__((target("f16c"))) static float hw_f16_to_f32(uint16_t h) { return _cvtsh_ss(h); }
#endif

struct Acc {
  double max_err = 0.0, aux = 0.0;
  uint32_t arg = 0;
  bool any = false;
};

static void acc_range(int fn, uint64_t lo, uint64_t hi, Acc* out) {
  Acc a;
  for (uint64_t i = lo; i < hi; i++) {
    const uint32_t u = (uint32_t)i;
    const float x = rt_u2f(u);
    double err = 0.0;
    switch (fn) {
      case ACC_SIN: case ACC_COS: {
        float s, c;
        rt_sincos(x, &s, &c);
        err = fn == ACC_SIN ? std::fabs((double)s - std::sin((double)x)) : std::fabs((double)c - std::cos((double)x));
        break;
      }
      case ACC_EXP: {
        const double r = std::exp((double)x);
        const float f = rt_exp(x);
        // at the upper threshold itself exp(x) lies more than half an ulp above the largest f32: inf is the rounded answer
        err = (f == (float)r && std::isinf(f)) ? 0.0 : std::fabs((double)f - r) / ulp_of(r);
        break;
      }
      case ACC_LOG: { const double r = std::log((double)x); err = std::fabs((double)rt_log(x) - r) / ulp_of(r); break; }
      case ACC_POW: err = std::fabs((double)rt_pow(x, MATH_POW22_Y) - std::pow((double)x, (double)MATH_POW22_Y)); break;
      case ACC_UNORM8_POW: {
        const double want = std::floor(255.0 * std::pow((double)x, (double)MATH_POW22_Y) + 0.5);
        const double d = std::fabs((double)rt_unorm8(rt_pow(x, MATH_POW22_Y)) - want);
        if (d != 0.0) { if (a.max_err == 0.0) a.arg = u; a.max_err += 1.0; if (d > a.aux) a.aux = d; a.any = true; }
        continue;
      }
#if defined(__x86_64__)
      case ACC_F32_TO_F16: {
        const uint16_t got = rt_f32_to_f16(x), want = hw_f32_to_f16(x);
        const bool gn = (got & 0x7fffu) > 0x7c00u, wn = (want & 0x7fffu) > 0x7c00u;
        if (gn != wn || (!gn && got != want)) { if (a.max_err == 0.0) a.arg = u; a.max_err += 1.0; a.any = true; }
        continue;
      }
      case ACC_F16_TO_F32: {
        const float got = rt_f16_to_f32((uint16_t)u), want = hw_f16_to_f32((uint16_t)u);
        const bool gn = got != got, wn = want != want;
        if (gn != wn || (!gn && rt_f2u(got) != rt_f2u(want))) { if (a.max_err == 0.0) a.arg = u; a.max_err += 1.0; a.any = true; }
        continue;
      }
#endif
      default: break;
    }
    if (err != err) err = HUGE_VAL;   // a NaN on one side only (the sweeps stay inside the domains, where neither side has one)
    if (!a.any || err > a.max_err) { a.max_err = err; a.arg = u; a.any = true; }
  }
  *out = a;
}

extern "C" int math_ref_accuracy(int fn, uint64_t first, uint64_t count, int threads, double* out_max, uint32_t* out_arg, double* out_aux) {
  if (fn < 0 || fn > ACC_F16_TO_F32) return -1;
#if !defined(__x86_64__)
  if (fn >= ACC_F32_TO_F16) return -2;
#endif
  if (threads < 1) threads = 1;
  std::vector<Acc> part((size_t)threads);
  parallel(first, count, threads, [&](int t, uint64_t lo, uint64_t hi) { acc_range(fn, lo, hi, &part[(size_t)t]); });
  const bool counting = fn >= ACC_UNORM8_POW;
  Acc a;
  for (const Acc& p : part) {
    if (!p.any) continue;
    if (counting) {
      if (!a.any) a.arg = p.arg;
      a.max_err += p.max_err;
      if (p.aux > a.aux) a.aux = p.aux;
    } else if (!a.any || p.max_err > a.max_err) {
      a.max_err = p.max_err;
      a.arg = p.arg;
    }
    a.any = true;
  }
  if (out_max) *out_max = a.max_err;
  if (out_arg) *out_arg = a.arg;
  if (out_aux) *out_aux = a.aux;
  return 0;
}

#ifdef MATH_REF_MAIN
int main() {
  for (int op = 0; op < MATH_OP_COUNT; op++)
    std::printf("%s %016llx\n", k_names[op], (unsigned long long)math_ref_reduced_checksum(op, 4));
  return 0;
}
#endif
