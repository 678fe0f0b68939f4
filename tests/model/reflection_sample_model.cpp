// reflection_sample_model.cpp — TEST INFRASTRUCTURE: the reference of the reflection sampler (mi355rt.h "THE REFLECTION SAMPLE
// RULE").  A stand-alone restatement of the rule in plain scalar C++ on mi355rt_math.h and mi355rt_layout.h alone: one query at
// a time, one block per sentence of the rule, a tap of weight zero really left out and a level of weight zero really not
// read.  Nothing is shared with csrc/k_reflection_sample.hip.h or with the other models.  Beside the sampler it exports the
// parts the tests look at on their own: the corrected direction, the fold and the taps of one level - and a clamp-to-edge
// form of the fetch, which is NOT the rule: tests/test_reflection_sample_model.py shows on it what the fold is for.
// build: the flags of oracle/Makefile, -I include (tests/reflection_sample_util.py does it)
#include <cstddef>
#include <cstdint>

#include "mi355rt_layout.h"
#include "mi355rt_math.h"

namespace {

const float kInf = __builtin_inff();

rt2 pack(rt3 v) {
  const float s = rt_rcp(rt_abs(v.x) + rt_abs(v.y) + rt_abs(v.z));
  const rt2 p = rt2_make(v.x * s, v.y * s);
  if (v.z < 0.0f)
    return rt2_make((1.0f - rt_abs(p.y)) * (p.x >= 0.0f ? 1.0f : -1.0f), (1.0f - rt_abs(p.x)) * (p.y >= 0.0f ? 1.0f : -1.0f));
  return p;
}

// direction and parallax
rt3 corrected(const rt_reflection_sample_desc& D, const rt_probe* probes, const rt_reflection_box* boxes,
              const rt_reflection_query& Q) {
  const rt3 d = rt3_make(Q.direction[0], Q.direction[1], Q.direction[2]);
  if (!(D.flags & RT_REFLECTION_SAMPLE_PARALLAX)) return d;
  const float* x = Q.position;
  const float* c = probes[Q.probe].position;
  const rt_reflection_box& B = boxes[Q.probe];
  const float dv[3] = {d.x, d.y, d.z};
  bool inside = true;
  for (int a = 0; a < 3; a++) inside = inside && (B.lo[a] <= x[a] && x[a] <= B.hi[a]);
  if (!inside) return d;
  float ta[3];
  for (int a = 0; a < 3; a++) {
    if (dv[a] > 0.0f)
      ta[a] = rt_div(B.hi[a] - x[a], dv[a]);
    else if (dv[a] < 0.0f)
      ta[a] = rt_div(B.lo[a] - x[a], dv[a]);
    else
      ta[a] = kInf;
  }
  const float t = rt_min(rt_min(ta[0], ta[1]), ta[2]);
  if (!(t < kInf)) return d;
  float out[3];
  for (int a = 0; a < 3; a++) {
    const float step = dv[a] * t;
    const float h = x[a] + step;
    out[a] = h - c[a];
  }
  return rt3_make(out[0], out[1], out[2]);
}

// fold: x first, then y
uint32_t fold(int i, int j, int S) {
  if (i < 0 || i >= S) {
    i = (i < 0) ? -1 - i : 2 * S - 1 - i;
    j = S - 1 - j;
  }
  if (j < 0 || j >= S) {
    j = (j < 0) ? -1 - j : 2 * S - 1 - j;
    i = S - 1 - i;
  }
  return (uint32_t)(j * S + i);
}
// what a sampler without the fold would do: the tap outside is the nearest one inside
uint32_t clamp_to_edge(int i, int j, int S) {
  i = i < 0 ? 0 : (i >= S ? S - 1 : i);
  j = j < 0 ? 0 : (j >= S ? S - 1 : j);
  return (uint32_t)(j * S + i);
}

struct Axis {
  int i0;
  float f;
};
Axis axis(float q, uint32_t S) {
  float u = (q * 0.5f + 0.5f) * (float)S - 0.5f;
  if (!(u >= -0.5f)) u = -0.5f;
  u = rt_min(u, (float)S - 0.5f);
  const float fl = rt_floor(u);
  Axis a;
  a.i0 = (int)fl;
  a.f = u - fl;
  return a;
}

struct Taps {
  uint32_t t[4];   // t00, t10, t01, t11
  float w[4];
};
Taps taps(rt2 q, uint32_t S, bool clamp) {
  const Axis ax = axis(q.x, S), ay = axis(q.y, S);
  const float wx[2] = {1.0f - ax.f, ax.f}, wy[2] = {1.0f - ay.f, ay.f};
  Taps T;
  for (int b = 0; b < 2; b++)
    for (int a = 0; a < 2; a++) {
      T.t[2 * b + a] = clamp ? clamp_to_edge(ax.i0 + a, ay.i0 + b, (int)S) : fold(ax.i0 + a, ay.i0 + b, (int)S);
      T.w[2 * b + a] = wx[a] * wy[b];
    }
  return T;
}

// fetch: level: S * S texels of four floats
void fetch(const float* level, uint32_t S, rt2 q, bool clamp, float value[4]) {
  const Taps T = taps(q, S, clamp);
  for (int ch = 0; ch < 4; ch++) {
    float acc = 0.0f;
    for (int k = 0; k < 4; k++) {
      if (T.w[k] == 0.0f) continue;
      const float term = T.w[k] * level[4 * (size_t)T.t[k] + ch];
      acc = acc + term;
    }
    value[ch] = acc;
  }
}

void sample(const rt_reflection_sample_desc& D, const float* chains, uint32_t n_probes, const rt_probe* probes,
            const rt_reflection_box* boxes, const rt_reflection_query& Q, bool clamp, float out[4]) {
  // probe
  for (int ch = 0; ch < 4; ch++) out[ch] = 0.0f;
  if (Q.probe >= n_probes) return;
  const rt3 d = corrected(D, probes, boxes, Q);
  // level
  float r = Q.roughness;
  if (!(r > 0.0f)) r = 0.0f;
  r = rt_min(r, 1.0f);
  const float xl = r * (float)(D.levels - 1u);
  uint32_t m0 = (uint32_t)xl;
  if (m0 > D.levels - 2u) m0 = D.levels - 2u;
  const uint32_t m1 = m0 + 1u;
  const float g = xl - (float)m0;
  const float weight[2] = {1.0f - g, g};
  const uint32_t level[2] = {m0, m1};
  // the chain
  size_t chain_texels = 0;
  for (uint32_t m = 0; m < D.levels; m++) chain_texels += (size_t)(D.size >> m) * (D.size >> m);
  const float* chain = chains + 4 * chain_texels * Q.probe;
  const rt2 q = pack(d);
  // fetch and mix
  for (int k = 0; k < 2; k++) {
    if (weight[k] == 0.0f) continue;
    size_t offset = 0;
    for (uint32_t m = 0; m < level[k]; m++) offset += (size_t)(D.size >> m) * (D.size >> m);
    float v[4];
    fetch(chain + 4 * offset, D.size >> level[k], q, clamp, v);
    for (int ch = 0; ch < 4; ch++) {
      const float term = weight[k] * v[ch];
      out[ch] = out[ch] + term;
    }
  }
}

}  // namespace

extern "C" {

// n queries -> n results of four floats; clamp != 0: the clamp-to-edge form, not the rule
void reflection_sample_model(const rt_reflection_sample_desc* D, const float* chains, uint32_t n_probes, const rt_probe* probes,
                             const rt_reflection_box* boxes, const rt_reflection_query* queries, uint32_t n, int clamp, float* out) {
  for (uint32_t i = 0; i < n; i++) sample(*D, chains, n_probes, probes, boxes, queries[i], clamp != 0, out + 4 * (size_t)i);
}

// n queries (every probe index below the length of probes and boxes) -> n corrected directions of three floats
void reflection_sample_model_direction(const rt_reflection_sample_desc* D, const rt_probe* probes, const rt_reflection_box* boxes,
                                       const rt_reflection_query* queries, uint32_t n, float* out) {
  for (uint32_t i = 0; i < n; i++) {
    const rt3 d = corrected(*D, probes, boxes, queries[i]);
    out[3 * (size_t)i] = d.x;
    out[3 * (size_t)i + 1] = d.y;
    out[3 * (size_t)i + 2] = d.z;
  }
}

uint32_t reflection_sample_model_fold(uint32_t S, int i, int j) { return fold(i, j, (int)S); }

// n directions of three floats -> the four texel indices j * S + i and the four weights of a level of side S, in the order
// t00, t10, t01, t11
void reflection_sample_model_taps(uint32_t S, const float* dirs, uint32_t n, uint32_t* index, float* weight) {
  for (uint32_t i = 0; i < n; i++) {
    const Taps T = taps(pack(rt3_make(dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2])), S, false);
    for (int k = 0; k < 4; k++) {
      index[4 * (size_t)i + k] = T.t[k];
      weight[4 * (size_t)i + k] = T.w[k];
    }
  }
}

}  // extern "C"
