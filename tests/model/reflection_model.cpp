// reflection_model.cpp — TEST INFRASTRUCTURE: the reference of reflection probes (rt_capture_reflection / rt_filter_reflection /
// rt_bake_reflection, mi355rt.h "THE REFLECTION RULE").
// This file includes the radiance model (and through it the oracle) as its translation unit - the result is that library plus
// the entry points below.  The CAPTURE is stated once on the model's own pieces, as the probe model states a gather: the
// jittered octahedral direction from the oracle's rng, intersect_tlas for every sample's first segment, surface_frame and
// bounce_loop behind it.  It does not call radiance_model_trace: that a capture is the composition of radiance queries on
// these directions is what tests/test_reflection_model.py checks.  The FILTER is stated on the two public headers alone
// (mi355rt_math.h, mi355rt_layout.h): the octahedral mapping, the frame and the lobe are written out here, not taken from the
// oracle.
// build: the flags of oracle/Makefile (tests/reflection_util.py does it)
#include "radiance_model.cpp"

namespace {

const uint32_t RF_DIR_STREAM = 0x80000000u;   // pad ^ this = the stream id of a texel's directions (the gathers')
const int RF_LANES = 64;

struct RfOnb {
  rt3 u, v, w;
};

rt3 rf_unpack(float px, float py) {
  rt3 n = rt3_make(px, py, 1.0f - rt_abs(px) - rt_abs(py));
  const float t = rt_saturate(-n.z);
  n.x += (n.x >= 0.0f) ? -t : t;
  n.y += (n.y >= 0.0f) ? -t : t;
  return rt_normalize(n);
}

rt2 rf_pack(rt3 v) {
  const float s = rt_rcp(rt_abs(v.x) + rt_abs(v.y) + rt_abs(v.z));
  const rt2 p = rt2_make(v.x * s, v.y * s);
  if (v.z < 0.0f)
    return rt2_make((1.0f - rt_abs(p.y)) * (p.x >= 0.0f ? 1.0f : -1.0f), (1.0f - rt_abs(p.x)) * (p.y >= 0.0f ? 1.0f : -1.0f));
  return p;
}

RfOnb rf_onb(rt3 n) {
  const float sign = (n.z >= 0.0f) ? 1.0f : -1.0f;
  const float a = -rt_rcp(sign + n.z);
  const float b = n.x * n.y * a;
  RfOnb o;
  o.u = rt3_make(1.0f + sign * n.x * n.x * a, sign * b, -sign * n.x);
  o.v = rt3_make(b, sign + n.y * n.y * a, -n.y);
  o.w = n;
  return o;
}

rt3 rf_to_world(const RfOnb& o, rt3 t) { return t.x * o.u + t.y * o.v + t.z * o.w; }

uint32_t rf_bitreverse32(uint32_t x) {
  uint32_t r = 0u;
  for (int b = 0; b < 32; b++) r |= ((x >> b) & 1u) << (31 - b);
  return r;
}

// l_t of (roughness a, sample s of K); the weight is its z
rt3 rf_lobe(float a, uint32_t s, uint32_t K) {
  const float ux = rt_div((float)s + 0.5f, (float)K);
  const float uy = (float)(rf_bitreverse32(s) >> 8) * 0x1p-24f;
  const float phi = RT_TWO_PI * ux;
  const float cos_theta = rt_sqrt(rt_max(0.0f, rt_div(1.0f - uy, 1.0f + (a * a - 1.0f) * uy)));
  const float sin_theta = rt_sqrt(rt_max(0.0f, 1.0f - cos_theta * cos_theta));
  float sp, cp;
  rt_sincos(phi, &sp, &cp);
  const rt3 h = rt3_make(sin_theta * cp, sin_theta * sp, cos_theta);
  return rt3_make(2.0f * (h.z * h.x), 2.0f * (h.z * h.y), 2.0f * (h.z * h.z) - 1.0f);
}

uint32_t rf_axis_index(float q, uint32_t size) {
  float u = (q * 0.5f + 0.5f) * (float)size;
  if (!(u > 0.0f)) u = 0.0f;
  const uint32_t i = rt_f2u32_sat(rt_floor(u));
  return i < size - 1u ? i : size - 1u;
}

float rf_tree(float* P) {   // the six butterfly steps on 64 partials; the sum is P[0]
  for (int m = 32; m >= 1; m >>= 1) {
    float Q[RF_LANES];
    for (int l = 0; l < RF_LANES; l++) Q[l] = P[l] + P[l ^ m];
    for (int l = 0; l < RF_LANES; l++) P[l] = Q[l];
  }
  return P[0];
}

rt3 rf_direction(uint32_t pad_t, uint32_t f, uint32_t i, uint32_t j, uint32_t size) {
  uint32_t rng_d = Oracle::init_rng(pad_t ^ RF_DIR_STREAM, f);
  const float jx = Oracle::rand_pcg(&rng_d);
  const float jy = Oracle::rand_pcg(&rng_d);
  const float px = rt_div((float)i + jx, (float)size) * 2.0f - 1.0f;
  const float py = rt_div((float)j + jy, (float)size) * 2.0f - 1.0f;
  return rf_unpack(px, py);
}

}  // namespace

extern "C" {

// out: n x size x size x spt x 3 f32: the direction of sample s of texel (i, j) of probe p
void reflection_model_directions(const rt_probe* probes, uint32_t n, uint32_t size, uint32_t spt, uint32_t seed, float* out) {
  for (uint32_t p = 0; p < n; p++)
    for (uint32_t t = 0; t < size * size; t++)
      for (uint32_t s = 0; s < spt; s++) {
        const rt3 d = rf_direction(probes[p].pad + t, seed * spt + s, t % size, t / size, size);
        float* w = out + (((size_t)p * size * size + t) * spt + s) * 3;
        w[0] = d.x;
        w[1] = d.y;
        w[2] = d.z;
      }
}

// out: n x size x size x 4 f32 {r, g, b, hit_fraction}.  counts: 5 u64 {extension_rays, shadow_rays, shaded_hits,
// nodes_visited, tris_tested}, the sums over the call (may be null).
void reflection_model_capture(oracle_ctx* ctx, const rt_reflection_desc* D, const rt_probe* probes, uint32_t n, uint32_t max_depth,
                              uint32_t seed, float* out, uint64_t* counts) {
  const Oracle& o = ctx->o;
  const uint32_t size = D->size, spt = D->spt;
  Counters cn;
  for (uint32_t p = 0; p < n; p++) {
    const rt_probe& q = probes[p];
    const rt3 origin = rt3_make(q.position[0], q.position[1], q.position[2]);
    for (uint32_t t = 0; t < size * size; t++) {
      const uint32_t pad_t = q.pad + t;
      rt3 col = rt3_splat(0.0f);
      uint32_t hits = 0u;
      for (uint32_t s = 0; s < spt; s++) {
        const uint32_t f = seed * spt + s;
        const Ray ray = make_ray(origin, rf_direction(pad_t, f, t % size, t / size, size));
        rt3 sample = rt3_splat(0.0f);
        cn.extension_rays++;
        HitResult hit = o.intersect_tlas(ray, T_MIN, q.t_max, cn);
        if (hit.t < q.t_max) hits++;   // a miss hands the bound back
        if (hit.inst_idx >= 0 && max_depth != 0u) {
          uint32_t rng = Oracle::init_rng(pad_t, f);
          Surface sf;
          surface_frame(o, ray, rt_f2u32_sat(hit.tri_idx), hit.inst_idx, hit.t, nullptr, nullptr, sf);
          sample = sample + bounce_loop(o, ray, &rng, sf, max_depth, cn);   // a radiance query's 0 + r at spp = 1
        }
        col = col + sample;
      }
      if (spt != 1u) col = col / (float)spt;
      float* w = out + ((size_t)p * size * size + t) * 4;
      w[0] = col.x;
      w[1] = col.y;
      w[2] = col.z;
      w[3] = rt_div((float)hits, (float)spt);
    }
  }
  if (counts) {
    counts[0] = cn.extension_rays;
    counts[1] = cn.shadow_rays;
    counts[2] = cn.shaded_hits;
    counts[3] = cn.nodes_visited;
    counts[4] = cn.tris_tested;
  }
}

// maps: n x size x size x 4 f32; chains: n x chain_texels x 4 f32.  No scene.
void reflection_model_filter(const rt_reflection_desc* D, const float* maps, uint32_t n, float* chains) {
  const uint32_t size = D->size, K = D->filter_samples;
  size_t chain = 0;
  for (uint32_t m = 0; m < D->levels; m++) chain += (size_t)(size >> m) * (size >> m);
  for (uint32_t p = 0; p < n; p++) {
    const float* src = maps + (size_t)p * size * size * 4;
    float* dst = chains + (size_t)p * chain * 4;
    for (size_t k = 0; k < (size_t)size * size * 4; k++) dst[k] = src[k];   // level 0, word for word (callers compare bits)
    size_t off = (size_t)size * size;
    for (uint32_t m = 1; m < D->levels; m++) {
      const uint32_t S = size >> m;
      const float a = rt_div((float)m, (float)(D->levels - 1u));
      for (uint32_t j = 0; j < S; j++)
        for (uint32_t i = 0; i < S; i++) {
          const float cx = rt_div((float)i + 0.5f, (float)S) * 2.0f - 1.0f;
          const float cy = rt_div((float)j + 0.5f, (float)S) * 2.0f - 1.0f;
          const RfOnb onb = rf_onb(rf_unpack(cx, cy));
          float P[5][RF_LANES];
          for (int c = 0; c < 5; c++)
            for (int l = 0; l < RF_LANES; l++) P[c][l] = 0.0f;
          for (uint32_t s = 0; s < K; s++) {
            const rt3 lt = rf_lobe(a, s, K);
            const float w = lt.z;
            float term[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (w > 0.0f) {
              const rt2 q = rf_pack(rf_to_world(onb, lt));
              const float* texel = src + ((size_t)rf_axis_index(q.y, size) * size + rf_axis_index(q.x, size)) * 4;
              for (int c = 0; c < 4; c++) term[c] = w * texel[c];
              term[4] = w;
            }
            for (int c = 0; c < 5; c++) P[c][s % RF_LANES] = P[c][s % RF_LANES] + term[c];
          }
          float sum[5];
          for (int c = 0; c < 5; c++) sum[c] = rf_tree(P[c]);
          float* w4 = dst + (off + (size_t)j * S + i) * 4;
          for (int c = 0; c < 4; c++) w4[c] = sum[4] > 0.0f ? rt_div(sum[c], sum[4]) : 0.0f;
        }
      off += (size_t)S * S;
    }
  }
}

// the lobe of one level: l_t (K x 3 f32) and sum_w (1 f32) as the filter forms them
void reflection_model_lobe(uint32_t level, uint32_t levels, uint32_t K, float* lt_out, float* sum_w) {
  const float a = rt_div((float)level, (float)(levels - 1u));
  float P[RF_LANES];
  for (int l = 0; l < RF_LANES; l++) P[l] = 0.0f;
  for (uint32_t s = 0; s < K; s++) {
    const rt3 lt = rf_lobe(a, s, K);
    lt_out[3 * s + 0] = lt.x;
    lt_out[3 * s + 1] = lt.y;
    lt_out[3 * s + 2] = lt.z;
    P[s % RF_LANES] = P[s % RF_LANES] + (lt.z > 0.0f ? lt.z : 0.0f);
  }
  *sum_w = rf_tree(P);
}

// texel-centre directions of a size x size map: size x size x 3 f32
void reflection_model_centres(uint32_t size, float* out) {
  for (uint32_t j = 0; j < size; j++)
    for (uint32_t i = 0; i < size; i++) {
      const rt3 n = rf_unpack(rt_div((float)i + 0.5f, (float)size) * 2.0f - 1.0f, rt_div((float)j + 0.5f, (float)size) * 2.0f - 1.0f);
      float* w = out + ((size_t)j * size + i) * 3;
      w[0] = n.x;
      w[1] = n.y;
      w[2] = n.z;
    }
}

}  // extern "C"
