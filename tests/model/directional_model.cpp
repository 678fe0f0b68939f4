// directional_model.cpp — TEST INFRASTRUCTURE: the reference of the directional gathers (rt_gather_directional, mi355rt.h).
// This file includes the radiance model (and through it the oracle) as its translation unit - the result is that library
// plus two entry points - and states the directional gather ONCE on the model's own pieces: the uniform-sphere direction from
// the oracle's rng mirrored into the hemisphere of the point's normal, intersect_tlas for every sample's first segment,
// surface_frame and bounce_loop behind it, the band 0 .. 1 basis and the fixed summation tree in the arithmetic of
// mi355rt_math.h.  It does not call radiance_model_trace: that a directional gather is the composition of radiance queries on
// these directions (and on the pad' rays at seed 0) is what tests/test_directional_model.py checks.
// build: the flags of oracle/Makefile (tests/directional_util.py does it)
#include "radiance_model.cpp"

namespace {

const uint32_t DIR_STREAM = 0x80000000u;   // pad ^ this = the stream id of a point's directions (the gather's)
const int SH = 4, WORDS = 12, LANES = 64;

// direction of sample f of a point with normal n (as given): uniform on the sphere from the direction stream, its sign
// flipped where the f32 dot with n is < 0; not normalised again
rt3 directional_direction(uint32_t pad, uint32_t f, const float* n) {
  uint32_t rng_d = Oracle::init_rng(pad ^ DIR_STREAM, f);
  const float u1 = Oracle::rand_pcg(&rng_d);
  const float u2 = Oracle::rand_pcg(&rng_d);
  const float z = 1.0f - 2.0f * u1;
  const float r = rt_sqrt(rt_max(0.0f, 1.0f - z * z));
  float sp, cp;
  rt_sincos(RT_TWO_PI * u2, &sp, &cp);
  const rt3 d0 = rt3_make(r * cp, r * sp, z);
  const float c = (d0.x * n[0] + d0.y * n[1]) + d0.z * n[2];
  return (c < 0.0f) ? rt3_make(-d0.x, -d0.y, -d0.z) : d0;
}

}  // namespace

extern "C" {

// points: n x rt_gather_point.  out: n x spp x 3 f32, the direction of sample s of point i at (i * spp + s) * 3.
void directional_model_directions(const rt_gather_point* points, uint32_t n, uint32_t spp, uint32_t seed, float* out) {
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t s = 0u; s < spp; s++) {
      const rt3 d = directional_direction(points[i].pad, seed * spp + s, points[i].normal);
      float* w = out + ((size_t)i * spp + s) * 3;
      w[0] = d.x;
      w[1] = d.y;
      w[2] = d.z;
    }
}

// out: n x 16 f32, rt_directional: row k {sh[k].rgb, hit_fraction}.  hits: n x u32, the samples whose first segment hit (may
// be null).  counts: n x 5 u64 {extension_rays, shadow_rays, shaded_hits, nodes_visited, tris_tested} of each point (may be
// null).
void directional_model_gather(oracle_ctx* ctx, const rt_gather_point* points, uint32_t n, uint32_t max_depth, uint32_t spp,
                              uint32_t seed, float* out, uint32_t* hits_out, uint64_t* counts) {
  const Oracle& o = ctx->o;
  for (uint32_t i = 0; i < n; i++) {
    const rt_gather_point& q = points[i];
    const rt3 origin = rt3_make(q.position[0], q.position[1], q.position[2]);
    Counters cn;
    float P[LANES][WORDS];
    for (int l = 0; l < LANES; l++)
      for (int j = 0; j < WORDS; j++) P[l][j] = 0.0f;
    uint32_t hits = 0u;
    for (uint32_t s = 0u; s < spp; s++) {
      const uint32_t f = seed * spp + s;
      const rt3 d = directional_direction(q.pad, f, q.normal);
      const Ray ray = make_ray(origin, d);
      rt3 sample = rt3_splat(0.0f);
      // the first segment: one extension ray of every sample
      cn.extension_rays++;
      HitResult hit = o.intersect_tlas(ray, T_MIN, q.t_max, cn);
      if (hit.t < q.t_max) hits++;   // a miss hands the bound back
      if (hit.inst_idx >= 0 && max_depth != 0u) {
        uint32_t rng = Oracle::init_rng(q.pad, f);
        Surface sf;
        surface_frame(o, ray, rt_f2u32_sat(hit.tri_idx), hit.inst_idx, hit.t, nullptr, nullptr, sf);
        sample = sample + bounce_loop(o, ray, &rng, sf, max_depth, cn);   // a radiance query's 0 + r at spp = 1
      }
      const float Y[SH] = {0.282094792f, 0.488602512f * d.y, 0.488602512f * d.z, 0.488602512f * d.x};
      float* p = P[s % LANES];
      for (int k = 0; k < SH; k++) {
        p[3 * k + 0] = p[3 * k + 0] + sample.x * Y[k];
        p[3 * k + 1] = p[3 * k + 1] + sample.y * Y[k];
        p[3 * k + 2] = p[3 * k + 2] + sample.z * Y[k];
      }
    }
    for (int m = 32; m >= 1; m >>= 1) {
      float Q[LANES][WORDS];
      for (int l = 0; l < LANES; l++)
        for (int j = 0; j < WORDS; j++) Q[l][j] = P[l][j] + P[l ^ m][j];
      for (int l = 0; l < LANES; l++)
        for (int j = 0; j < WORDS; j++) P[l][j] = Q[l][j];
    }
    float* w = out + (size_t)i * 16;
    const float hf = rt_div((float)hits, (float)spp);
    for (int k = 0; k < SH; k++) {
      for (int c = 0; c < 3; c++) w[4 * k + c] = rt_div(P[0][3 * k + c], (float)spp) * RT_TWO_PI;
      w[4 * k + 3] = hf;
    }
    if (hits_out) hits_out[i] = hits;
    if (counts) {
      uint64_t* k = counts + (size_t)i * 5;
      k[0] = cn.extension_rays;
      k[1] = cn.shadow_rays;
      k[2] = cn.shaded_hits;
      k[3] = cn.nodes_visited;
      k[4] = cn.tris_tested;
    }
  }
}

}  // extern "C"
