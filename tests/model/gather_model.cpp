// gather_model.cpp — TEST INFRASTRUCTURE: the reference of the irradiance gathers (rt_gather_irradiance, mi355rt.h).
// This file includes the radiance model (and through it the oracle) as its translation unit - the result is that library
// plus two entry points - and states the gather ONCE on the model's own pieces: the oracle's Lambert sampler for the
// direction, intersect_tlas for every sample's first segment, surface_frame and bounce_loop behind it, and the arithmetic
// of mi355rt_math.h for the mean.  It does not call radiance_model_trace: that a gather is the composition of radiance
// queries on these directions is what tests/test_gather_model.py checks.
// build: the flags of oracle/Makefile (tests/gather_util.py does it)
#include "radiance_model.cpp"

namespace {

const uint32_t DIR_STREAM = 0x80000000u;   // pad ^ this = the stream id of a point's directions

// direction of sample f of a point: the .dir of sample_diffuse on the normalised normal, from the direction stream
rt3 gather_direction(const rt_gather_point& q, uint32_t f) {
  const rt3 n = rt_normalize(rt3_make(q.normal[0], q.normal[1], q.normal[2]));
  uint32_t rng_d = Oracle::init_rng(q.pad ^ DIR_STREAM, f);
  return Oracle::sample_diffuse(n, rt3_splat(0.0f), &rng_d).dir;
}

}  // namespace

extern "C" {

// points: n x rt_gather_point.  out: n x spp x 3 f32, the direction of sample s of point i at (i * spp + s) * 3.
void gather_model_directions(const rt_gather_point* points, uint32_t n, uint32_t spp, uint32_t seed, float* out) {
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t s = 0u; s < spp; s++) {
      const rt3 d = gather_direction(points[i], seed * spp + s);
      float* w = out + ((size_t)i * spp + s) * 3;
      w[0] = d.x;
      w[1] = d.y;
      w[2] = d.z;
    }
}

// out: n x 4 f32 {r, g, b, hit_fraction}.  hits: n x u32, the samples whose first segment hit (may be null).  counts: n x 5
// u64 {extension_rays, shadow_rays, shaded_hits, nodes_visited, tris_tested} of each point (may be null).
void gather_model_gather(oracle_ctx* ctx, const rt_gather_point* points, uint32_t n, uint32_t max_depth, uint32_t spp,
                         uint32_t seed, float* out, uint32_t* hits_out, uint64_t* counts) {
  const Oracle& o = ctx->o;
  for (uint32_t i = 0; i < n; i++) {
    const rt_gather_point& q = points[i];
    const rt3 origin = rt3_make(q.position[0], q.position[1], q.position[2]);
    Counters cn;
    rt3 col = rt3_splat(0.0f);
    uint32_t hits = 0u;
    for (uint32_t s = 0u; s < spp; s++) {
      const uint32_t f = seed * spp + s;
      const Ray ray = make_ray(origin, gather_direction(q, f));
      rt3 sample = rt3_splat(0.0f);
      // the first segment: one extension ray of every sample
      cn.extension_rays++;
      HitResult hit = o.intersect_tlas(ray, T_MIN, q.t_max, cn);
      if (hit.inst_idx >= 0) {
        hits++;
        if (max_depth != 0u) {
          uint32_t rng = Oracle::init_rng(q.pad, f);
          Surface sf;
          surface_frame(o, ray, rt_f2u32_sat(hit.tri_idx), hit.inst_idx, hit.t, nullptr, nullptr, sf);
          sample = sample + bounce_loop(o, ray, &rng, sf, max_depth, cn);   // a radiance query's 0 + r at spp = 1
        }
      }
      col = col + sample;
    }
    if (spp != 1u) col = col / (float)spp;
    float* w = out + (size_t)i * 4;
    w[0] = col.x;
    w[1] = col.y;
    w[2] = col.z;
    w[3] = rt_div((float)hits, (float)spp);
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
