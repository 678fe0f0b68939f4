// volume_visibility_model.cpp — TEST INFRASTRUCTURE: the reference of probe visibility maps (mi355rt.h "THE VISIBILITY RULE").
// A stand-alone restatement of the rule's parts - the rays of a capture, the reduction of their hits, the wrap, the fetch, the
// sample and the tiled export - in plain scalar C++ on mi355rt_math.h and mi355rt_layout.h alone: one point at a time, one
// loop per sentence of the rule, nothing shared with csrc/k_volume_visibility.hip.h or with tests/model/volume_model.cpp (that
// the two samplers agree where every probe is visible is what tests/test_volume_visibility_model.py checks).  The trace
// between rays and reduction is the ray query's, whose reference is the oracle.
// build: the flags of oracle/Makefile, -I include (tests/volume_visibility_util.py does it)
#include <cstddef>
#include <cstdint>

#include "mi355rt_layout.h"
#include "mi355rt_math.h"

namespace {

uint32_t probe_count(const rt_volume_desc& D) { return D.nx * D.ny * D.nz; }

// the renderer's random numbers (a PCG hash), restated
uint32_t vv_init_rng(uint32_t id, uint32_t frame) {
  uint32_t s = id + frame * 719393u;
  s ^= 2747636419u;
  s *= 2654435769u;
  s ^= s >> 16;
  s *= 2654435769u;
  s ^= s >> 16;
  s *= 2654435769u;
  return s;
}
float vv_rand(uint32_t* state) {
  const uint32_t old = *state;
  *state = old * 747796405u + 2891336453u;
  const uint32_t word = (*state >> ((old >> 28) + 4u)) ^ *state;
  return (float)((word >> 22) ^ word) * 2.3283064365386962890625e-10f;
}

rt3 vv_unpack(float px, float py) {
  rt3 n = rt3_make(px, py, 1.0f - rt_abs(px) - rt_abs(py));
  const float t = rt_saturate(-n.z);
  n.x += (n.x >= 0.0f) ? -t : t;
  n.y += (n.y >= 0.0f) ? -t : t;
  return rt_normalize(n);
}

rt2 vv_pack(rt3 v) {
  const float s = rt_rcp(rt_abs(v.x) + rt_abs(v.y) + rt_abs(v.z));
  const rt2 p = rt2_make(v.x * s, v.y * s);
  if (v.z < 0.0f)
    return rt2_make((1.0f - rt_abs(p.y)) * (p.x >= 0.0f ? 1.0f : -1.0f), (1.0f - rt_abs(p.x)) * (p.y >= 0.0f ? 1.0f : -1.0f));
  return p;
}

rt3 probe_position(const rt_volume_desc& D, uint32_t x, uint32_t y, uint32_t z) {
  const float fx = (float)x * D.step[0], fy = (float)y * D.step[1], fz = (float)z * D.step[2];
  return rt3_make(D.origin[0] + fx, D.origin[1] + fy, D.origin[2] + fz);
}

// the wrap: x first, then y; *wrapped is set when the tap was outside
uint32_t wrap(int i, int j, int size, int* wrapped) {
  if (i < 0 || i >= size || j < 0 || j >= size) *wrapped = 1;
  if (i < 0) {
    i = -1 - i;
    j = size - 1 - j;
  } else if (i >= size) {
    i = 2 * size - 1 - i;
    j = size - 1 - j;
  }
  if (j < 0) {
    j = -1 - j;
    i = size - 1 - i;
  } else if (j >= size) {
    j = 2 * size - 1 - j;
    i = size - 1 - i;
  }
  return (uint32_t)(j * size + i);
}

struct Tap {
  int i0;
  float f;
};
Tap axis(float q, uint32_t size) {
  const float u = (q * 0.5f + 0.5f) * (float)size - 0.5f;
  float fl = rt_floor(u);
  if (!(fl >= -1.0f)) fl = -1.0f;
  fl = rt_min(fl, (float)(size - 1u));
  Tap t;
  t.i0 = (int)fl;
  t.f = u - fl;
  return t;
}

// map: size * size texels of two floats; m: the two fetched words; -> whether a tap was wrapped
int fetch(const float* map, uint32_t size, rt3 v, float m[2]) {
  const rt2 q = vv_pack(v);
  const Tap tx = axis(q.x, size), ty = axis(q.y, size);
  int wrapped = 0;
  const float* t00 = map + 2 * (size_t)wrap(tx.i0, ty.i0, (int)size, &wrapped);
  const float* t10 = map + 2 * (size_t)wrap(tx.i0 + 1, ty.i0, (int)size, &wrapped);
  const float* t01 = map + 2 * (size_t)wrap(tx.i0, ty.i0 + 1, (int)size, &wrapped);
  const float* t11 = map + 2 * (size_t)wrap(tx.i0 + 1, ty.i0 + 1, (int)size, &wrapped);
  for (int k = 0; k < 2; k++) {
    const float a = t00[k] + tx.f * (t10[k] - t00[k]);
    const float b = t01[k] + tx.f * (t11[k] - t01[k]);
    m[k] = a + ty.f * (b - a);
  }
  return wrapped;
}

struct Axis {
  uint32_t i[2];
  float w[2];
};
Axis cell(float position, float origin, float step, uint32_t N) {
  float g = rt_div(position - origin, step);
  if (!(g > 0.0f)) g = 0.0f;
  g = rt_min(g, (float)(N - 1u));
  uint32_t i0 = (uint32_t)g;
  if (N > 1u && i0 > N - 2u) i0 = N - 2u;
  Axis a;
  a.i[0] = i0;
  a.i[1] = N == 1u ? i0 : i0 + 1u;
  const float f = N == 1u ? 0.0f : g - (float)i0;
  a.w[0] = 1.0f - f;
  a.w[1] = f;
  return a;
}

float visibility(const rt_volume_visibility_desc& V, const float* map, rt3 P, rt3 position, rt3 n) {
  const rt3 B = position + n * V.normal_bias;
  const rt3 e = B - P;
  const float len = rt_sqrt(rt_dot(e, e));
  float vis = 1.0f;
  if (len > 0.0f) {
    float m[2];
    fetch(map, V.size, e * rt_rcp(len), m);
    if (!(len <= m[0])) {
      const float var = rt_abs(m[0] * m[0] - m[1]);
      const float g = len - m[0];
      float c = rt_div(var, var + g * g);
      if (!(c > 0.0f)) c = 0.0f;
      c = (c * c) * c;
      vis = rt_max(c, V.min_visibility);
    }
  }
  if (V.flags & RT_VOLUME_VIS_BACKFACE) {
    const rt3 h = rt_normalize(P - position);
    const float b = (rt_dot(h, n) + 1.0f) * 0.5f;
    vis = vis * (b * b + 0.2f);
  }
  if (V.crush_threshold > 0.0f && vis < V.crush_threshold) vis = rt_div((vis * vis) * vis, V.crush_threshold * V.crush_threshold);
  return vis;
}

}  // namespace

extern "C" {

// rays: nx * ny * nz * size * size * spt rt_ray in (probe, texel, sample) order, written
void vvis_model_rays(const rt_volume_desc* desc, const rt_volume_visibility_desc* vis, uint32_t seed, rt_ray* rays) {
  const rt_volume_desc& D = *desc;
  const uint32_t size = vis->size, spt = vis->spt;
  for (uint32_t z = 0; z < D.nz; z++)
    for (uint32_t y = 0; y < D.ny; y++)
      for (uint32_t x = 0; x < D.nx; x++) {
        const uint32_t p = (z * D.ny + y) * D.nx + x;
        const rt3 P = probe_position(D, x, y, z);
        for (uint32_t t = 0; t < size * size; t++)
          for (uint32_t s = 0; s < spt; s++) {
            const uint32_t f = seed * spt + s;
            const uint32_t pad_t = D.pad_first + p * size * size + t;
            uint32_t rng_d = vv_init_rng(pad_t ^ 0x80000000u, f);
            const float jx = vv_rand(&rng_d);
            const float jy = vv_rand(&rng_d);
            const float px = rt_div((float)(t % size) + jx, (float)size) * 2.0f - 1.0f;
            const float py = rt_div((float)(t / size) + jy, (float)size) * 2.0f - 1.0f;
            const rt3 d = vv_unpack(px, py);
            rt_ray& r = rays[((size_t)p * size * size + t) * spt + s];
            r.origin[0] = P.x;
            r.origin[1] = P.y;
            r.origin[2] = P.z;
            r.t_max = vis->max_distance;
            r.dir[0] = d.x;
            r.dir[1] = d.y;
            r.dir[2] = d.z;
            r.pad = pad_t;
          }
      }
}

// hits: n_texels * spt rt_ray_hit in (texel, sample) order; out: n_texels texels of two floats
void vvis_model_texels(const rt_volume_visibility_desc* vis, const rt_ray_hit* hits, uint32_t n_texels, float* out) {
  const uint32_t spt = vis->spt;
  for (uint32_t t = 0; t < n_texels; t++) {
    float m1 = 0.0f, m2 = 0.0f;
    for (uint32_t s = 0; s < spt; s++) {
      const float x = rt_min(hits[(size_t)t * spt + s].t, vis->max_distance);
      m1 = m1 + x;
      m2 = m2 + x * x;
    }
    if (spt != 1u) {
      m1 = rt_div(m1, (float)spt);
      m2 = rt_div(m2, (float)spt);
    }
    out[2 * (size_t)t] = m1;
    out[2 * (size_t)t + 1] = m2;
  }
}

// the wrapped texel index of tap (i, j), i and j in -1 .. size
uint32_t vvis_model_wrap(uint32_t size, int i, int j) {
  int wrapped = 0;
  return wrap(i, j, (int)size, &wrapped);
}

// dirs: n x 3 f32; out: n x 2 f32; wrapped: n bytes, 1 where one of the four taps was outside the map
void vvis_model_fetch(uint32_t size, const float* map, const float* dirs, uint32_t n, float* out, uint8_t* wrapped) {
  for (uint32_t i = 0; i < n; i++)
    wrapped[i] = (uint8_t)fetch(map, size, rt3_make(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]), out + 2 * (size_t)i);
}

// the eight weights vis_c of each point, before the product with the trilinear weight; out: n x 8 f32
void vvis_model_weights(const rt_volume_desc* desc, const rt_volume_visibility_desc* vis, const float* maps,
                        const rt_gather_point* points, uint32_t n, float* out) {
  const rt_volume_desc& D = *desc;
  const size_t map_floats = 2 * (size_t)vis->size * vis->size;
  for (uint32_t i = 0; i < n; i++) {
    const rt_gather_point& pt = points[i];
    const Axis ax = cell(pt.position[0], D.origin[0], D.step[0], D.nx);
    const Axis ay = cell(pt.position[1], D.origin[1], D.step[1], D.ny);
    const Axis az = cell(pt.position[2], D.origin[2], D.step[2], D.nz);
    const rt3 position = rt3_make(pt.position[0], pt.position[1], pt.position[2]);
    const rt3 nrm = rt_normalize(rt3_make(pt.normal[0], pt.normal[1], pt.normal[2]));
    for (int c = 0; c < 8; c++) {
      const uint32_t x = ax.i[c & 1], y = ay.i[(c >> 1) & 1], z = az.i[c >> 2];
      const size_t p = (size_t)(z * D.ny + y) * D.nx + x;
      out[8 * (size_t)i + c] = visibility(*vis, maps + p * map_floats, probe_position(D, x, y, z), position, nrm);
    }
  }
}

// points: n rt_gather_point; out: n rt_irradiance
void vvis_model_sample(const rt_volume_desc* desc, const rt_volume_visibility_desc* vis, const rt_probe_sh9* volume,
                       const float* maps, const rt_gather_point* points, uint32_t n, rt_irradiance* out) {
  const rt_volume_desc& D = *desc;
  const size_t map_floats = 2 * (size_t)vis->size * vis->size;
  for (uint32_t i = 0; i < n; i++) {
    const rt_gather_point& pt = points[i];
    const Axis ax = cell(pt.position[0], D.origin[0], D.step[0], D.nx);
    const Axis ay = cell(pt.position[1], D.origin[1], D.step[1], D.ny);
    const Axis az = cell(pt.position[2], D.origin[2], D.step[2], D.nz);
    const rt3 position = rt3_make(pt.position[0], pt.position[1], pt.position[2]);
    const rt3 nrm = rt_normalize(rt3_make(pt.normal[0], pt.normal[1], pt.normal[2]));
    const rt_probe_sh9* corner[8];
    float w[8];
    float W = 0.0f;
    for (int c = 0; c < 8; c++) {
      const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
      const size_t p = (size_t)(az.i[dz] * D.ny + ay.i[dy]) * D.nx + ax.i[dx];
      corner[c] = volume + p;
      const float tri = (ax.w[dx] * ay.w[dy]) * az.w[dz];
      const float v = visibility(*vis, maps + p * map_floats, probe_position(D, ax.i[dx], ay.i[dy], az.i[dz]), position, nrm);
      w[c] = v * tri;
      if (!(corner[c]->hit_fraction <= D.max_hit_fraction)) w[c] = 0.0f;
      W = W + w[c];
    }
    rt_irradiance& r = out[i];
    if (!(W > 0.0f)) {
      r.rgb[0] = r.rgb[1] = r.rgb[2] = r.hit_fraction = 0.0f;
      continue;
    }
    float coef[9][3];
    for (int k = 0; k < 9; k++)
      for (int ch = 0; ch < 3; ch++) {
        float S = 0.0f;
        for (int c = 0; c < 8; c++)
          if (w[c] != 0.0f) S = S + w[c] * corner[c]->sh[k][ch];
        coef[k][ch] = rt_div(S, W);
      }
    const rt3 d = nrm;
    float Y[9];
    Y[0] = 0.282094792f;
    Y[1] = 0.488602512f * d.y;
    Y[2] = 0.488602512f * d.z;
    Y[3] = 0.488602512f * d.x;
    Y[4] = 1.092548431f * (d.x * d.y);
    Y[5] = 1.092548431f * (d.y * d.z);
    Y[6] = 0.315391565f * (3.0f * (d.z * d.z) - 1.0f);
    Y[7] = 1.092548431f * (d.x * d.z);
    Y[8] = 0.546274215f * (d.x * d.x - d.y * d.y);
    for (int ch = 0; ch < 3; ch++) {
      float E = 0.0f;
      for (int k = 0; k < 9; k++) E = E + coef[k][ch] * Y[k];
      r.rgb[ch] = rt_max(0.0f, E);
    }
    r.hit_fraction = W;
  }
}

// out: the image of ny * nz * (size + 2) rows of nx * (size + 2) texels, 2 f32 (f16 == 0) or 2 half bit patterns per texel
void vvis_model_tiles(const rt_volume_desc* desc, const rt_volume_visibility_desc* vis, const float* maps, int f16, void* out) {
  const rt_volume_desc& D = *desc;
  const uint32_t size = vis->size, tile = size + 2u, width = D.nx * tile;
  const uint32_t n = probe_count(D);
  for (uint32_t p = 0; p < n; p++) {
    const uint32_t tx = p % D.nx, ty = p / D.nx;
    for (uint32_t b = 0; b < tile; b++)
      for (uint32_t a = 0; a < tile; a++) {
        int wrapped = 0;
        const float* t = maps + 2 * ((size_t)p * size * size + wrap((int)a - 1, (int)b - 1, (int)size, &wrapped));
        const size_t at = ((size_t)(ty * tile + b) * width + tx * tile + a) * 2;
        for (int k = 0; k < 2; k++) {
          if (f16)
            ((uint16_t*)out)[at + k] = rt_f32_to_f16(t[k]);
          else
            ((float*)out)[at + k] = t[k];
        }
      }
  }
}

}  // extern "C"
