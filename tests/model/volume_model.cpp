// volume_model.cpp — TEST INFRASTRUCTURE: the reference of irradiance volumes (mi355rt.h "THE VOLUME RULE").
// A stand-alone restatement of the rule's three parts - the probes of a grid, the finish, the sample - and of the layer
// export, in plain scalar C++ on mi355rt_math.h and mi355rt_layout.h alone: one point at a time, one loop per sentence of the
// rule, nothing shared with csrc/k_volume.hip.h.  The path work between probes and finish is the probe gather's, whose
// reference is tests/model/probe_model.cpp; tests/test_volume_model.py puts the two together.
// build: the flags of oracle/Makefile, -I include (tests/volume_util.py does it)
#include <cstddef>
#include <cstdint>

#include "mi355rt_layout.h"
#include "mi355rt_math.h"

namespace {

uint32_t probe_count(const rt_volume_desc& D) { return D.nx * D.ny * D.nz; }

int band_of(int k) { return k == 0 ? 0 : k <= 3 ? 1 : 2; }

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

}  // namespace

extern "C" {

// probes: nx * ny * nz rt_probe, written
void volume_model_probes(const rt_volume_desc* desc, rt_probe* probes) {
  const rt_volume_desc& D = *desc;
  for (uint32_t z = 0; z < D.nz; z++)
    for (uint32_t y = 0; y < D.ny; y++)
      for (uint32_t x = 0; x < D.nx; x++) {
        const uint32_t p = (z * D.ny + y) * D.nx + x;
        rt_probe& q = probes[p];
        const float fx = (float)x * D.step[0], fy = (float)y * D.step[1], fz = (float)z * D.step[2];
        q.position[0] = D.origin[0] + fx;
        q.position[1] = D.origin[1] + fy;
        q.position[2] = D.origin[2] + fz;
        q.t_max = D.t_max;
        q.unused[0] = q.unused[1] = q.unused[2] = 0.0f;
        q.pad = D.pad_first + p;
      }
}

// volume: nx * ny * nz rt_probe_sh9 of radiance coefficients, finished in place
void volume_model_finish(const rt_volume_desc* desc, rt_probe_sh9* volume) {
  static const float A[3] = {3.141592654f, 2.094395102f, 0.785398163f};
  const uint32_t n = probe_count(*desc);
  for (uint32_t p = 0; p < n; p++)
    for (int k = 0; k < 9; k++)
      for (int c = 0; c < 3; c++) {
        const float scaled = volume[p].sh[k][c] * A[band_of(k)];
        volume[p].sh[k][c] = scaled * desc->window[band_of(k)];
      }
}

// points: n rt_gather_point; out: n rt_irradiance
void volume_model_sample(const rt_volume_desc* desc, const rt_probe_sh9* volume, const rt_gather_point* points, uint32_t n,
                         rt_irradiance* out) {
  const rt_volume_desc& D = *desc;
  for (uint32_t i = 0; i < n; i++) {
    const rt_gather_point& pt = points[i];
    const Axis ax = cell(pt.position[0], D.origin[0], D.step[0], D.nx);
    const Axis ay = cell(pt.position[1], D.origin[1], D.step[1], D.ny);
    const Axis az = cell(pt.position[2], D.origin[2], D.step[2], D.nz);
    const rt_probe_sh9* corner[8];
    float w[8];
    float W = 0.0f;
    for (int c = 0; c < 8; c++) {
      const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
      corner[c] = volume + ((size_t)(az.i[dz] * D.ny + ay.i[dy]) * D.nx + ax.i[dx]);
      w[c] = (ax.w[dx] * ay.w[dy]) * az.w[dz];
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
    const rt3 d = rt_normalize(rt3_make(pt.normal[0], pt.normal[1], pt.normal[2]));
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

// out: 7 layers of n texels, 4 f32 (f16 == 0) or 4 half bit patterns (f16 != 0) per texel
void volume_model_layers(const rt_volume_desc* desc, const rt_probe_sh9* volume, int f16, void* out) {
  const uint32_t n = probe_count(*desc);
  for (uint32_t j = 0; j < 7; j++)
    for (uint32_t p = 0; p < n; p++)
      for (uint32_t i = 0; i < 4; i++) {
        const float v = ((const float*)&volume[p])[4 * j + i];
        const size_t at = ((size_t)j * n + p) * 4 + i;
        if (f16)
          ((uint16_t*)out)[at] = rt_f32_to_f16(v);
        else
          ((float*)out)[at] = v;
      }
}

}  // extern "C"
