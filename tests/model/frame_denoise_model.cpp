// frame_denoise_model.cpp — the frame denoise rule of include/mi355rt.h ("THE FRAME DENOISE RULE") restated for the CPU in plain
// loops on the two public headers: prepare, one pass, finish and their composition into a call.  No tiles, no windows, no
// forms: nothing of csrc/k_frame_denoise.hip.h is shared.  A pass can also report, per pixel, the extremes of the colours of
// the taps it accepted and how many it accepted.  Has a main of its own (a small self-check), so that the same file builds
// as a stand-alone program - under a sanitizer, if wanted - and as the shared library tests/frame_denoise_util.py loads.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mi355rt.h"
#include "mi355rt_math.h"

namespace {

float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

void modulation(uint32_t alb, uint32_t flags, float m[3]) {
  if (!(flags & RT_FRAME_DENOISE_DEMODULATE) || (alb >> 24) == 0u) {
    m[0] = m[1] = m[2] = 1.0f;
    return;
  }
  for (int c = 0; c < 3; c++) m[c] = rt_max(rt_from_unorm8((alb >> (8 * c)) & 255u), RT_FRAME_DENOISE_MIN_ALBEDO);
}

// q(x, y) of the rule, coordinates clamped
void quantity(const float* accum, const uint32_t* albedo, uint32_t flags, int W, int H, int cx, int cy, float q[3]) {
  const int x = clampi(cx, W - 1), y = clampi(cy, H - 1);
  const float* a = accum + 4 * ((size_t)y * W + x);
  float rad[3] = {0.0f, 0.0f, 0.0f};
  if (!(a[3] <= 0.0f))
    for (int c = 0; c < 3; c++) rad[c] = a[c] / a[3];
  float m[3];
  modulation(albedo[(size_t)y * W + x], flags, m);
  for (int c = 0; c < 3; c++) q[c] = rt_div(rad[c], m[c]);
}

}  // namespace

extern "C" {

// accum: W * H x 4 f32; albedo: W * H u32; normal_id: W * H x 4 f32; depth: W * H f32; U: the frame's uniform block.
// col: W * H x 4 f32 {q, var}; guide: W * H x 8 f32 {P, bits(inst)} {N, bits(surface)}; mod: W * H x 4 f32 {m, alpha}.
void fd_model_prepare(const float* accum, const uint32_t* albedo, const float* normal_id, const float* depth,
                      const rt_scene_uniforms* U, uint32_t flags, float* col, float* guide, float* mod) {
  const int W = (int)U->width, H = (int)U->height;
  const rt3 eye = rt3_make(U->camera.origin[0], U->camera.origin[1], U->camera.origin[2]);
  const rt3 ll = rt3_make(U->camera.lower_left[0], U->camera.lower_left[1], U->camera.lower_left[2]);
  const rt3 hor = rt3_make(U->camera.horizontal[0], U->camera.horizontal[1], U->camera.horizontal[2]);
  const rt3 ver = rt3_make(U->camera.vertical[0], U->camera.vertical[1], U->camera.vertical[2]);
  const rt3 center = ll + hor * 0.5f + ver * 0.5f;
  const float focal = rt_length(center - eye);
  const float ca = 10000.0f / (10000.0f - 0.001f), cb = (10000.0f * 0.001f) / (10000.0f - 0.001f);
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      const size_t i = (size_t)y * W + x;
      float q[3], m[3];
      quantity(accum, albedo, flags, W, H, x, y, q);
      modulation(albedo[i], flags, m);
      float m1 = 0.0f, m2 = 0.0f;
      for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
          float n[3];
          quantity(accum, albedo, flags, W, H, x + dx, y + dy, n);
          const float l = lum(n[0], n[1], n[2]);
          m1 = m1 + l;
          m2 = m2 + l * l;
        }
      const float mean = rt_div(m1, 9.0f);
      const float var = rt_max(rt_div(m2, 9.0f) - mean * mean, 0.0f);
      col[4 * i + 0] = q[0]; col[4 * i + 1] = q[1]; col[4 * i + 2] = q[2]; col[4 * i + 3] = var;
      mod[4 * i + 0] = m[0]; mod[4 * i + 1] = m[1]; mod[4 * i + 2] = m[2];
      mod[4 * i + 3] = accum[4 * i + 3] > 0.0f ? 1.0f : 0.0f;
      float* g = guide + 8 * i;
      for (int k = 0; k < 8; k++) g[k] = 0.0f;
      if ((albedo[i] >> 24) == 0u) continue;
      const float ox = normal_id[4 * i], oy = normal_id[4 * i + 1];
      rt3 n = rt3_make(ox, oy, 1.0f - rt_abs(ox) - rt_abs(oy));
      const float t = rt_saturate(-n.z);
      n.x += (n.x >= 0.0f) ? -t : t;
      n.y += (n.y >= 0.0f) ? -t : t;
      const rt3 N = rt_normalize(n);
      const float u = ((float)x + 0.5f + U->jitter[0] * (float)W) / (float)W;
      const float v = 1.0f - ((float)y + 0.5f + U->jitter[1] * (float)H) / (float)H;
      const rt3 d = ll + u * hor + v * ver - eye;
      const float z_view = rt_div(cb, ca - depth[i]);
      const float th = rt_div(z_view, focal);
      g[0] = eye.x + d.x * th; g[1] = eye.y + d.y * th; g[2] = eye.z + d.z * th;
      g[3] = normal_id[4 * i + 3];
      g[4] = N.x; g[5] = N.y; g[6] = N.z;
      g[7] = rt_u2f(1u);
    }
}

// One pass at spacing `step`.  lo, hi (W * H x 3 f32) and accepted (W * H u32) may be NULL: the extremes of the colours of
// the accepted taps of a surface pixel (NaN colours skipped) and their number, the centre included.
void fd_model_pass(const float* in, const float* guide, uint32_t W_, uint32_t H_, uint32_t step, uint32_t flags, float normal_cos,
                   float plane_eps, float sigma_lum, float* out, float* lo, float* hi, uint32_t* accepted) {
  const int64_t W = W_, H = H_, s = step;
  const float kw[3] = {0.375f, 0.25f, 0.0625f};
  for (int64_t y = 0; y < H; y++)
    for (int64_t x = 0; x < W; x++) {
      const int64_t i = y * W + x;
      const float* g = guide + 8 * i;
      if (accepted) accepted[i] = 0;
      if (rt_f2u(g[7]) == 0u) {
        std::memcpy(out + 4 * i, in + 4 * i, 16);
        continue;
      }
      const float lum_p = lum(in[4 * i], in[4 * i + 1], in[4 * i + 2]);
      const float den = sigma_lum * rt_sqrt(in[4 * i + 3]) + 1e-4f;
      float acc[3] = {0.0f, 0.0f, 0.0f}, vacc = 0.0f, wsum = 0.0f;
      float l[3] = {INFINITY, INFINITY, INFINITY}, h3[3] = {-INFINITY, -INFINITY, -INFINITY};
      for (int64_t dy = -2; dy <= 2; dy++)
        for (int64_t dx = -2; dx <= 2; dx++) {
          const float hw = kw[dx < 0 ? -dx : dx] * kw[dy < 0 ? -dy : dy];
          const int64_t qx = x + dx * s, qy = y + dy * s;
          if (dx != 0 || dy != 0) {
            if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
            const float* gq = guide + 8 * (qy * W + qx);
            if (rt_f2u(gq[7]) == 0u) continue;
            if ((flags & RT_FRAME_DENOISE_SAME_INSTANCE) && rt_f2u(gq[3]) != rt_f2u(g[3])) continue;
            if (!((g[4] * gq[4] + g[5] * gq[5]) + g[6] * gq[6] >= normal_cos)) continue;
            const float e[3] = {gq[0] - g[0], gq[1] - g[1], gq[2] - g[2]};
            if (!(rt_abs((g[4] * e[0] + g[5] * e[1]) + g[6] * e[2]) <= plane_eps)) continue;
          }
          const float* c = in + 4 * (qy * W + qx);
          float w = hw;
          if (sigma_lum > 0.0f) w = hw * rt_exp(rt_div(-rt_abs(lum(c[0], c[1], c[2]) - lum_p), den));
          for (int k = 0; k < 3; k++) acc[k] = acc[k] + w * c[k];
          vacc = vacc + (w * w) * c[3];
          wsum = wsum + w;
          if (accepted) accepted[i]++;
          for (int k = 0; k < 3; k++) {
            if (c[k] < l[k]) l[k] = c[k];
            if (c[k] > h3[k]) h3[k] = c[k];
          }
        }
      for (int k = 0; k < 3; k++) out[4 * i + k] = rt_div(acc[k], wsum);
      out[4 * i + 3] = rt_div(vacc, wsum * wsum);
      if (lo) for (int k = 0; k < 3; k++) lo[3 * i + k] = l[k];
      if (hi) for (int k = 0; k < 3; k++) hi[3 * i + k] = h3[k];
    }
}

void fd_model_finish(const float* col, const float* mod, uint64_t n, float* out) {
  for (uint64_t i = 0; i < n; i++) {
    for (int k = 0; k < 3; k++) out[4 * i + k] = col[4 * i + k] * mod[4 * i + k];
    out[4 * i + 3] = mod[4 * i + 3];
  }
}

// a call: prepare, the passes at step << p, finish.  Returns 0, or -1 for a descriptor the library refuses.
int fd_model_call(const float* accum, const uint32_t* albedo, const float* normal_id, const float* depth,
                  const rt_scene_uniforms* U, const rt_frame_denoise_desc* d, float* out) {
  if (d->passes == 0 || d->passes > RT_FRAME_DENOISE_MAX_PASSES || d->step == 0 || d->step > RT_FRAME_DENOISE_MAX_STEP ||
      (d->step << (d->passes - 1)) > RT_FRAME_DENOISE_MAX_STEP || d->reserved[0] || d->reserved[1] ||
      (d->flags & ~(RT_FRAME_DENOISE_DEMODULATE | RT_FRAME_DENOISE_SAME_INSTANCE)))
    return -1;
  const size_t n = (size_t)U->width * U->height;
  std::vector<float> col(4 * n), guide(8 * n), mod(4 * n), tmp(4 * n);
  fd_model_prepare(accum, albedo, normal_id, depth, U, d->flags, col.data(), guide.data(), mod.data());
  for (uint32_t p = 0; p < d->passes; p++) {
    fd_model_pass(col.data(), guide.data(), U->width, U->height, d->step << p, d->flags, d->normal_cos, d->plane_eps, d->sigma_lum,
                  tmp.data(), nullptr, nullptr, nullptr);
    col.swap(tmp);
  }
  fd_model_finish(col.data(), mod.data(), n, out);
  return 0;
}

}  // extern "C"

// Self-check: a constant image over a wall facing the camera stays constant to a few ulps, and the background passes through.
int main() {
  const uint32_t W = 21, H = 13;
  rt_scene_uniforms U;
  std::memset(&U, 0, sizeof(U));
  U.width = W;
  U.height = H;
  const float cam[16] = {0, 0, 0, 0, -1, -1, -1, 0, 2, 0, 0, 0, 0, 2, 0, 0};
  std::memcpy(&U.camera, cam, sizeof(cam));
  const size_t n = (size_t)W * H;
  std::vector<float> accum(4 * n), nid(4 * n, 0.0f), depth(n), out(4 * n);
  std::vector<uint32_t> alb(n, 0xff808080u);
  const float ca = 10000.0f / (10000.0f - 0.001f), cb = (10000.0f * 0.001f) / (10000.0f - 0.001f);
  for (size_t i = 0; i < n; i++) {
    accum[4 * i] = 0.75f; accum[4 * i + 1] = 1.5f; accum[4 * i + 2] = 3.0f; accum[4 * i + 3] = 3.0f;
    depth[i] = ca - cb / 2.0f;   // z_view = 2 everywhere: the plane z = -2, normal +z (oct 0, 0)
  }
  alb[0] = 0u;   // one background pixel
  accum[0] = 9.0f;
  rt_frame_denoise_desc d = {4, 1, RT_FRAME_DENOISE_DEMODULATE, 0.9f, 0.05f, 4.0f, {0, 0}};
  if (fd_model_call(accum.data(), alb.data(), nid.data(), depth.data(), &U, &d, out.data()) != 0) return 2;
  int bad = 0;
  for (size_t i = 1; i < n; i++)
    for (int k = 0; k < 3; k++)
      if (!(std::fabs(out[4 * i + k] - accum[4 * i + k] / 3.0f) <= 1e-5f)) bad++;
  if (out[0] != 3.0f || out[3] != 1.0f) bad++;
  std::printf("frame_denoise_model self-check: %d bad words of %zu\n", bad, 3 * n);
  return bad ? 1 : 0;
}
