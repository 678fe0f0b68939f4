// frame_temporal_model.cpp — the frame temporal rule of include/mi355rt.h ("THE FRAME TEMPORAL RULE") restated for the CPU in
// plain loops on the two public headers: one run of the stage over an image.  Nothing of csrc/k_frame_temporal.hip.h is
// shared.  The stage can also report, per pixel, how many taps it accepted.  Has a main of its own (a small self-check), so
// that the same file builds as a stand-alone program - under a sanitizer, if wanted - and as the shared library
// tests/frame_temporal_util.py loads.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mi355rt.h"
#include "mi355rt_math.h"

namespace {

float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

}  // namespace

extern "C" {

// col: W * H x 4 f32 {c, vs} and guide: W * H x 8 f32 of the current frame (fd_model_prepare's outputs).  prev_hist (x 4),
// prev_mom (x 2), prev_guide (x 8) and prev_U: the previous set and the block of its frame; prev_hist == NULL: none is kept.
// Out: integ (x 4), hist (x 4), mom (x 2); accepted (W * H u32, may be NULL).  Returns 0, or -1 for a descriptor the library
// refuses.
int ft_model_stage(const float* col, const float* guide, const float* prev_hist, const float* prev_mom, const float* prev_guide,
                   const rt_scene_uniforms* prev_U, const rt_frame_temporal_desc* d, uint32_t W_, uint32_t H_, float* integ,
                   float* hist, float* mom, uint32_t* accepted) {
  if ((d->flags & ~RT_FRAME_TEMPORAL_SAME_INSTANCE) || d->reserved[0] || d->reserved[1] || d->reserved[2] || d->max_history == 0 ||
      d->max_history > RT_FRAME_TEMPORAL_MAX_HISTORY || d->var_history == 0)
    return -1;
  const int64_t W = W_, H = H_;
  const float Wf = (float)W_, Hf = (float)H_;
  float eye[3] = {0, 0, 0}, c0[3] = {0, 0, 0}, hor[3] = {0, 0, 0}, ver[3] = {0, 0, 0}, nrm[3] = {0, 0, 0}, jx = 0.0f, jy = 0.0f;
  if (prev_hist) {
    for (int k = 0; k < 3; k++) {
      eye[k] = prev_U->camera.origin[k];
      c0[k] = prev_U->camera.lower_left[k] - eye[k];
      hor[k] = prev_U->camera.horizontal[k];
      ver[k] = prev_U->camera.vertical[k];
    }
    nrm[0] = hor[1] * ver[2] - hor[2] * ver[1];
    nrm[1] = hor[2] * ver[0] - hor[0] * ver[2];
    nrm[2] = hor[0] * ver[1] - hor[1] * ver[0];
    jx = prev_U->jitter[0];
    jy = prev_U->jitter[1];
  }
  for (int64_t y = 0; y < H; y++)
    for (int64_t x = 0; x < W; x++) {
      const int64_t i = y * W + x;
      const float* c = col + 4 * i;
      const float* g = guide + 8 * i;
      if (accepted) accepted[i] = 0;
      if (rt_f2u(g[7]) == 0u) {   // background
        std::memcpy(integ + 4 * i, c, 16);
        std::memcpy(hist + 4 * i, c, 12);
        hist[4 * i + 3] = 0.0f;
        mom[2 * i] = mom[2 * i + 1] = 0.0f;
        continue;
      }
      const float l = lum(c[0], c[1], c[2]);
      float wsum = 0.0f, acc[3] = {0.0f, 0.0f, 0.0f}, s1 = 0.0f, s2 = 0.0f, n_prev = 0.0f;
      int n_acc = 0;
      if (prev_hist && d->max_history != 1u) {
        float e[3], r[3];
        for (int k = 0; k < 3; k++) e[k] = g[k] - eye[k];
        const float s = rt_div(dot3(c0, nrm), dot3(e, nrm));
        for (int k = 0; k < 3; k++) r[k] = e[k] * s - c0[k];
        const float u = rt_div(dot3(r, hor), dot3(hor, hor));
        const float v = rt_div(dot3(r, ver), dot3(ver, ver));
        const float fx = (u * Wf - 0.5f) - jx * Wf;
        const float fy = ((1.0f - v) * Hf - 0.5f) - jy * Hf;
        if (s > 0.0f && fx >= -1.0f && fx < Wf && fy >= -1.0f && fy < Hf) {
          const int64_t x0 = (int64_t)rt_floor(fx), y0 = (int64_t)rt_floor(fy);
          const float tx = fx - rt_floor(fx), ty = fy - rt_floor(fy);
          const float w4[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
          for (int t = 0; t < 4; t++) {
            const float w = w4[t];
            if (!(w > 0.0f)) continue;
            const int64_t qx = x0 + (t & 1), qy = y0 + (t >> 1);
            if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
            const int64_t q = qy * W + qx;
            const float* gq = prev_guide + 8 * q;
            const float* hq = prev_hist + 4 * q;
            if (rt_f2u(gq[7]) == 0u) continue;
            if (!(hq[3] >= 1.0f)) continue;
            if ((d->flags & RT_FRAME_TEMPORAL_SAME_INSTANCE) && rt_f2u(gq[3]) != rt_f2u(g[3])) continue;
            if (!(dot3(g + 4, gq + 4) >= d->normal_cos)) continue;
            const float dp[3] = {gq[0] - g[0], gq[1] - g[1], gq[2] - g[2]};
            if (!(rt_abs(dot3(g + 4, dp)) <= d->plane_eps)) continue;
            wsum = wsum + w;
            for (int k = 0; k < 3; k++) acc[k] = acc[k] + w * hq[k];
            s1 = s1 + w * prev_mom[2 * q];
            s2 = s2 + w * prev_mom[2 * q + 1];
            if (n_acc == 0 || hq[3] < n_prev) n_prev = hq[3];
            n_acc++;
          }
        }
      }
      if (accepted) accepted[i] = (uint32_t)n_acc;
      if (n_acc == 0) {   // no history
        std::memcpy(integ + 4 * i, c, 16);
        std::memcpy(hist + 4 * i, c, 12);
        hist[4 * i + 3] = 1.0f;
        mom[2 * i] = l;
        mom[2 * i + 1] = l * l;
        continue;
      }
      float n = n_prev + 1.0f;
      if (!(n < (float)d->max_history)) n = (float)d->max_history;
      const float a = rt_div(1.0f, n);
      for (int k = 0; k < 3; k++) {
        const float h = rt_div(acc[k], wsum);
        const float q = h + a * (c[k] - h);
        integ[4 * i + k] = hist[4 * i + k] = q;
      }
      const float hm1 = rt_div(s1, wsum), hm2 = rt_div(s2, wsum);
      const float m1 = hm1 + a * (l - hm1), m2 = hm2 + a * (l * l - hm2);
      integ[4 * i + 3] = n >= (float)d->var_history ? rt_max(m2 - m1 * m1, 0.0f) : c[3];
      hist[4 * i + 3] = n;
      mom[2 * i] = m1;
      mom[2 * i + 1] = m2;
    }
  return 0;
}

}  // extern "C"

// Self-check: a constant image on a wall facing a static camera keeps its constant to a few ulps over six frames, n grows to
// max_history and stops, and a background pixel passes through with n = 0.
int main() {
  const uint32_t W = 21, H = 13;
  rt_scene_uniforms U;
  std::memset(&U, 0, sizeof(U));
  U.width = W;
  U.height = H;
  const float cam[16] = {0, 0, 0, 0, -1, -1, -1, 0, 2, 0, 0, 0, 0, 2, 0, 0};
  std::memcpy(&U.camera, cam, sizeof(cam));
  U.jitter[0] = 0.004f;
  U.jitter[1] = -0.003f;
  const size_t n = (size_t)W * H;
  std::vector<float> col(4 * n), guide(8 * n, 0.0f), integ(4 * n), hist[2], mom[2];
  for (int k = 0; k < 2; k++) hist[k].assign(4 * n, 0.0f), mom[k].assign(2 * n, 0.0f);
  for (uint32_t y = 0; y < H; y++)
    for (uint32_t x = 0; x < W; x++) {
      const size_t i = (size_t)y * W + x;
      col[4 * i] = 0.25f; col[4 * i + 1] = 0.5f; col[4 * i + 2] = 1.7f; col[4 * i + 3] = 0.125f;
      if (i == 0) continue;   // one background pixel: its guide stays zero
      const float u = ((float)x + 0.5f + U.jitter[0] * (float)W) / (float)W;
      const float v = 1.0f - ((float)y + 0.5f + U.jitter[1] * (float)H) / (float)H;
      float* g = guide.data() + 8 * i;   // the plane z = -2: the pixel's ray (-1 + 2 u, -1 + 2 v, -1) times 2
      g[0] = (-1.0f + u * 2.0f) * 2.0f; g[1] = (-1.0f + v * 2.0f) * 2.0f; g[2] = -2.0f;
      g[6] = 1.0f;
      g[7] = rt_u2f(1u);
    }
  const rt_frame_temporal_desc d = {0, 4, 3, 0.9f, 0.01f, {0, 0, 0}};
  int bad = 0, cur = 0;
  for (int f = 0; f < 6; f++) {
    const bool have = f > 0;
    if (ft_model_stage(col.data(), guide.data(), have ? hist[cur].data() : nullptr, mom[cur].data(), guide.data(), &U, &d, W, H,
                       integ.data(), hist[cur ^ 1].data(), mom[cur ^ 1].data(), nullptr) != 0)
      return 2;
    cur ^= 1;
    const float want_n = (float)(f + 1 < 4 ? f + 1 : 4);
    for (size_t i = 1; i < n; i++) {
      if (hist[cur][4 * i + 3] != want_n) bad++;
      for (int k = 0; k < 3; k++)
        if (!(std::fabs(integ[4 * i + k] - col[4 * i + k]) <= 1e-5f * col[4 * i + k])) bad++;
    }
    if (hist[cur][3] != 0.0f || std::memcmp(integ.data(), col.data(), 16) != 0) bad++;
  }
  std::printf("frame_temporal_model self-check: %d bad words\n", bad);
  return bad ? 1 : 0;
}
