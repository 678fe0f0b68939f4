// denoise_model.cpp — one pass of the denoise rule of include/mi355rt.h ("atlas denoise") restated for the CPU in plain loops:
// a linear search for every texel's lowest guide, then per guided texel the 25 taps in the order of the rule.  No index map
// made by a minimum, no tiles, no windows: nothing of csrc/k_denoise.hip.h is shared.  Also counts, over the non-centre taps
// of guided texels, how each was decided.  Python composes passes (tests/denoise_util.py).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "mi355rt_math.h"

extern "C" {

// in, out: W * H texels of 4 f32 (out is another array).  points: n records of 8 f32 {position, t_max, normal, pad}; texels: n
// u32.  counts: six u64 - accepted, outside the atlas, unguided, rejected by the normal, by the plane, by the distance (the
// first test that fails, in the order of the rule).
void denoise_model_pass(const float* in, uint32_t W, uint32_t H, uint32_t step, float normal_cos, float plane_eps, float max_dist,
                        const float* points, const uint32_t* texels, uint32_t n, float* out, uint64_t* counts) {
  const int64_t w = W, h = H, s = step;
  // the guide of texel i: the lowest j with texels[j] == i, -1 for none; an index past the atlas is ignored
  std::vector<int64_t> guide((size_t)(w * h), -1);
  for (int64_t j = (int64_t)n - 1; j >= 0; j--)
    if ((int64_t)texels[j] < w * h) guide[texels[j]] = j;
  for (int k = 0; k < 6; k++) counts[k] = 0;
  const float kw[3] = {0.375f, 0.25f, 0.0625f};
  const float md2 = max_dist * max_dist;
  for (int64_t y = 0; y < h; y++)
    for (int64_t x = 0; x < w; x++) {
      const int64_t i = y * w + x;
      if (guide[i] < 0) {
        std::memcpy(out + 4 * i, in + 4 * i, 16);
        continue;
      }
      const float* P = points + 8 * guide[i];
      const float* N = P + 4;
      float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wsum = 0.0f;
      for (int64_t dy = -2; dy <= 2; dy++)
        for (int64_t dx = -2; dx <= 2; dx++) {
          const float hw = kw[dx < 0 ? -dx : dx] * kw[dy < 0 ? -dy : dy];
          const int64_t qx = x + dx * s, qy = y + dy * s;
          if (dx != 0 || dy != 0) {
            if (qx < 0 || qy < 0 || qx >= w || qy >= h) { counts[1]++; continue; }
            const int64_t g = guide[qy * w + qx];
            if (g < 0) { counts[2]++; continue; }
            const float* Pq = points + 8 * g;
            const float* Nq = Pq + 4;
            if (!((N[0] * Nq[0] + N[1] * Nq[1]) + N[2] * Nq[2] >= normal_cos)) { counts[3]++; continue; }
            const float d[3] = {Pq[0] - P[0], Pq[1] - P[1], Pq[2] - P[2]};
            if (!(std::fabs((N[0] * d[0] + N[1] * d[1]) + N[2] * d[2]) <= plane_eps)) { counts[4]++; continue; }
            if (!((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= md2)) { counts[5]++; continue; }
            counts[0]++;
          }
          const float* c = in + 4 * (qy * w + qx);
          for (int k = 0; k < 4; k++) acc[k] = acc[k] + hw * c[k];
          wsum = wsum + hw;
        }
      for (int k = 0; k < 4; k++) out[4 * i + k] = rt_div(acc[k], wsum);
    }
}

}  // extern "C"
