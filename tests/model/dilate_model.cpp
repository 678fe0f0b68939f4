// dilate_model.cpp — the dilation rule of include/mi355rt.h ("atlas dilation") restated for the CPU as a brute force: for
// every uncovered texel EVERY texel of the disc is visited, and the covered one with the smallest (d2, index) is its source.
// No bitmap, no row order, no early exit: nothing of csrc/k_dilate.hip.h is shared.  Also reports, per filled texel, whether
// more than one covered texel attained the smallest d2 (a tie the index had to break).
#include <cstdint>
#include <cstring>

extern "C" {

// atlas: W * H texels of 4 f32, dilated in place.  src: W * H u32 (own index / source index / 0xffffffff).  tie: W * H bytes,
// 1 where a filled texel had several nearest covered texels.  Returns the number of filled texels.
uint32_t dilate_model(float* atlas, uint32_t W, uint32_t H, uint32_t R, uint32_t* src, uint8_t* tie) {
  const int64_t w = W, h = H, r = R;
  // coverage is decided on the input, before anything is written
  for (int64_t i = 0; i < w * h; i++) {
    const bool covered = atlas[4 * i + 3] >= 0.0f;   // false for NaN
    src[i] = covered ? (uint32_t)i : 0xffffffffu;
    tie[i] = 0;
  }
  uint32_t filled = 0;
  for (int64_t y = 0; y < h; y++)
    for (int64_t x = 0; x < w; x++) {
      const int64_t i = y * w + x;
      if (atlas[4 * i + 3] >= 0.0f) continue;
      int64_t best_d2 = -1, best = -1, attained = 0;
      for (int64_t sy = y - r; sy <= y + r; sy++)
        for (int64_t sx = x - r; sx <= x + r; sx++) {
          if (sx < 0 || sy < 0 || sx >= w || sy >= h) continue;   // texels outside the atlas do not exist
          const int64_t d2 = (sx - x) * (sx - x) + (sy - y) * (sy - y);
          if (d2 > r * r) continue;
          const int64_t s = sy * w + sx;
          if (!(atlas[4 * s + 3] >= 0.0f)) continue;
          if (best < 0 || d2 < best_d2 || (d2 == best_d2 && s < best)) {
            attained = (best >= 0 && d2 == best_d2) ? attained + 1 : 1;
            best_d2 = d2;
            best = s;
          } else if (d2 == best_d2) {
            attained++;
          }
        }
      if (best < 0) continue;
      src[i] = (uint32_t)best;
      tie[i] = attained > 1;
      filled++;
    }
  // sources are covered texels, which are never written: the copies can be made in any order
  const float minus_two = -2.0f;
  for (int64_t i = 0; i < w * h; i++)
    if (src[i] != 0xffffffffu && src[i] != (uint32_t)i) {
      std::memcpy(atlas + 4 * i, atlas + 4 * (int64_t)src[i], 12);
      std::memcpy(atlas + 4 * i + 3, &minus_two, 4);
    }
  return filled;
}

}  // extern "C"
