// k_dilate.hip.h — k_dilate_mask, k_dilate_source and k_dilate_apply: the nearest-texel gutter fill of a baked atlas
// (rt_dilate_atlas, mi355rt.h "atlas dilation").
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_DILATE_HIP_H
#define MI355RT_K_DILATE_HIP_H

namespace rtk {

// The rule is integer arithmetic on a coverage bitmap; no float is computed, only compared (w >= 0.0f) and copied.
//   k_dilate_mask    one wave per 64 consecutive texels of a row: the ballot of w >= 0.0f is one u64 of the bitmap, ceil(W /
//                    64) words per row, bits past W zero
//   k_dilate_source  one workgroup per 16 x 16 tile: the 64 x 64 window around it (RT_DILATE_MAX_RADIUS texels on every
//                    side) as 64 u64 in LDS, then per lane a scan over the rows dy = -R .. R; writes the source map and adds
//                    the tile's filled texels to the count
//   k_dilate_apply   one thread per texel: a filled texel copies its source's 16 bytes with w = -2.0f
// THE ORDER.  A row's nearest set bit (smallest |dx|, the left one when both sides are as near) is the only texel of that row
// that can win: any other has a larger d2, or the same d2 and a higher index.  Rows are visited in ascending dy and a
// candidate replaces the best only when its d2 is STRICTLY smaller, so among equal d2 the lowest row stays, and a lower row
// is a lower index.  Together: smallest d2, then lowest texel index.
// Nothing here reads what another workgroup of the same launch wrote: the mask reads w, the source pass reads the bitmap of
// the launch before it, and the apply pass reads covered texels (which no thread writes) and writes uncovered ones (which no
// thread reads).
#define RT_DILATE_TILE 16u
#define RT_DILATE_WINDOW 64u   // RT_DILATE_TILE + 2 * RT_DILATE_MAX_RADIUS: one u64 per window row
#define RT_DILATE_NONE 0xffffffffu
static_assert(RT_DILATE_TILE + 2u * RT_DILATE_MAX_RADIUS <= RT_DILATE_WINDOW, "a window row is one u64");

struct DilateArgs {
  float4* atlas;            // W * H texels, row-major
  uint64_t* bitmap;         // H * wpr words
  uint32_t* src;            // W * H: the source map
  uint32_t* filled;         // one u32, zeroed by the host before the launch, or null
  uint32_t W, H, R;
  uint32_t wpr;             // ceil(W / 64)
  uint32_t tiles_x;         // ceil(W / 16)
};

// Wave g of the grid holds word g of the bitmap: row g / wpr, columns 64 * (g % wpr) .. + 63.  n_words = H * wpr <= 2^24.
__global__ __launch_bounds__(256)
void k_dilate_mask(DilateArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = blockIdx.x * 4u + (threadIdx.x >> 6);   // wave-uniform
  if (g >= A.H * A.wpr) return;
  const uint32_t y = g / A.wpr;
  const uint32_t x = (g - y * A.wpr) * 64u + lane;
  bool covered = false;
  if (x < A.W) covered = A.atlas[(size_t)y * A.W + x].w >= 0.0f;   // false for NaN
  const uint64_t word = __ballot(covered);
  if (lane == 0u) A.bitmap[g] = word;
}

// Workgroup `blockIdx.x` holds tile (blockIdx.x % tiles_x, blockIdx.x / tiles_x); thread t its texel (t % 16, t / 16).  Bit b
// of window row r is texel (x0 - 24 + b, y0 - 24 + r); texels outside the atlas are zero bits.
__global__ __launch_bounds__(256)
void k_dilate_source(DilateArgs A) {
  __shared__ uint64_t win[RT_DILATE_WINDOW];
  __shared__ uint32_t s_wave[4];
  const uint32_t t = threadIdx.x;
  const uint32_t ty = blockIdx.x / A.tiles_x, tx = blockIdx.x - ty * A.tiles_x;
  const int x0 = (int)(tx * RT_DILATE_TILE), y0 = (int)(ty * RT_DILATE_TILE);
  if (t < RT_DILATE_WINDOW) {
    const int wy = y0 - (int)RT_DILATE_MAX_RADIUS + (int)t;
    uint64_t m = 0ull;
    if (wy >= 0 && wy < (int)A.H) {
      const int c0 = x0 - (int)RT_DILATE_MAX_RADIUS;     // column of bit 0; may be negative
      const int k = c0 >> 6;                             // floor(c0 / 64): -1 at the left border
      const uint32_t s = (uint32_t)(c0 - k * 64);        // 0 .. 63
      const uint64_t* row = A.bitmap + (size_t)wy * A.wpr;
      const uint64_t lo = (k >= 0 && k < (int)A.wpr) ? row[k] : 0ull;
      const uint64_t hi = (k + 1 >= 0 && k + 1 < (int)A.wpr) ? row[k + 1] : 0ull;
      m = s ? (lo >> s) | (hi << (64u - s)) : lo;
    }
    win[t] = m;
  }
  __syncthreads();
  const uint32_t lx = t & (RT_DILATE_TILE - 1u), ly = t / RT_DILATE_TILE;
  const uint32_t x = (uint32_t)x0 + lx, y = (uint32_t)y0 + ly;
  const uint32_t cb = RT_DILATE_MAX_RADIUS + lx, rb = RT_DILATE_MAX_RADIUS + ly;   // this texel's bit and row of the window
  const bool inside = x < A.W && y < A.H;
  const bool covered = (win[rb] >> cb) & 1ull;
  const bool open = inside && !covered;
  uint32_t best = RT_DILATE_NONE;
  // wave-uniform: nothing to search in a wave without an uncovered texel, nor in a window without a covered one
  const bool window_empty = __ballot(win[t & 63u] != 0ull) == 0ull;
  if (__ballot(open) != 0ull && !window_empty) {
    const int R = (int)A.R;
    int best_d2 = R * R + 1;
    for (int dy = -R; dy <= R; dy++) {
      const uint64_t m = win[(int)rb + dy];              // 0 .. 63: rb is 24 .. 39 and |dy| <= 24
      if (m == 0ull) continue;
      const uint64_t left = m & ((2ull << cb) - 1ull);   // bits 0 .. cb
      const uint64_t right = m >> cb;                    // bits cb .. 63, moved down
      const int dl = left ? (int)cb - (63 - __clzll((long long)left)) : 64;
      const int dr = right ? __ffsll((unsigned long long)right) - 1 : 64;
      const int dx = dl <= dr ? -dl : dr;                // the left one wins when both are as near
      const int d2 = dx * dx + dy * dy;
      if (d2 < best_d2) {                                // <= R * R the first time, strictly smaller afterwards
        best_d2 = d2;
        best = (uint32_t)((int)y + dy) * A.W + (uint32_t)((int)x + dx);
      }
    }
  }
  const bool got = open && best != RT_DILATE_NONE;
  if (inside) A.src[(size_t)y * A.W + x] = covered ? y * A.W + x : best;
  const uint32_t sum = block_count<256>(got, s_wave);
  if (t == 0u && A.filled && sum) atomicAdd(A.filled, sum);
}

// One thread per texel.  A filled texel (a source that is not itself) receives the source's first three words bit for bit
// and w = -2.0f; nothing else is stored.  Sources are covered texels and stay as they are: in place is safe.
__global__ __launch_bounds__(256)
void k_dilate_apply(DilateArgs A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= A.W * A.H) return;
  const uint32_t s = A.src[i];
  if (s == RT_DILATE_NONE || s == i) return;
  uint4 v = reinterpret_cast<const uint4*>(A.atlas)[s];
  v.w = 0xc0000000u;   // -2.0f
  reinterpret_cast<uint4*>(A.atlas)[i] = v;
}

}  // namespace rtk
#endif
