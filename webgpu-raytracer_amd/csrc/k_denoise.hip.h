// k_denoise.hip.h — k_denoise_index and k_denoise_pass: the edge-stopped a-trous filter of a baked atlas (rt_denoise_atlas,
// mi355rt.h "atlas denoise").
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_DENOISE_HIP_H
#define MI355RT_K_DENOISE_HIP_H

namespace rtk {

//   k_denoise_index  one thread per point: atomicMin of j into the guide index map at texels[j] (the host sets the map to all
//                    ones before it), so a texel's guide is its LOWEST j whatever the order the threads run in
//   k_denoise_pass   one workgroup per tile of 32 x 8 texels: the tile's window - 2 * step texels of halo on every side, at
//                    most 48 x 24 - goes to LDS as eleven planes of one word per texel (colour 4, position 3, normal 3, guided
//                    flag; thread t the cells t, t + 256, ...), then every thread walks the 25 taps of its texel out of LDS in
//                    the order of the rule
// THE TILE.  A wave is two rows of 32 texels, and a 4-byte LDS read is served in the lane groups {0-31} and {32-63}: at any
// tap a group reads 32 CONSECUTIVE words of one window row, which lie in 32 different banks whatever the row stride - so the
// rows are packed (stride = window width) and no read of the tap walk has a bank conflict.  The window fill stores consecutive
// words per wave as well.  (Derived from the bank model, not measured.  A 16 x 16 tile puts two window rows into one lane group
// and needs a stride of 16 mod 32 to keep them apart, 48 words for a 32-wide window: 1536 cells against 1152 here.)
// THE ORDER.  The taps are a fully unrolled loop, dy outer and dx inner, and acc / wsum are chains of single f32 adds and
// multiplies in that order (the build has -ffp-contract=off), so a result word is a function of the inputs alone.
// Nothing here reads what another workgroup of the same launch wrote: a pass reads `in`, the index map and the points, and
// writes `out`, which is another array.
#define RT_DENOISE_TILE_W 32u
#define RT_DENOISE_TILE_H 8u
#define RT_DENOISE_CELLS ((RT_DENOISE_TILE_W + 4u * RT_DENOISE_MAX_STEP) * (RT_DENOISE_TILE_H + 4u * RT_DENOISE_MAX_STEP))
#define RT_DENOISE_FILL ((RT_DENOISE_CELLS + 255u) / 256u)   // cells per thread of the largest window: 5
#define RT_DENOISE_NONE 0xffffffffu
static_assert(RT_DENOISE_TILE_W * RT_DENOISE_TILE_H == 256u, "one thread per texel of the tile");
static_assert(RT_DENOISE_CELLS * 11u * 4u <= 50688u, "the LDS figure of DESIGN.md 4.1k");

struct DenoiseArgs {
  const uint4* in;          // W * H texels, row-major
  uint4* out;               // W * H texels, not `in`
  const float4* points;     // n rt_gather_point as two float4 each: {position, t_max} {normal, pad}
  const uint32_t* texels;   // n
  uint32_t* index;          // W * H: the guide index map, all ones = unguided
  uint32_t W, H, n;
  uint32_t step;            // of this pass, 1 .. RT_DENOISE_MAX_STEP
  uint32_t tiles_x;         // ceil(W / 32)
  float normal_cos, plane_eps, md2;
};

__global__ __launch_bounds__(256)
void k_denoise_index(DenoiseArgs A) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= A.n) return;
  const uint32_t i = A.texels[j];
  if (i < A.W * A.H) atomicMin(A.index + i, j);
}

// Workgroup `blockIdx.x` holds tile (blockIdx.x % tiles_x, blockIdx.x / tiles_x); thread t its texel (t % 32, t / 32).  Cell
// (wx, wy) of the window is texel (32 * tx - 2 * step + wx, 8 * ty - 2 * step + wy); a cell outside the atlas is unguided.
__global__ __launch_bounds__(256)
void k_denoise_pass(DenoiseArgs A) {
  __shared__ uint32_t s_col[4][RT_DENOISE_CELLS];
  __shared__ float s_pos[3][RT_DENOISE_CELLS];
  __shared__ float s_nrm[3][RT_DENOISE_CELLS];
  __shared__ uint32_t s_guided[RT_DENOISE_CELLS];
  const uint32_t t = threadIdx.x;
  const uint32_t ty = blockIdx.x / A.tiles_x, tx = blockIdx.x - ty * A.tiles_x;
  const int s = (int)A.step;
  const int ww = (int)RT_DENOISE_TILE_W + 4 * s, wh = (int)RT_DENOISE_TILE_H + 4 * s;
  const int x0 = (int)(tx * RT_DENOISE_TILE_W) - 2 * s, y0 = (int)(ty * RT_DENOISE_TILE_H) - 2 * s;
  // The fill, thread t the cells t, t + 256, ...: at most RT_DENOISE_FILL of them.  Three unrolled sweeps - colour and index
  // of every cell, then the points the indices name, then the LDS stores - so that a thread has all its loads of one kind in
  // flight together instead of one cell's dependent pair at a time.
  uint4 c[RT_DENOISE_FILL];
  uint32_t j[RT_DENOISE_FILL];
  float4 p[RT_DENOISE_FILL], nr[RT_DENOISE_FILL];
#pragma unroll
  for (int k = 0; k < (int)RT_DENOISE_FILL; k++) {
    const int i = (int)t + 256 * k;
    const int wy = i / ww, wx = i - wy * ww;
    const int gx = x0 + wx, gy = y0 + wy;
    c[k] = make_uint4(0u, 0u, 0u, 0u);
    j[k] = RT_DENOISE_NONE;
    if (i < ww * wh && gx >= 0 && gy >= 0 && gx < (int)A.W && gy < (int)A.H) {
      const size_t gi = (size_t)gy * A.W + (size_t)gx;
      c[k] = A.in[gi];
      j[k] = A.index[gi];
    }
  }
#pragma unroll
  for (int k = 0; k < (int)RT_DENOISE_FILL; k++) {
    p[k] = nr[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (j[k] != RT_DENOISE_NONE) {
      p[k] = A.points[2u * (size_t)j[k]];
      nr[k] = A.points[2u * (size_t)j[k] + 1u];
    }
  }
#pragma unroll
  for (int k = 0; k < (int)RT_DENOISE_FILL; k++) {
    const int i = (int)t + 256 * k;
    if (i < ww * wh) {
      s_col[0][i] = c[k].x; s_col[1][i] = c[k].y; s_col[2][i] = c[k].z; s_col[3][i] = c[k].w;
      s_pos[0][i] = p[k].x; s_pos[1][i] = p[k].y; s_pos[2][i] = p[k].z;
      s_nrm[0][i] = nr[k].x; s_nrm[1][i] = nr[k].y; s_nrm[2][i] = nr[k].z;
      s_guided[i] = j[k] != RT_DENOISE_NONE ? 1u : 0u;
    }
  }
  __syncthreads();
  const uint32_t lx = t & (RT_DENOISE_TILE_W - 1u), ly = t / RT_DENOISE_TILE_W;
  const uint32_t x = tx * RT_DENOISE_TILE_W + lx, y = ty * RT_DENOISE_TILE_H + ly;
  const bool inside = x < A.W && y < A.H;
  const int cc = ((int)ly + 2 * s) * ww + (int)lx + 2 * s;   // this texel's cell
  const bool guided = inside && s_guided[cc] != 0u;
  uint4 res = make_uint4(s_col[0][cc], s_col[1][cc], s_col[2][cc], s_col[3][cc]);   // an unguided texel: copied bit for bit
  // wave-uniform: a wave without a guided texel has no taps to walk
  if (__ballot(guided) != 0ull) {
    if (guided) {
      const float kw[3] = {0.375f, 0.25f, 0.0625f};
      const float Px = s_pos[0][cc], Py = s_pos[1][cc], Pz = s_pos[2][cc];
      const float Nx = s_nrm[0][cc], Ny = s_nrm[1][cc], Nz = s_nrm[2][cc];
      float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f, wsum = 0.0f;
#pragma unroll
      for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
          const float h = kw[dx < 0 ? -dx : dx] * kw[dy < 0 ? -dy : dy];
          const int q = cc + (dy * ww + dx) * s;   // inside the window: the halo is 2 * s cells
          bool ok = dx == 0 && dy == 0;
          if (!ok && s_guided[q] != 0u) {
            const float Qx = s_nrm[0][q], Qy = s_nrm[1][q], Qz = s_nrm[2][q];
            const float ex = s_pos[0][q] - Px, ey = s_pos[1][q] - Py, ez = s_pos[2][q] - Pz;
            const float nd = (Nx * Qx + Ny * Qy) + Nz * Qz;
            const float pl = (Nx * ex + Ny * ey) + Nz * ez;
            const float d2 = (ex * ex + ey * ey) + ez * ez;
            ok = nd >= A.normal_cos && __builtin_fabsf(pl) <= A.plane_eps && d2 <= A.md2;   // a NaN fails each
          }
          if (ok) {
            a0 = a0 + h * __uint_as_float(s_col[0][q]);
            a1 = a1 + h * __uint_as_float(s_col[1][q]);
            a2 = a2 + h * __uint_as_float(s_col[2][q]);
            a3 = a3 + h * __uint_as_float(s_col[3][q]);
            wsum = wsum + h;
          }
        }
      }
      res = make_uint4(__float_as_uint(rt_div(a0, wsum)), __float_as_uint(rt_div(a1, wsum)), __float_as_uint(rt_div(a2, wsum)),
                       __float_as_uint(rt_div(a3, wsum)));
    }
  }
  if (inside) A.out[(size_t)y * A.W + x] = res;
}

}  // namespace rtk
#endif
