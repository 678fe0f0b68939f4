// k_frame_denoise.hip.h — k_frame_prepare, k_frame_pass_lds, k_frame_pass_direct and k_frame_finish: the G-buffer-guided
// a-trous filter of a frame (rt_denoise_frame, mi355rt.h "THE FRAME DENOISE RULE").
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_FRAME_DENOISE_HIP_H
#define MI355RT_K_FRAME_DENOISE_HIP_H

namespace rtk {

//   k_frame_prepare      one thread per pixel: radiance (get_radiance of the post pass) and the G-buffer of the frame ->
//                        colour texel {filtered quantity rgb, luminance variance}, guide texel (two float4: {P.xyz, bits(inst)}
//                        {N.xyz, bits(surface flag)}) and modulation texel {m.rgb, alpha}
//   k_frame_pass_lds<S>  one workgroup per tile of 32 x 8 pixels: the tile's window (2 * S pixels of halo on every side) goes
//                        to LDS as twelve planes of one word per pixel, then every thread walks its 25 taps out of LDS.
//                        One instantiation per spacing S = 1 .. 4, so the LDS a workgroup takes is that of ITS window:
//                        (32 + 4 S) * (8 + 4 S) * 48 bytes = 20 736 / 30 720 / 42 240 / 55 296
//   k_frame_pass_direct  one thread per pixel, the taps read through the vector L1 and L2 with no staging: every spacing.  The
//                        fifteen loads of a row of taps are issued before the first is used
//   k_frame_finish       one thread per pixel: colour times modulation, alpha in the fourth word
// THE GUIDE IS 32 BYTES, the unit normal as three f32: a 16-byte guide {P.xyz, two snorm16} would halve the tap bytes of the
// direct form, but every tap would then decode - rt_normalize: a square root, a division and seven more operations - 25 times
// per pixel and pass, and the instance word and the surface flag would need a plane of their own; the L2 form is paid in bytes
// instead, and the LDS form decodes nothing either.  (The 16-byte form was not built or timed.)
// THE TILE of the LDS form is k_denoise_pass's, with its derivation: a wave is two rows of 32 pixels, a 4-byte LDS read is
// served in the lane groups {0-31} and {32-63}, and at any tap a group reads 32 CONSECUTIVE words of one window row, which lie
// in 32 different banks whatever the row stride: the derived conflict count of the tap walk is 0; the fill stores consecutive
// words per wave as well.  (Derived from the bank model, not measured.)  There is no index indirection here: the guide of a
// pixel is at the pixel's own index.
// THE ORDER.  The taps are a fully unrolled loop, dy outer and dx inner, and every sum is a chain of single f32 operations in
// that order (the build has -ffp-contract=off); both forms run the SAME tap function on the same words, so a result word is a
// function of the inputs alone.  No atomics, no cross-lane sums.  A pass reads `in` and the guides and writes `out`, another
// array.
#define RT_FRAME_TILE_W 32u
#define RT_FRAME_TILE_H 8u
#define RT_FRAME_LDS_MAX_STEP 4u
#define RT_FRAME_PLANES 12u
static_assert(RT_FRAME_TILE_W * RT_FRAME_TILE_H == 256u, "one thread per pixel of the tile");

struct FramePrepareArgs {
  const float4* accum;        // W * H
  const uint32_t* albedo;     // the G-buffer of the frame: unorm8 albedo, alpha byte 0 = background
  const float4* normal_id;    // {oct.x, oct.y, bits(tri), bits(inst)}
  const float* depth;
  float4* col;                // out: {q.rgb, var}
  float4* guide;              // out: 2 per pixel
  float4* mod;                // out: {m.rgb, alpha}
  uint32_t flags;
};

struct FramePassArgs {
  const float4* in;           // W * H colour texels
  float4* out;                // not `in`
  const float4* guide;        // 2 per pixel
  uint32_t W, H;
  uint32_t step;
  uint32_t tiles_x;           // ceil(W / 32), LDS form
  uint32_t flags;
  float normal_cos, plane_eps, sigma_lum;
};

__device__ __forceinline__ float fd_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__device__ __forceinline__ rt3 fd_radiance(const float4* accum, uint32_t W, uint32_t H, int cx, int cy) {
  const int x = cx < 0 ? 0 : (cx > (int)W - 1 ? (int)W - 1 : cx);
  const int y = cy < 0 ? 0 : (cy > (int)H - 1 ? (int)H - 1 : cy);
  const float4 a = accum[(size_t)y * W + (size_t)x];
  if (a.w <= 0.0f) return rt3_splat(0.0f);
  return rt_div3_plain(rt3_make(a.x, a.y, a.z), a.w);
}
// the factor the filtered quantity is divided by, and multiplied back with: 1 without the flag and on the background
__device__ __forceinline__ rt3 fd_modulation(uint32_t albedo, uint32_t flags) {
  if (!(flags & RT_FRAME_DENOISE_DEMODULATE) || (albedo >> 24) == 0u) return rt3_splat(1.0f);
  return rt3_make(rt_max(rt_from_unorm8(albedo & 255u), RT_FRAME_DENOISE_MIN_ALBEDO),
                  rt_max(rt_from_unorm8((albedo >> 8) & 255u), RT_FRAME_DENOISE_MIN_ALBEDO),
                  rt_max(rt_from_unorm8((albedo >> 16) & 255u), RT_FRAME_DENOISE_MIN_ALBEDO));
}
__device__ __forceinline__ rt3 fd_quantity(const FramePrepareArgs& A, uint32_t W, uint32_t H, int cx, int cy) {
  const int x = cx < 0 ? 0 : (cx > (int)W - 1 ? (int)W - 1 : cx);
  const int y = cy < 0 ? 0 : (cy > (int)H - 1 ? (int)H - 1 : cy);
  const rt3 rad = fd_radiance(A.accum, W, H, x, y);
  const rt3 m = fd_modulation(A.albedo[(size_t)y * W + (size_t)x], A.flags);
  return rt3_make(rt_div(rad.x, m.x), rt_div(rad.y, m.y), rt_div(rad.z, m.z));
}

__global__ __launch_bounds__(256) void k_frame_prepare(FramePrepareArgs A, rt_scene_uniforms U) {
  const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y;
  const uint32_t W = U.width, H = U.height;
  if (x >= W || y >= H) return;
  const size_t i = (size_t)y * W + x;
  const float4 a = A.accum[i];
  const uint32_t alb = A.albedo[i];
  const bool surface = (alb >> 24) != 0u;
  const rt3 m = fd_modulation(alb, A.flags);
  const rt3 q = fd_quantity(A, W, H, (int)x, (int)y);
  float m1 = 0.0f, m2 = 0.0f;
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      const rt3 n = fd_quantity(A, W, H, (int)x + dx, (int)y + dy);
      const float l = fd_lum(n.x, n.y, n.z);
      m1 = m1 + l;
      m2 = m2 + l * l;
    }
  const float mean = rt_div(m1, 9.0f);
  const float var = rt_max(rt_div(m2, 9.0f) - mean * mean, 0.0f);
  A.col[i] = make_float4(q.x, q.y, q.z, var);
  A.mod[i] = make_float4(m.x, m.y, m.z, a.w > 0.0f ? 1.0f : 0.0f);
  float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0;
  if (surface) {
    const float4 nid = A.normal_id[i];
    const rt3 N = unpack_normal(nid.x, nid.y);
    // the inverse of k_primary_visibility's depth: z_view from the clip depth, the hit distance along the pixel's own ray
    const rt3 eye = rt3_make(U.camera.origin[0], U.camera.origin[1], U.camera.origin[2]);
    const rt3 ll = rt3_make(U.camera.lower_left[0], U.camera.lower_left[1], U.camera.lower_left[2]);
    const rt3 hor = rt3_make(U.camera.horizontal[0], U.camera.horizontal[1], U.camera.horizontal[2]);
    const rt3 ver = rt3_make(U.camera.vertical[0], U.camera.vertical[1], U.camera.vertical[2]);
    const rt3 center = ll + hor * 0.5f + ver * 0.5f;
    const float focal_length = rt_length(center - eye);
    const float z_near = 0.001f, z_far = 10000.0f;
    const float u = ((float)x + 0.5f + U.jitter[0] * (float)W) / (float)W;
    const float v = 1.0f - ((float)y + 0.5f + U.jitter[1] * (float)H) / (float)H;
    const rt3 d = ll + u * hor + v * ver - eye;
    const float ca = z_far / (z_far - z_near), cb = (z_far * z_near) / (z_far - z_near);
    const float z_view = rt_div(cb, ca - A.depth[i]);
    const float t = rt_div(z_view, focal_length);
    g0 = make_float4(eye.x + d.x * t, eye.y + d.y * t, eye.z + d.z * t, nid.w);
    g1 = make_float4(N.x, N.y, N.z, rt_u2f(1u));
  }
  A.guide[2 * i] = g0;
  A.guide[2 * i + 1] = g1;
}

// What a pixel carries through its tap walk, and one tap of the rule: the SAME function in both forms.
struct FdCentre {
  float Px, Py, Pz, Nx, Ny, Nz, lum, den;
  uint32_t inst;
};
struct FdSums {
  float a0, a1, a2, av, wsum;
};
__device__ __forceinline__ void fd_tap(const FramePassArgs& A, const FdCentre& C, FdSums& S, bool centre, bool inside, float h,
                                       float cr, float cg, float cb, float cv, float Qx, float Qy, float Qz, uint32_t qinst,
                                       float Mx, float My, float Mz, uint32_t qflag) {
  bool ok = centre;
  if (!ok && inside && qflag != 0u && (!(A.flags & RT_FRAME_DENOISE_SAME_INSTANCE) || qinst == C.inst)) {
    const float ex = Qx - C.Px, ey = Qy - C.Py, ez = Qz - C.Pz;
    const float nd = (C.Nx * Mx + C.Ny * My) + C.Nz * Mz;
    const float pl = (C.Nx * ex + C.Ny * ey) + C.Nz * ez;
    ok = nd >= A.normal_cos && rt_abs(pl) <= A.plane_eps;   // a NaN fails each
  }
  if (ok) {
    float w = h;
    if (A.sigma_lum > 0.0f) w = h * rt_exp(rt_div(-rt_abs(fd_lum(cr, cg, cb) - C.lum), C.den));
    S.a0 = S.a0 + w * cr;
    S.a1 = S.a1 + w * cg;
    S.a2 = S.a2 + w * cb;
    S.av = S.av + (w * w) * cv;
    S.wsum = S.wsum + w;
  }
}
__device__ __forceinline__ FdCentre fd_centre(const FramePassArgs& A, float4 c, float4 g0, float4 g1) {
  FdCentre C;
  C.Px = g0.x; C.Py = g0.y; C.Pz = g0.z;
  C.Nx = g1.x; C.Ny = g1.y; C.Nz = g1.z;
  C.inst = rt_f2u(g0.w);
  C.lum = fd_lum(c.x, c.y, c.z);
  C.den = A.sigma_lum * rt_sqrt(c.w) + 1e-4f;
  return C;
}
__device__ __forceinline__ float4 fd_result(const FdSums& S) {
  return make_float4(rt_div(S.a0, S.wsum), rt_div(S.a1, S.wsum), rt_div(S.a2, S.wsum), rt_div(S.av, S.wsum * S.wsum));
}

// Thread (blockIdx.x * 256 + threadIdx.x, blockIdx.y) holds one pixel; a tap outside the image is loaded from the pixel's own
// (valid) address and not used.
__global__ __launch_bounds__(256) void k_frame_pass_direct(FramePassArgs A) {
  const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y;
  if (x >= A.W || y >= A.H) return;
  const size_t i = (size_t)y * A.W + x;
  const float4 c = A.in[i];
  const float4 g0 = A.guide[2 * i], g1 = A.guide[2 * i + 1];
  if (rt_f2u(g1.w) == 0u) {   // background: copied bit for bit
    A.out[i] = c;
    return;
  }
  const FdCentre C = fd_centre(A, c, g0, g1);
  FdSums S = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const float kw[3] = {0.375f, 0.25f, 0.0625f};
  const int s = (int)A.step;
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    float4 tc[5], t0[5], t1[5];
    bool in_img[5];
    const int qy = (int)y + dy * s;
#pragma unroll
    for (int k = 0; k < 5; k++) {   // the loads of the row, all in flight before the first is used
      const int qx = (int)x + (k - 2) * s;
      in_img[k] = qx >= 0 && qy >= 0 && qx < (int)A.W && qy < (int)A.H;
      const size_t q = in_img[k] ? (size_t)qy * A.W + (size_t)qx : i;
      tc[k] = A.in[q];
      t0[k] = A.guide[2 * q];
      t1[k] = A.guide[2 * q + 1];
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
      const int dx = k - 2;
      const float h = kw[dx < 0 ? -dx : dx] * kw[dy < 0 ? -dy : dy];
      fd_tap(A, C, S, dx == 0 && dy == 0, in_img[k], h, tc[k].x, tc[k].y, tc[k].z, tc[k].w, t0[k].x, t0[k].y, t0[k].z,
             rt_f2u(t0[k].w), t1[k].x, t1[k].y, t1[k].z, rt_f2u(t1[k].w));
    }
  }
  A.out[i] = fd_result(S);
}

// Workgroup `blockIdx.x` holds tile (blockIdx.x % tiles_x, blockIdx.x / tiles_x); thread t its pixel (t % 32, t / 32).  Cell
// (wx, wy) of the window is pixel (32 * tx - 2 * S + wx, 8 * ty - 2 * S + wy); a cell outside the image has surface flag 0.
template <int S_>
__global__ __launch_bounds__(256) void k_frame_pass_lds(FramePassArgs A) {
  constexpr int WW = (int)RT_FRAME_TILE_W + 4 * S_, WH = (int)RT_FRAME_TILE_H + 4 * S_, CELLS = WW * WH;
  constexpr int FILL = (CELLS + 255) / 256;
  static_assert(S_ >= 1 && S_ <= (int)RT_FRAME_LDS_MAX_STEP, "the window of this spacing fits LDS");
  __shared__ float s_w[RT_FRAME_PLANES][CELLS];   // colour 4, position 3, instance, normal 3, surface flag
  const uint32_t t = threadIdx.x;
  const uint32_t ty = blockIdx.x / A.tiles_x, tx = blockIdx.x - ty * A.tiles_x;
  const int x0 = (int)(tx * RT_FRAME_TILE_W) - 2 * S_, y0 = (int)(ty * RT_FRAME_TILE_H) - 2 * S_;
  // the fill, thread t the cells t, t + 256, ...: two unrolled sweeps, so that a thread has all its loads in flight together
  float4 c[FILL], g0[FILL], g1[FILL];
#pragma unroll
  for (int k = 0; k < FILL; k++) {
    const int i = (int)t + 256 * k;
    const int wy = i / WW, wx = i - wy * WW;
    const int gx = x0 + wx, gy = y0 + wy;
    c[k] = g0[k] = g1[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i < CELLS && gx >= 0 && gy >= 0 && gx < (int)A.W && gy < (int)A.H) {
      const size_t gi = (size_t)gy * A.W + (size_t)gx;
      c[k] = A.in[gi];
      g0[k] = A.guide[2 * gi];
      g1[k] = A.guide[2 * gi + 1];
    }
  }
#pragma unroll
  for (int k = 0; k < FILL; k++) {
    const int i = (int)t + 256 * k;
    if (i < CELLS) {
      s_w[0][i] = c[k].x; s_w[1][i] = c[k].y; s_w[2][i] = c[k].z; s_w[3][i] = c[k].w;
      s_w[4][i] = g0[k].x; s_w[5][i] = g0[k].y; s_w[6][i] = g0[k].z; s_w[7][i] = g0[k].w;
      s_w[8][i] = g1[k].x; s_w[9][i] = g1[k].y; s_w[10][i] = g1[k].z; s_w[11][i] = g1[k].w;
    }
  }
  __syncthreads();
  const uint32_t lx = t & (RT_FRAME_TILE_W - 1u), ly = t / RT_FRAME_TILE_W;
  const uint32_t x = tx * RT_FRAME_TILE_W + lx, y = ty * RT_FRAME_TILE_H + ly;
  if (x >= A.W || y >= A.H) return;
  const int cc = ((int)ly + 2 * S_) * WW + (int)lx + 2 * S_;   // this pixel's cell
  const float4 cen = make_float4(s_w[0][cc], s_w[1][cc], s_w[2][cc], s_w[3][cc]);
  float4 res = cen;   // background: copied bit for bit
  if (rt_f2u(s_w[11][cc]) != 0u) {
    const FdCentre C = fd_centre(A, cen, make_float4(s_w[4][cc], s_w[5][cc], s_w[6][cc], s_w[7][cc]),
                                 make_float4(s_w[8][cc], s_w[9][cc], s_w[10][cc], s_w[11][cc]));
    FdSums S = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const float kw[3] = {0.375f, 0.25f, 0.0625f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
      for (int dx = -2; dx <= 2; dx++) {
        const float h = kw[dx < 0 ? -dx : dx] * kw[dy < 0 ? -dy : dy];
        const int q = cc + (dy * WW + dx) * S_;   // inside the window: the halo is 2 * S cells
        // a cell outside the image holds surface flag 0, which refuses it like `inside` would
        fd_tap(A, C, S, dx == 0 && dy == 0, true, h, s_w[0][q], s_w[1][q], s_w[2][q], s_w[3][q], s_w[4][q], s_w[5][q],
               s_w[6][q], rt_f2u(s_w[7][q]), s_w[8][q], s_w[9][q], s_w[10][q], rt_f2u(s_w[11][q]));
      }
    }
    res = fd_result(S);
  }
  A.out[(size_t)y * A.W + x] = res;
}

// out = {col.rgb * m.rgb, alpha}: the remodulation, and the accumulator's format (present() reads rgb / a with a in {0, 1}).
__global__ __launch_bounds__(256) void k_frame_finish(const float4* __restrict__ col, const float4* __restrict__ mod,
                                                      float4* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float4 c = col[i], m = mod[i];
  out[i] = make_float4(c.x * m.x, c.y * m.y, c.z * m.z, m.w);
}

}  // namespace rtk
#endif
