// k_frame_temporal.hip.h — k_frame_temporal: the temporal stage of the frame denoiser (rt_set_frame_temporal, mi355rt.h "THE
// FRAME TEMPORAL RULE"): last frame's history, gathered at this frame's pixels, blended with this frame's colour.
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_FRAME_TEMPORAL_HIP_H
#define MI355RT_K_FRAME_TEMPORAL_HIP_H

namespace rtk {

//   k_frame_temporal     one thread per pixel, between k_frame_prepare and the first pass: the pixel's world position goes
//                        through the PREVIOUS frame's pinhole to a bilinear footprint of four pixels of the previous history,
//                        every tap tested against the previous guide; the blend goes to the integrated image (the input of pass
//                        0), the next history and the next moments.
// THE BYTES.  A pixel reads its own colour texel and guide (16 + 32 B), four taps of previous guide, history and moments (32 +
// 16 + 8 B each) and writes 16 + 16 + 8 B: 312 B in nineteen wave-level loads, three of its own and sixteen of the taps, and
// three stores.
// THE LOADS of the four taps, sixteen of 16 bytes or fewer, are issued before the first is used (the direct
// forms pay per wave-level load instruction, about 33 CU cycles, whatever the lines); a tap that is outside the image or has no
// weight loads the pixel's own (valid) address and is not used.  Neighbouring pixels reproject to neighbouring addresses, so the
// taps come out of L1 / L2.  No LDS, no atomics, no cross-lane operation: a result word is a function of the inputs alone.
// THE ORDER is the rule's, every sum a chain of single f32 operations (the build has -ffp-contract=off).
struct FrameTemporalArgs {
  const float4* col;          // this frame's colour texels {q.rgb, var}, from k_frame_prepare
  const float4* guide;        // this frame's guide, 2 per pixel (the next set's)
  const float4* prev_hist;    // the previous set: history {q.rgb, (float)n}, moments {m1, m2}, guide
  const float2* prev_mom;
  const float4* prev_guide;
  float4* integ;              // out: {q'.rgb, var'}
  float4* hist;               // out: the next set
  float2* mom;
  uint32_t W, H;
  uint32_t flags;
  uint32_t have;              // 0: no history is kept (the first frame, or after a drop): the previous set is not read
  float max_history, var_history;   // the descriptor's words as f32
  float normal_cos, plane_eps;
  float eye[3], ll[3], hor[3], ver[3], jit[2];   // the previous frame's pinhole and jitter
};

__device__ __forceinline__ float ft_dot(rt3 a, rt3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// The stage's body.  MOTION false: the rule as it stands (k_frame_temporal).  MOTION true (k_frame_temporal_motion, mi355rt.h
// "THE FRAME MOTION RULE"): P, N and the pixel's stable id come from the carry plane k_frame_motion wrote, an UNTRACKED pixel
// has no history, and SAME_INSTANCE compares the id the previous frame recorded for the tap - four more 4-byte loads, issued
// with the sixteen of the footprint.
template <bool MOTION>
__device__ __forceinline__ void frame_temporal_body(const FrameTemporalArgs A, const float4* carry, const uint32_t* prev_id) {
  const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y;
  if (x >= A.W || y >= A.H) return;
  const size_t i = (size_t)y * A.W + x;
  const float4 c = A.col[i];
  const float4 g0 = A.guide[2 * i], g1 = A.guide[2 * i + 1];
  if (rt_f2u(g1.w) == 0u) {   // background
    A.integ[i] = c;
    A.hist[i] = make_float4(c.x, c.y, c.z, 0.0f);
    A.mom[i] = make_float2(0.0f, 0.0f);
    return;
  }
  const float l = fd_lum(c.x, c.y, c.z);
  float wsum = 0.0f, a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, s1 = 0.0f, s2 = 0.0f, n_prev = 0.0f;
  bool any = false;
  float4 k0 = g0, k1 = g1;   // {P, -} {N, -}: the guide's, or the carry's {P', status} {N', sid}
  bool tracked = true;
  if constexpr (MOTION) {
    k0 = carry[2 * i];
    k1 = carry[2 * i + 1];
    tracked = rt_f2u(k0.w) != RT_FRAME_MOTION_UNTRACKED;
  }
  if (A.have != 0u && A.max_history > 1.0f && tracked) {
    const rt3 P = rt3_make(k0.x, k0.y, k0.z), N = rt3_make(k1.x, k1.y, k1.z);
    const rt3 eye = rt3_make(A.eye[0], A.eye[1], A.eye[2]), ll = rt3_make(A.ll[0], A.ll[1], A.ll[2]);
    const rt3 hor = rt3_make(A.hor[0], A.hor[1], A.hor[2]), ver = rt3_make(A.ver[0], A.ver[1], A.ver[2]);
    const rt3 e = P - eye, c0 = ll - eye;
    const rt3 nrm = rt3_make(hor.y * ver.z - hor.z * ver.y, hor.z * ver.x - hor.x * ver.z, hor.x * ver.y - hor.y * ver.x);
    const float s = rt_div(ft_dot(c0, nrm), ft_dot(e, nrm));
    const rt3 r = e * s - c0;
    const float u = rt_div(ft_dot(r, hor), ft_dot(hor, hor)), v = rt_div(ft_dot(r, ver), ft_dot(ver, ver));
    const float Wf = (float)A.W, Hf = (float)A.H;
    const float fx = (u * Wf - 0.5f) - A.jit[0] * Wf, fy = ((1.0f - v) * Hf - 0.5f) - A.jit[1] * Hf;
    if (s > 0.0f && fx >= -1.0f && fx < Wf && fy >= -1.0f && fy < Hf) {   // a NaN fails each
      const float flx = rt_floor(fx), fly = rt_floor(fy);
      const int x0 = (int)flx, y0 = (int)fly;
      const float tx = fx - flx, ty = fy - fly;
      const float w[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
      float4 t0[4], t1[4], th[4];
      float2 tm[4];
      uint32_t tid[4] = {0u, 0u, 0u, 0u};
      bool use[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {   // the loads of the footprint, all in flight before the first is used
        const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
        use[k] = w[k] > 0.0f && qx >= 0 && qy >= 0 && qx < (int)A.W && qy < (int)A.H;
        const size_t q = use[k] ? (size_t)qy * A.W + (size_t)qx : i;
        t0[k] = A.prev_guide[2 * q];
        t1[k] = A.prev_guide[2 * q + 1];
        th[k] = A.prev_hist[q];
        tm[k] = A.prev_mom[q];
        if constexpr (MOTION) tid[k] = prev_id[q];
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        // the tap's instance is the pixel's: by stable id, else by the guides' TLAS positions
        bool ok = use[k] && rt_f2u(t1[k].w) != 0u && th[k].w >= 1.0f &&
                  (!(A.flags & RT_FRAME_TEMPORAL_SAME_INSTANCE) || (MOTION ? tid[k] : rt_f2u(t0[k].w)) == rt_f2u(MOTION ? k1.w : g0.w));
        if (ok) {
          const rt3 d = rt3_make(t0[k].x - P.x, t0[k].y - P.y, t0[k].z - P.z);
          const float nd = ft_dot(N, rt3_make(t1[k].x, t1[k].y, t1[k].z));
          const float pl = ft_dot(N, d);
          ok = nd >= A.normal_cos && rt_abs(pl) <= A.plane_eps;   // a NaN fails each
        }
        if (ok) {
          wsum = wsum + w[k];
          a0 = a0 + w[k] * th[k].x;
          a1 = a1 + w[k] * th[k].y;
          a2 = a2 + w[k] * th[k].z;
          s1 = s1 + w[k] * tm[k].x;
          s2 = s2 + w[k] * tm[k].y;
          if (!any || th[k].w < n_prev) n_prev = th[k].w;
          any = true;
        }
      }
    }
  }
  if (!any) {   // no history
    A.integ[i] = c;
    A.hist[i] = make_float4(c.x, c.y, c.z, 1.0f);
    A.mom[i] = make_float2(l, l * l);
    return;
  }
  const float hq0 = rt_div(a0, wsum), hq1 = rt_div(a1, wsum), hq2 = rt_div(a2, wsum);
  const float hm1 = rt_div(s1, wsum), hm2 = rt_div(s2, wsum);
  float n = n_prev + 1.0f;
  if (!(n < A.max_history)) n = A.max_history;
  const float a = rt_div(1.0f, n);
  const float q0 = hq0 + a * (c.x - hq0), q1 = hq1 + a * (c.y - hq1), q2 = hq2 + a * (c.z - hq2);
  const float m1 = hm1 + a * (l - hm1), m2 = hm2 + a * (l * l - hm2);
  const float var = n >= A.var_history ? rt_max(m2 - m1 * m1, 0.0f) : c.w;
  A.integ[i] = make_float4(q0, q1, q2, var);
  A.hist[i] = make_float4(q0, q1, q2, n);
  A.mom[i] = make_float2(m1, m2);
}

__global__ __launch_bounds__(256) void k_frame_temporal(FrameTemporalArgs A) { frame_temporal_body<false>(A, nullptr, nullptr); }
__global__ __launch_bounds__(256) void k_frame_temporal_motion(FrameTemporalArgs A, const float4* carry, const uint32_t* prev_id) {
  frame_temporal_body<true>(A, carry, prev_id);
}

}  // namespace rtk
#endif
