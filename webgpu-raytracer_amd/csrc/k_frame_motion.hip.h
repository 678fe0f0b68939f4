// k_frame_motion.hip.h — k_frame_motion and k_frame_motion_scatter: the motion stage of the frame denoiser's temporal stage
// (RT_FRAME_TEMPORAL_MOTION, mi355rt.h "THE FRAME MOTION RULE"): where the pixel's own surface point was in the previous frame.
// Part of the kernel set of csrc/kernels.hip.h (included from there, in order; not a stand-alone header).
#ifndef MI355RT_K_FRAME_MOTION_HIP_H
#define MI355RT_K_FRAME_MOTION_HIP_H

namespace rtk {

//   k_frame_motion          one thread per pixel, the grid of k_frame_prepare, between it and k_frame_temporal_motion: the
//                           pixel's triangle in this frame and in the snapshot of the previous one, the point's barycentrics in
//                           the first, the same point of the second -> the carry texel {P', status} {N', sid} and the id plane
//   k_frame_motion_scatter  one thread per instance, after the temporal stage: the forward transform of the instance at TLAS
//                           position p goes to row ids[p] of the snapshot
// THE BYTES.  A pixel reads its normal_id texel and guide (16 + 32 B), the first 16 B of its topology row, its id (4 B), two
// transforms (64 + 64 B) and six vertices (6 x 16 B) and writes 32 + 4 B: 328 B in eighteen wave-level loads and three stores.
// THE LOADS come in three dependent rounds - (1) normal_id and guide; (2) topology row, id, this frame's transform; (3) the six
// vertices and the snapshot's transform, whose row is the id - and every load of a round is issued before the first is used
// (the direct forms pay per wave-level load instruction, whatever the lines).  Every index is compared with
// its array's count before the load it guards, and a lane whose index fails makes no load at all (the load sits under the
// lane's execution mask): no address is ever formed from a bad index, and an empty array is never read.
// THE TRANSFORMS ARE NEARLY WAVE-UNIFORM: the 64 pixels of a wave mostly lie on one instance, so the eight 16-byte transform
// loads of a wave touch one 64-byte line each time and coalesce to one L1 request per instruction; the topology row and the
// vertices of neighbouring pixels are those of one or two triangles likewise.  They cannot be scalar loads - the instance is a
// per-lane value - so what uniformity buys is lines, not instructions: the kernel is bound by its eighteen load instructions.
// No LDS, no atomics, no cross-lane operation: a result word is a function of the inputs alone.
// THE ORDER is the rule's, every sum a chain of single f32 operations (the build has -ffp-contract=off).
struct FrameMotionArgs {
  const float4* normal_id;    // the G-buffer plane of the frame: {oct.x, oct.y, bits(tri), bits(inst)}
  const float4* guide;        // this frame's guide, 2 per pixel
  const float4* topo;         // 5 per triangle; the first is {v0, v1, v2, geometry} as words
  const float4* pos;          // 1 per vertex
  const float4* inst;         // 9 per instance, TLAS order; the first four are the forward transform's columns
  const uint32_t* ids;        // stable id per TLAS position, or nullptr: the identity
  const float4* snap_pos;     // the snapshot: 1 per vertex ...
  const float4* snap_xf;      // ... 4 per stable id
  float4* carry;              // out: 2 per pixel
  uint32_t* pix_id;           // out: the id plane of this frame
  uint32_t W, H;
  uint32_t n_tris, n_verts, n_inst;
  uint32_t have;              // 0: no snapshot is kept: the snapshot arrays are not read
};

__device__ __forceinline__ bool fm_finite(float x) { return (rt_f2u(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ rt3 fm_point(float4 c0, float4 c1, float4 c2, float4 c3, float4 v) {
  const float m[16] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
  return rt_mat_mul_point(m, rt3_make(v.x, v.y, v.z));
}
__device__ __forceinline__ bool fm_same(rt3 a, rt3 b) {
  return rt_f2u(a.x) == rt_f2u(b.x) && rt_f2u(a.y) == rt_f2u(b.y) && rt_f2u(a.z) == rt_f2u(b.z);
}

__global__ __launch_bounds__(256) void k_frame_motion(FrameMotionArgs A) {
  const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y;
  if (x >= A.W || y >= A.H) return;
  const size_t i = (size_t)y * A.W + x;
  // round 1
  const float4 nid = A.normal_id[i];
  const float4 g0 = A.guide[2 * i], g1 = A.guide[2 * i + 1];
  if (rt_f2u(g1.w) == 0u) {   // background
    A.carry[2 * i] = make_float4(0.0f, 0.0f, 0.0f, rt_u2f(RT_FRAME_MOTION_BACKGROUND));
    A.carry[2 * i + 1] = make_float4(0.0f, 0.0f, 0.0f, rt_u2f(RT_FRAME_MOTION_NO_ID));
    A.pix_id[i] = RT_FRAME_MOTION_NO_ID;
    return;
  }
  const uint32_t tri = rt_f2u(nid.z), inst = rt_f2u(nid.w);
  const bool tri_ok = tri < A.n_tris, inst_ok = inst < A.n_inst;
  // round 2: a lane that fails a check loads nothing
  float4 row = make_float4(0.0f, 0.0f, 0.0f, 0.0f), m0 = row, m1 = row, m2 = row, m3 = row;
  uint32_t sid = RT_FRAME_MOTION_NO_ID;
  if (tri_ok) row = A.topo[5 * (size_t)tri];
  if (inst_ok) {
    const float4* I = A.inst + 9 * (size_t)inst;
    if (A.ids) sid = A.ids[inst];
    m0 = I[0];
    m1 = I[1];
    m2 = I[2];
    m3 = I[3];
    if (!A.ids) sid = inst;
    if (sid >= A.n_inst) sid = RT_FRAME_MOTION_NO_ID;
  }
  const uint32_t v0 = rt_f2u(row.x), v1 = rt_f2u(row.y), v2 = rt_f2u(row.z);
  const bool tracked = A.have != 0u && tri_ok && inst_ok && sid != RT_FRAME_MOTION_NO_ID && v0 < A.n_verts && v1 < A.n_verts &&
                       v2 < A.n_verts;
  A.pix_id[i] = sid;
  uint32_t status = RT_FRAME_MOTION_UNTRACKED;
  rt3 Pc = rt3_make(g0.x, g0.y, g0.z), Nc = rt3_make(g1.x, g1.y, g1.z);
  if (tracked) {
    // round 3
    const float4 p0 = A.pos[v0], p1 = A.pos[v1], p2 = A.pos[v2];
    const float4 q0 = A.snap_pos[v0], q1 = A.snap_pos[v1], q2 = A.snap_pos[v2];
    const float4* X = A.snap_xf + 4 * (size_t)sid;
    const float4 s0 = X[0], s1 = X[1], s2 = X[2], s3 = X[3];
    const rt3 a = fm_point(m0, m1, m2, m3, p0), b = fm_point(m0, m1, m2, m3, p1), c = fm_point(m0, m1, m2, m3, p2);
    const rt3 ap = fm_point(s0, s1, s2, s3, q0), bp = fm_point(s0, s1, s2, s3, q1), cp = fm_point(s0, s1, s2, s3, q2);
    if (fm_same(a, ap) && fm_same(b, bp) && fm_same(c, cp)) {
      status = RT_FRAME_MOTION_UNMOVED;
    } else {
      const rt3 e1 = b - a, e2 = c - a, ep = Pc - a;
      const float d11 = ft_dot(e1, e1), d12 = ft_dot(e1, e2), d22 = ft_dot(e2, e2);
      const float dp1 = ft_dot(ep, e1), dp2 = ft_dot(ep, e2);
      const float den = d11 * d22 - d12 * d12;
      if (den > 0.0f) {   // a NaN fails
        const float b1 = rt_div(d22 * dp1 - d12 * dp2, den), b2 = rt_div(d11 * dp2 - d12 * dp1, den);
        const rt3 f1 = bp - ap, f2 = cp - ap;
        const rt3 Pp = rt3_make(ap.x + (b1 * f1.x + b2 * f2.x), ap.y + (b1 * f1.y + b2 * f2.y), ap.z + (b1 * f1.z + b2 * f2.z));
        if (fm_finite(Pp.x) && fm_finite(Pp.y) && fm_finite(Pp.z)) {
          rt3 Np = rt_normalize(rt_cross(f1, f2));
          if (ft_dot(rt_cross(e1, e2), Nc) < 0.0f) Np = rt3_make(-Np.x, -Np.y, -Np.z);
          Pc = Pp;
          Nc = Np;
          status = RT_FRAME_MOTION_MOVED;
        }
      }
    }
  }
  A.carry[2 * i] = make_float4(Pc.x, Pc.y, Pc.z, rt_u2f(status));
  A.carry[2 * i + 1] = make_float4(Nc.x, Nc.y, Nc.z, rt_u2f(sid));
}

// after the temporal stage: this frame's transforms, by stable id, become the snapshot's.  ids is a permutation (the TLAS
// builder's order, or checked by rt_set_frame_motion_ids), so every row is written once; the range check stays.
__global__ __launch_bounds__(256) void k_frame_motion_scatter(const float4* __restrict__ inst, const uint32_t* __restrict__ ids,
                                                              float4* __restrict__ snap_xf, uint32_t n_inst) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_inst) return;
  const uint32_t sid = ids ? ids[p] : p;
  if (sid >= n_inst) return;
  const float4* I = inst + 9 * (size_t)p;
  const float4 c0 = I[0], c1 = I[1], c2 = I[2], c3 = I[3];
  float4* X = snap_xf + 4 * (size_t)sid;
  X[0] = c0;
  X[1] = c1;
  X[2] = c2;
  X[3] = c3;
}

}  // namespace rtk
#endif
