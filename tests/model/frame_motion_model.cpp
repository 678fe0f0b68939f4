// frame_motion_model.cpp — the frame motion rule of include/mi355rt.h ("THE FRAME MOTION RULE") restated for the CPU in plain
// loops on the two public headers: the carry of every pixel (fm_model_carry), the temporal stage on that carry
// (fm_model_stage) and the snapshot's transforms by stable id (fm_model_scatter).  Nothing of csrc/k_frame_motion.hip.h or
// csrc/k_frame_temporal.hip.h is shared.  Has a main of its own: every UNTRACKED cause, every index out of its array included,
// on arrays allocated at their exact sizes - so that the same file builds as a stand-alone program under AddressSanitizer and
// UBSan, which then prove that no load is made through a bad index - and as the shared library tests/frame_motion_util.py loads.
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
void cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
bool finite_word(float x) { return (rt_f2u(x) & 0x7f800000u) != 0x7f800000u; }
void corner(const float* m, const float* v, float* o) {
  const rt3 r = rt_mat_mul_point(m, rt3_make(v[0], v[1], v[2]));
  o[0] = r.x;
  o[1] = r.y;
  o[2] = r.z;
}

}  // namespace

extern "C" {

// normal_id: W * H x 4 f32 and guide: W * H x 8 f32 of the current frame.  topo: n_tris rows of 20 words (rt_topology); pos:
// n_verts x 4 f32; inst: n_inst records of 36 words (rt_instance), TLAS order; ids: n_inst words or NULL (the identity).  snap_pos
// (n_verts x 4 f32) and snap_xf (n_inst x 16 f32, by stable id): the snapshot; snap_pos == NULL: none is kept.  Out: carry (W *
// H x 8 words), pix_id (W * H).
void fm_model_carry(const float* normal_id, const float* guide, const uint32_t* topo, uint32_t n_tris, const float* pos,
                    uint32_t n_verts, const float* inst, uint32_t n_inst, const uint32_t* ids, const float* snap_pos,
                    const float* snap_xf, uint32_t W, uint32_t H, float* carry, uint32_t* pix_id) {
  const size_t n = (size_t)W * H;
  for (size_t i = 0; i < n; i++) {
    const float* g = guide + 8 * i;
    float* o = carry + 8 * i;
    if (rt_f2u(g[7]) == 0u) {   // background
      for (int k = 0; k < 8; k++) o[k] = 0.0f;
      o[3] = rt_u2f(RT_FRAME_MOTION_BACKGROUND);
      o[7] = rt_u2f(RT_FRAME_MOTION_NO_ID);
      pix_id[i] = RT_FRAME_MOTION_NO_ID;
      continue;
    }
    const uint32_t tri = rt_f2u(normal_id[4 * i + 2]), in = rt_f2u(normal_id[4 * i + 3]);
    uint32_t sid = RT_FRAME_MOTION_NO_ID;
    if (in < n_inst) {
      sid = ids ? ids[in] : in;
      if (sid >= n_inst) sid = RT_FRAME_MOTION_NO_ID;
    }
    pix_id[i] = sid;
    std::memcpy(o, g, 32);   // {P, -} {N, -}
    o[3] = rt_u2f(RT_FRAME_MOTION_UNTRACKED);
    o[7] = rt_u2f(sid);
    if (!snap_pos || tri >= n_tris || in >= n_inst || sid == RT_FRAME_MOTION_NO_ID) continue;
    const uint32_t* row = topo + 20 * (size_t)tri;
    if (row[0] >= n_verts || row[1] >= n_verts || row[2] >= n_verts) continue;
    const float* M = inst + 36 * (size_t)in;
    const float* Mp = snap_xf + 16 * (size_t)sid;
    float c[3][3], cp[3][3];
    for (int k = 0; k < 3; k++) {
      corner(M, pos + 4 * (size_t)row[k], c[k]);
      corner(Mp, snap_pos + 4 * (size_t)row[k], cp[k]);
    }
    if (std::memcmp(c, cp, sizeof(c)) == 0) {
      o[3] = rt_u2f(RT_FRAME_MOTION_UNMOVED);
      continue;
    }
    float e1[3], e2[3], ep[3], f1[3], f2[3];
    for (int k = 0; k < 3; k++) {
      e1[k] = c[1][k] - c[0][k];
      e2[k] = c[2][k] - c[0][k];
      ep[k] = g[k] - c[0][k];
      f1[k] = cp[1][k] - cp[0][k];
      f2[k] = cp[2][k] - cp[0][k];
    }
    const float d11 = dot3(e1, e1), d12 = dot3(e1, e2), d22 = dot3(e2, e2), dp1 = dot3(ep, e1), dp2 = dot3(ep, e2);
    const float den = d11 * d22 - d12 * d12;
    if (!(den > 0.0f)) continue;
    const float b1 = rt_div(d22 * dp1 - d12 * dp2, den), b2 = rt_div(d11 * dp2 - d12 * dp1, den);
    float Pp[3];
    for (int k = 0; k < 3; k++) Pp[k] = cp[0][k] + (b1 * f1[k] + b2 * f2[k]);
    if (!finite_word(Pp[0]) || !finite_word(Pp[1]) || !finite_word(Pp[2])) continue;
    float nn[3], cn[3];
    cross3(f1, f2, nn);
    cross3(e1, e2, cn);
    rt3 Np = rt_normalize(rt3_make(nn[0], nn[1], nn[2]));
    if (dot3(cn, g + 4) < 0.0f) Np = rt3_make(-Np.x, -Np.y, -Np.z);
    o[0] = Pp[0]; o[1] = Pp[1]; o[2] = Pp[2];
    o[3] = rt_u2f(RT_FRAME_MOTION_MOVED);
    o[4] = Np.x; o[5] = Np.y; o[6] = Np.z;
  }
}

// the snapshot's transforms: the forward transform of the instance at TLAS position p goes to row ids[p]
void fm_model_scatter(const float* inst, uint32_t n_inst, const uint32_t* ids, float* snap_xf) {
  for (uint32_t p = 0; p < n_inst; p++) {
    const uint32_t sid = ids ? ids[p] : p;
    if (sid < n_inst) std::memcpy(snap_xf + 16 * (size_t)sid, inst + 36 * (size_t)p, 64);
  }
}

// The temporal stage under RT_FRAME_TEMPORAL_MOTION.  col, guide: the current frame's; carry: fm_model_carry's; prev_hist (x
// 4), prev_mom (x 2), prev_guide (x 8), prev_id (u32) and prev_U: the previous set; prev_hist == NULL: none is kept.  Out as
// ft_model_stage's.  Returns 0, or -1 for a descriptor the library refuses or one without the flag.
int fm_model_stage(const float* col, const float* guide, const float* carry, const float* prev_hist, const float* prev_mom,
                   const float* prev_guide, const uint32_t* prev_id, const rt_scene_uniforms* prev_U,
                   const rt_frame_temporal_desc* d, uint32_t W_, uint32_t H_, float* integ, float* hist, float* mom,
                   uint32_t* accepted) {
  if (!(d->flags & RT_FRAME_TEMPORAL_MOTION) || (d->flags & ~(RT_FRAME_TEMPORAL_SAME_INSTANCE | RT_FRAME_TEMPORAL_MOTION)) ||
      d->reserved[0] || d->reserved[1] || d->reserved[2] || d->max_history == 0 || d->max_history > RT_FRAME_TEMPORAL_MAX_HISTORY ||
      d->var_history == 0)
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
    cross3(hor, ver, nrm);
    jx = prev_U->jitter[0];
    jy = prev_U->jitter[1];
  }
  for (int64_t y = 0; y < H; y++)
    for (int64_t x = 0; x < W; x++) {
      const int64_t i = y * W + x;
      const float* c = col + 4 * i;
      const float* g = guide + 8 * i;
      const float* k = carry + 8 * i;   // {P', status} {N', sid}
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
      if (prev_hist && d->max_history != 1u && rt_f2u(k[3]) != RT_FRAME_MOTION_UNTRACKED) {
        float e[3], r[3];
        for (int a = 0; a < 3; a++) e[a] = k[a] - eye[a];
        const float s = rt_div(dot3(c0, nrm), dot3(e, nrm));
        for (int a = 0; a < 3; a++) r[a] = e[a] * s - c0[a];
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
            if ((d->flags & RT_FRAME_TEMPORAL_SAME_INSTANCE) && prev_id[q] != rt_f2u(k[7])) continue;
            if (!(dot3(k + 4, gq + 4) >= d->normal_cos)) continue;
            const float dp[3] = {gq[0] - k[0], gq[1] - k[1], gq[2] - k[2]};
            if (!(rt_abs(dot3(k + 4, dp)) <= d->plane_eps)) continue;
            wsum = wsum + w;
            for (int a = 0; a < 3; a++) acc[a] = acc[a] + w * hq[a];
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
      for (int ch = 0; ch < 3; ch++) {
        const float h = rt_div(acc[ch], wsum);
        const float q = h + a * (c[ch] - h);
        integ[4 * i + ch] = hist[4 * i + ch] = q;
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

// Self-check: one pixel per case on arrays of exactly their sizes (std::vector: a sanitizer sees every byte past the end).  A
// tracked pixel of a translated triangle is MOVED to the translated point; every other case is UNTRACKED, keeps the guide's P
// and N, and reads nothing through the bad index.
int main() {
  const uint32_t n_tris = 2, n_verts = 4, n_inst = 2;
  std::vector<uint32_t> topo(20 * n_tris, 0u);
  const uint32_t rows[2][3] = {{0, 1, 2}, {0, 1, 1}};   // row 1 has no area
  for (uint32_t t = 0; t < n_tris; t++)
    for (int k = 0; k < 3; k++) topo[20 * t + k] = rows[t][k];
  std::vector<float> pos = {0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 1, 1, 0, 1}, snap_pos = pos;
  std::vector<float> inst(36 * n_inst, 0.0f), snap_xf(16 * n_inst, 0.0f);
  for (uint32_t p = 0; p < n_inst; p++)
    for (int k = 0; k < 4; k++) inst[36 * p + 5 * k] = snap_xf[16 * p + 5 * k] = 1.0f;
  inst[12] = 0.25f;   // instance 0 has moved by 0.25 along x since the snapshot
  const uint32_t ids_ok[2] = {1, 0}, ids_bad[2] = {7, 0};
  snap_xf[16 + 13] = 0.5f;   // the snapshot's transform of stable id 1 (position 0 under ids_ok): 0.5 along y
  struct Case {
    const char* name;
    uint32_t tri, inst;
    const uint32_t* ids;
    bool snapshot;
    uint32_t bad_vertex;   // written into word 2 of row 0 for this case
    float nan_vertex;      // written into snap_pos[0] for this case
    uint32_t want;
  };
  const float nan = std::nanf("");
  const Case cases[] = {
      {"tracked", 0, 0, nullptr, true, 2, 0.0f, RT_FRAME_MOTION_MOVED},
      {"tracked by id", 0, 0, ids_ok, true, 2, 0.0f, RT_FRAME_MOTION_MOVED},
      {"unmoved", 0, 1, ids_ok, true, 2, 0.0f, RT_FRAME_MOTION_UNMOVED},
      {"tri == n_tris", n_tris, 0, nullptr, true, 2, 0.0f, RT_FRAME_MOTION_UNTRACKED},
      {"tri = 2^32 - 1", 0xffffffffu, 0, nullptr, true, 2, 0.0f, RT_FRAME_MOTION_UNTRACKED},
      {"inst == n_inst", 0, n_inst, nullptr, true, 2, 0.0f, RT_FRAME_MOTION_UNTRACKED},
      {"inst = 2^31", 0, 0x80000000u, ids_ok, true, 2, 0.0f, RT_FRAME_MOTION_UNTRACKED},
      {"sid out of range", 0, 0, ids_bad, true, 2, 0.0f, RT_FRAME_MOTION_UNTRACKED},
      {"vertex == n_verts", 0, 0, nullptr, true, n_verts, 0.0f, RT_FRAME_MOTION_UNTRACKED},
      {"vertex = 2^32 - 1", 0, 0, nullptr, true, 0xffffffffu, 0.0f, RT_FRAME_MOTION_UNTRACKED},
      {"no snapshot", 0, 0, nullptr, false, 2, 0.0f, RT_FRAME_MOTION_UNTRACKED},
      {"no area", 1, 0, nullptr, true, 2, 0.0f, RT_FRAME_MOTION_UNTRACKED},
      {"NaN vertex in the snapshot", 0, 0, nullptr, true, 2, nan, RT_FRAME_MOTION_UNTRACKED},
  };
  int bad = 0;
  for (const Case& k : cases) {
    topo[2] = k.bad_vertex;
    snap_pos[0] = k.nan_vertex;
    std::vector<float> nid = {0.0f, 0.0f, rt_u2f(k.tri), rt_u2f(k.inst)};
    std::vector<float> guide = {0.25f, 0.25f, 0.0f, rt_u2f(k.inst), 0.0f, 0.0f, 1.0f, rt_u2f(1u)}, carry(8, -1.0f);
    guide[0] += k.inst == 0 ? 0.25f : 0.0f;   // the point (0.25, 0.25) of the object, through this frame's transform
    std::vector<uint32_t> pid(1, 5u);
    fm_model_carry(nid.data(), guide.data(), topo.data(), n_tris, pos.data(), n_verts, inst.data(), n_inst, k.ids,
                   k.snapshot ? snap_pos.data() : nullptr, k.snapshot ? snap_xf.data() : nullptr, 1, 1, carry.data(), pid.data());
    const uint32_t st = rt_f2u(carry[3]);
    bool ok = st == k.want;
    if (st == RT_FRAME_MOTION_MOVED) {
      const float wy = k.ids ? 0.75f : 0.25f;   // by id the snapshot's transform is the one moved along y
      ok = ok && std::fabs(carry[0] - 0.25f) < 1e-6f && std::fabs(carry[1] - wy) < 1e-6f && carry[2] == 0.0f && carry[6] == 1.0f;
    } else {
      ok = ok && std::memcmp(carry.data(), guide.data(), 12) == 0 && std::memcmp(carry.data() + 4, guide.data() + 4, 12) == 0;
    }
    if (!ok) {
      std::printf("case '%s': status %u, carry %g %g %g\n", k.name, st, carry[0], carry[1], carry[2]);
      bad++;
    }
  }
  std::printf("frame_motion_model self-check: %d bad cases\n", bad);
  return bad ? 1 : 0;
}
