// leaf_sweep_model.cpp — TEST INFRASTRUCTURE: single rays through a BLAS, on the host, by the reference's stackless walk
// (Raytracer.wgsl:455-494, 532-563: every node, each box against the bound of its moment) and by the leaf sweep of
// csrc/k_traverse.hip.h traverse_leaves (the leaf records of csrc/scene_facts.h walk_facts alone, in walk order).  The slab
// test and the triangle test are hit_box4 and hit_tri_nb of k_traverse.hip.h restated over include/mi355rt_math.h, whose
// rt_min / rt_max drop a NaN as the device's do.  tests/test_leaf_sweep_model.py compares the two walks ray by ray.
// What it does NOT model is which lane tests which item when: a leaf's result is the minimum of (bits(t) << 32 | triangle)
// over the tests that pass against the bound at leaf entry, however the items are spread over a wave.
// build: g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC (tests/test_leaf_sweep_model.py does it)
#include <cstddef>
#include <cstdint>

#include "../../webgpu-raytracer_amd/csrc/scene_facts.h"

namespace {

struct Ray {
  rt3 o, d, inv_d, o_inv_d;
};
Ray make_ray(const float* q) {   // make_ray of k_intersect.hip.h
  Ray r;
  r.o = rt3_make(q[0], q[1], q[2]);
  r.d = rt3_make(q[4], q[5], q[6]);
  r.inv_d = rt3_make(rt_rcp(r.d.x), rt_rcp(r.d.y), rt_rcp(r.d.z));
  r.o_inv_d = rt3_make(r.o.x * r.inv_d.x, r.o.y * r.inv_d.y, r.o.z * r.inv_d.z);
  return r;
}
bool hit_box(const float* lo, const float* hi, const Ray& r, float t_min, float t_max) {
  float t1x = lo[0] * r.inv_d.x - r.o_inv_d.x, t2x = hi[0] * r.inv_d.x - r.o_inv_d.x;
  float t1y = lo[1] * r.inv_d.y - r.o_inv_d.y, t2y = hi[1] * r.inv_d.y - r.o_inv_d.y;
  float t1z = lo[2] * r.inv_d.z - r.o_inv_d.z, t2z = hi[2] * r.inv_d.z - r.o_inv_d.z;
  float nx = rt_min(t1x, t2x), ny = rt_min(t1y, t2y), nz = rt_min(t1z, t2z);
  float fx = rt_max(t1x, t2x), fy = rt_max(t1y, t2y), fz = rt_max(t1z, t2z);
  float tm_near = rt_max(t_min, rt_max(nx, rt_max(ny, nz)));
  float tm_far = rt_min(t_max, rt_min(fx, rt_min(fy, fz)));
  return tm_near <= tm_far;
}
bool hit_tri(const float* g, const Ray& r, float t_min, float t_max, float& t_out) {
  rt3 v0 = rt3_make(g[0], g[1], g[2]), e1 = rt3_make(g[4], g[5], g[6]), e2 = rt3_make(g[8], g[9], g[10]);
  rt3 h = rt_cross(r.d, e2);
  float a = rt_dot(e1, h);
  float f = rt_rcp(a);
  rt3 s = r.o - v0;
  float u = f * rt_dot(s, h);
  rt3 q = rt_cross(s, e1);
  float v = f * rt_dot(r.d, q);
  float t = f * rt_dot(e2, q);
  t_out = t;
  bool reject = (rt_abs(a) < 1e-6f) | (u < 0.0f) | (u > 1.0f) | (v < 0.0f) | (u + v > 1.0f);
  return !reject & (t > t_min) & (t < t_max);
}
bool finite_bits(float v) { return (rt_f2u(v) & 0x7f800000u) != 0x7f800000u; }

}  // namespace

extern "C" {

// rays: n x 8 f32 {o.xyz, t_min, d.xyz, t_max}, in the BLAS's space.  tri_geom: 12 f32 per triangle {v0, -, e1, -, e2, -}.
// out: n x 6 u32 {bits(closest t), triangle or 0xffffffff, occluded, triangle tests of the closest-hit walk,
// mask of the leaves the closest-hit walk hit (bit = position among the leaves in array order), the guard's predicate}.

// the reference: every node from `root`, skips relative to `root`
void lsm_reference(const float* blas, uint32_t root, const float* tri_geom, const float* rays, uint64_t n, uint32_t* out) {
  const uint32_t* bw = (const uint32_t*)blas;
  const uint32_t end = root + bw[8 * (size_t)root + 3];
  for (uint64_t k = 0; k < n; k++) {
    const float* q = rays + 8 * k;
    const Ray r = make_ray(q);
    const float t_min = q[3], t_max = q[7];
    float closest = t_max;
    uint32_t best = 0xffffffffu, tests = 0, mask = 0, ordinal = 0;
    for (uint32_t c = root; c < end;) {
      const float* nd = blas + 8 * (size_t)c;
      const uint32_t data = bw[8 * (size_t)c + 7];
      uint32_t next = root + bw[8 * (size_t)c + 3];
      // (position among the leaves: leaves before c in array order)
      ordinal = 0;
      for (uint32_t j = root; j < c; j++) ordinal += bw[8 * (size_t)j + 7] != 0u;
      if (hit_box(nd, nd + 4, r, t_min, closest)) {
        if (data != 0u) {
          mask |= 1u << (ordinal & 31u);
          const uint32_t first = data >> 3, count = data & 7u;
          for (uint32_t i = 0; i < count; i++) {
            tests++;
            float t;
            if (hit_tri(tri_geom + 12 * (size_t)(first + i), r, t_min, closest, t)) {
              closest = t;
              best = first + i;
            }
          }
        } else {
          next = c + 1u;
        }
      }
      c = next;
    }
    uint32_t occluded = 0;
    for (uint32_t c = root; c < end && !occluded;) {
      const float* nd = blas + 8 * (size_t)c;
      const uint32_t data = bw[8 * (size_t)c + 7];
      uint32_t next = root + bw[8 * (size_t)c + 3];
      if (hit_box(nd, nd + 4, r, t_min, t_max)) {
        if (data != 0u) {
          const uint32_t first = data >> 3, count = data & 7u;
          for (uint32_t i = 0; i < count && !occluded; i++) {
            float t;
            if (hit_tri(tri_geom + 12 * (size_t)(first + i), r, t_min, t_max, t)) occluded = 1;
          }
        } else {
          next = c + 1u;
        }
      }
      c = next;
    }
    uint32_t* o = out + 6 * k;
    o[0] = rt_f2u(closest);
    o[1] = best;
    o[2] = occluded;
    o[3] = tests;
    o[4] = mask;
    o[5] = !(finite_bits(r.inv_d.x) && finite_bits(r.inv_d.y) && finite_bits(r.inv_d.z) && finite_bits(r.o_inv_d.x) &&
             finite_bits(r.o_inv_d.y) && finite_bits(r.o_inv_d.z));
  }
}

// the sweep: the leaf records of walk_facts, nothing else of the tree.  Returns the number of leaves, or -1 when the tree is
// not sweepable at this cap.
int lsm_sweep(const float* blas, uint64_t n_blas, uint32_t root, uint32_t cap, const float* tri_geom, const float* rays,
              uint64_t n, uint32_t* out) {
  scene_facts::LeafRecord recs[scene_facts::kMaxLeafRecords];
  const launch_plan::WalkFacts f = scene_facts::walk_facts((const rt_node*)blas, (size_t)n_blas, root, cap, recs);
  if (!f.known || !f.sweepable) return -1;
  for (uint64_t k = 0; k < n; k++) {
    const float* q = rays + 8 * k;
    const Ray r = make_ray(q);
    const float t_min = q[3], t_max = q[7];
    float closest = t_max;
    uint32_t best = 0xffffffffu, tests = 0, mask = 0, occluded = 0;
    for (uint32_t l = 0; l < f.n_leaves; l++) {
      const scene_facts::LeafRecord& rec = recs[l];
      const uint32_t first = rec.data >> 3, count = rec.data & 7u;
      if (hit_box(rec.lo, rec.hi, r, t_min, closest)) {
        mask |= 1u << (l & 31u);
        // the items of the leaf, (owner's rank, k) = divmod(item, count) by the record's multiplier; each against the bound
        // at leaf entry, the smallest (bits(t) << 32 | triangle) wins
        unsigned long long res = ~0ull;
        for (uint32_t j = 0; j < count; j++) {
          const uint32_t rank = (j * rec.div) >> 16, i = j - rank * count;
          if (rank != 0u || i != j) return -2;
          tests++;
          float t;
          if (hit_tri(tri_geom + 12 * (size_t)(first + i), r, t_min, closest, t)) {
            const unsigned long long key = ((unsigned long long)rt_f2u(t) << 32) | (first + i);
            if (key < res) res = key;
          }
        }
        if (res != ~0ull) {
          closest = rt_u2f((uint32_t)(res >> 32));
          best = (uint32_t)res;
        }
      }
      if (hit_box(rec.lo, rec.hi, r, t_min, t_max)) {
        for (uint32_t i = 0; i < count; i++) {
          float t;
          if (hit_tri(tri_geom + 12 * (size_t)(first + i), r, t_min, t_max, t)) occluded = 1;
        }
      }
    }
    uint32_t* o = out + 6 * k;
    o[0] = rt_f2u(closest);
    o[1] = best;
    o[2] = occluded;
    o[3] = tests;
    o[4] = mask;
    o[5] = !(finite_bits(r.inv_d.x) && finite_bits(r.inv_d.y) && finite_bits(r.inv_d.z) && finite_bits(r.o_inv_d.x) &&
             finite_bits(r.o_inv_d.y) && finite_bits(r.o_inv_d.z));
  }
  return (int)f.n_leaves;
}

}  // extern "C"
