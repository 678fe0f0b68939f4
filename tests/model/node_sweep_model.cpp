// node_sweep_model.cpp — TEST INFRASTRUCTURE: single rays through a sweepable BLAS, on the host, by the node sweep of
// csrc/k_traverse.hip.h traverse_leaves: the walk a wave takes when one of its rays has a non-finite slab operand.  The node
// records of csrc/scene_facts.h walk_facts (every node in array order; an inner node under a zero word, with the end of its
// subtree as a position), one word of state per ray (skip_until, the first position it tests again), and at a leaf the
// minimum of (bits(t) << 32 | triangle) over the tests that pass against the bound at leaf entry.  The slab test, the
// triangle test and the reference's stackless walk (lsm_reference) are those of leaf_sweep_model.cpp, included below, so
// that all three walks test with one piece of code over include/mi355rt_math.h.  tests/test_node_sweep_model.py compares
// the node sweep with the reference ray by ray, for rays of any bit pattern.
// build: g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC (tests/test_node_sweep_model.py does it)
#include <cstring>

#include "leaf_sweep_model.cpp"

extern "C" {

// The records walk_facts makes of a tree: leaves[0 .. return value) and nodes[0 .. *n_nodes), 8 words each, and the padding
// record the host puts behind either array.  -1: not sweepable at this cap.
int nsm_records(const float* blas, uint64_t n_blas, uint32_t root, uint32_t cap, uint32_t* leaves, uint32_t* nodes,
                uint32_t* n_nodes, uint32_t* padding) {
  static_assert(sizeof(scene_facts::NodeRecord) == 32, "8 words");
  const scene_facts::LeafRecord pad = scene_facts::padding_record();
  std::memcpy(padding, &pad, sizeof pad);
  const launch_plan::WalkFacts f =
      scene_facts::walk_facts((const rt_node*)blas, (size_t)n_blas, root, cap, (scene_facts::LeafRecord*)leaves,
                              (scene_facts::NodeRecord*)nodes, n_nodes);
  return f.known && f.sweepable ? (int)f.n_leaves : -1;
}

// rays, tri_geom, out: as lsm_reference.  Returns the number of nodes, or -1 when the tree is not sweepable at this cap.
int nsm_sweep(const float* blas, uint64_t n_blas, uint32_t root, uint32_t cap, const float* tri_geom, const float* rays,
              uint64_t n, uint32_t* out) {
  scene_facts::LeafRecord leaves[scene_facts::kMaxLeafRecords];
  scene_facts::NodeRecord recs[scene_facts::kMaxNodeRecords];
  uint32_t n_nodes = 0;
  const launch_plan::WalkFacts f = scene_facts::walk_facts((const rt_node*)blas, (size_t)n_blas, root, cap, leaves, recs, &n_nodes);
  if (!f.known || !f.sweepable) return -1;
  for (uint64_t k = 0; k < n; k++) {
    const float* q = rays + 8 * k;
    const Ray r = make_ray(q);
    const float t_min = q[3], t_max = q[7];
    // closest hit
    float closest = t_max;
    uint32_t best = 0xffffffffu, tests = 0, mask = 0, ordinal = 0, skip_until = 0;
    for (uint32_t i = 0; i < n_nodes; i++) {
      const scene_facts::NodeRecord& rec = recs[i];
      const uint32_t l = ordinal;   // position among the leaves
      ordinal += rec.data != 0u;
      if (i < skip_until) continue;
      const bool hit = hit_box(rec.lo, rec.hi, r, t_min, closest);
      if (rec.data == 0u) {
        if (!hit) skip_until = rec.div;   // the end of the subtree
        continue;
      }
      if (!hit) continue;
      mask |= 1u << (l & 31u);
      const uint32_t first = rec.data >> 3, count = rec.data & 7u;
      unsigned long long res = ~0ull;
      for (uint32_t j = 0; j < count; j++) {
        const uint32_t rank = (j * rec.div) >> 16, t_in_leaf = j - rank * count;
        if (rank != 0u || t_in_leaf != j) return -2;
        tests++;
        float t;
        if (hit_tri(tri_geom + 12 * (size_t)(first + t_in_leaf), r, t_min, closest, t)) {
          const unsigned long long key = ((unsigned long long)rt_f2u(t) << 32) | (first + t_in_leaf);
          if (key < res) res = key;
        }
      }
      if (res != ~0ull) {
        closest = rt_u2f((uint32_t)(res >> 32));
        best = (uint32_t)res;
      }
    }
    // any hit: every box against t_max; a ray found occluded tests no more (the device learns it a chunk later, which
    // changes no answer: an occluded ray stays occluded)
    uint32_t occluded = 0;
    skip_until = 0;
    for (uint32_t i = 0; i < n_nodes && !occluded; i++) {
      const scene_facts::NodeRecord& rec = recs[i];
      if (i < skip_until) continue;
      const bool hit = hit_box(rec.lo, rec.hi, r, t_min, t_max);
      if (rec.data == 0u) {
        if (!hit) skip_until = rec.div;
        continue;
      }
      if (!hit) continue;
      const uint32_t first = rec.data >> 3, count = rec.data & 7u;
      for (uint32_t j = 0; j < count; j++) {
        float t;
        if (hit_tri(tri_geom + 12 * (size_t)(first + j), r, t_min, t_max, t)) occluded = 1;
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
  return (int)n_nodes;
}

}  // extern "C"
