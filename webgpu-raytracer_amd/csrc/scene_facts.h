// scene_facts.h — what the host knows about the uploaded scene from the caller's own bytes: its materials (below), and whether
// the BLAS of a one-leaf scene can be walked over its leaves alone (walk_facts, at the end).  The materials are worked out
// once from the caller's topology bytes when they are uploaded (rt_upload(RT_KIND_TOPOLOGY)).  launch_plan.h persistent_shape
// reads it to choose the plain form of the wide one-leaf path tracer (k_pathtrace_persistent_plain), which carries no code
// for GGX, dielectrics, textures or emissive non-light triangles.  Functions of pure values, host-only C++17 over the shared
// math header, nothing of HIP:
// tests/test_scene_facts.py and tests/test_walk_facts.py run them without a GPU.
//
// Every clause below is the expression shade_bounce / setup_surface (k_pathtrace.hip.h) evaluate, on the same bits: the
// kernels read the record's data0..data3 from the shading record, to which k_prepare_tri_shade copies them unchanged, and
// mi355rt_math.h is one header for host and device (the device build is pinned to the host bit for bit).  A NaN therefore
// falls here as it falls in the kernel.
#ifndef MI355RT_SCENE_FACTS_H
#define MI355RT_SCENE_FACTS_H

#include <cstddef>
#include <cstdint>

#include "../../include/mi355rt_layout.h"
#include "../../include/mi355rt_math.h"
#include "launch_plan.h"

namespace scene_facts {

using launch_plan::SceneFacts;

// The most triangles a scene of a one-leaf LDS form can have: every triangle takes its traversal record, its shading record
// and its topology record of the 64 KB the whole scene must fit (launch_plan.h scene_lds_slots).  A larger upload cannot run
// the plain form and is not scanned.
constexpr size_t kMaxTris = (64 * 1024) / (16 * ((size_t)RT_TRI_STRIDE + 8 + 5));

// The triangle takes the Lambertian or the light branch of shade_bounce and no other: material word 0 or 3 as the kernel
// decodes it, none of the four texture tests true, and no emission on a triangle that is not a light.
inline bool triangle_is_plain(const rt_topology& t) {
  const uint32_t mat_type = rt_f2u32_sat(t.data0[3] + 0.5f);
  if (mat_type != 0u && mat_type != 3u) return false;
  if (t.data2[0] > -0.5f || t.data2[1] > -0.5f || t.data2[2] > -0.5f || t.data2[3] > -0.5f) return false;
  if (mat_type != 3u && rt_length(rt3_make(t.data3[0], t.data3[1], t.data3[2])) > 1e-4f) return false;
  return true;
}

// The facts of a topology upload of n_tris records.  known = false: too large to belong to a one-leaf LDS scene, not looked at.
inline SceneFacts topology_facts(const rt_topology* topo, size_t n_tris) {
  SceneFacts f;
  if (n_tris > kMaxTris || (n_tris && !topo)) return f;
  f.known = true;
  f.plain = true;
  for (size_t i = 0; i < n_tris; i++)
    if (!triangle_is_plain(topo[i])) {
      f.plain = false;
      break;
    }
  return f;
}

// ---- walk facts: can the BLAS of a one-leaf scene be walked over its leaves alone?
//
// The node walk (k_traverse.hip.h traverse) tests a ray against a leaf's box only after every ancestor's box has passed, each
// test against the bound `closest` of its own moment.  hit_box4 is a chain of rounded multiplies, subtractions, fmin and fmax,
// all monotone in the box words when the ray's inv_d and o_inv_d are finite, and `closest` only shrinks while a walk goes on.
// So when the stored box of every node lies inside the stored box of its parent (float compares on the words themselves), a
// leaf's test can pass only if the tests of all its ancestors passed before it: the leaves the node walk reaches and hits are
// the leaves whose own box test passes, taken in pre-order, each against the bound the leaves before it left.  walk_facts
// says whether the caller's BLAS bytes are such a tree, and lists its leaves in that order.  Anything it does not recognise
// keeps the node walk: a tree that is not in canonical pre-order (an inner node's first child is the next element, a node's
// skip is the end of its subtree, every node reachable, every inner node with two children or more), a leaf of 0 triangles, a
// non-finite or inverted box, a child box that sticks out of its parent's by as little as one ulp, more leaves than `cap`.
using launch_plan::WalkFacts;

// The most nodes the BLAS of a one-leaf LDS scene can have (32 bytes each of the 64 KB the scene must fit): the context keeps
// a host copy of no larger upload, and no larger one is scanned.
constexpr size_t kMaxWalkNodes = (64 * 1024) / 32;

// One leaf as traverse_leaves reads it: the node's 32 bytes with the skip word, which no sweep follows, replaced by the
// multiplier that divides an item number below 64 * 7 by the leaf's triangle count (item * div >> 16).
struct LeafRecord {
  float lo[3];
  uint32_t div;
  float hi[3];
  uint32_t data;   // first triangle << 3 | count, the node's word
};
static_assert(sizeof(LeafRecord) == 32, "a leaf record is a node's 32 bytes");
constexpr uint32_t kMaxLeafRecords = 64;   // what `out` of walk_facts must hold: no cap above it is honoured

// One node as the node sweep of traverse_leaves reads it (the walk a wave takes when the nesting argument above does not
// cover one of its rays): every node of the root's subtree in array order, which on a sweepable tree is the walk's order.  A
// leaf's record is its LeafRecord.  An inner node's has a zero word, which no leaf has, and in place of the skip the end of
// its subtree as a position in this array: where a ray that misses the box goes on.
typedef LeafRecord NodeRecord;
// every inner node of a sweepable tree has two children or more: what `nodes` of walk_facts must hold
constexpr uint32_t kMaxNodeRecords = 2u * kMaxLeafRecords - 1u;

inline uint32_t leaf_divider(uint32_t count) { return 65536u / count + 1u; }

// The record behind the last one of either array, which a sweep reads ahead and does not use.  It is no node: an inverted
// box under a zero word whose subtree would end at position 0, before the record itself.
inline LeafRecord padding_record() {
  LeafRecord r;
  for (int k = 0; k < 3; k++) {
    r.lo[k] = 3.402823466e+38f;
    r.hi[k] = -3.402823466e+38f;
  }
  r.div = 0u;
  r.data = 0u;
  return r;
}

// blas: the n_blas nodes of the caller's BLAS array; root: BLAS-local index of the root the one instance names.  Writes the
// leaves in walk order to out[0 .. n_leaves) when the tree is sweepable (out holds kMaxLeafRecords) and, when `nodes` is
// given (it holds kMaxNodeRecords), all its nodes in walk order to nodes[0 .. *n_nodes).
inline WalkFacts walk_facts(const rt_node* blas, size_t n_blas, uint32_t root, uint32_t cap, LeafRecord* out,
                            NodeRecord* nodes = nullptr, uint32_t* n_nodes = nullptr) {
  if (n_nodes) *n_nodes = 0u;
  WalkFacts f;
  if (!blas || !out || n_blas == 0 || n_blas > kMaxWalkNodes || root >= n_blas) return f;
  f.known = true;
  if (cap > kMaxLeafRecords) cap = kMaxLeafRecords;
  const uint32_t span = blas[root].skip;   // the walk ends at root + skip[root]
  if (span == 0u || span > n_blas - root) return f;
  const uint32_t end = root + span;
  struct Open {
    uint32_t end, node, kids;
  };
  Open open[64];   // the inner nodes whose subtree the scan is in: a deeper tree is not swept
  uint32_t depth = 0, n_leaves = 0;
  for (uint32_t i = root; i < end; i++) {
    const rt_node& n = blas[i];
    for (int k = 0; k < 3; k++) {
      // (x - x == 0 is false for an infinity and for a NaN; the compare below is false for a NaN too)
      if (!(n.min_b[k] - n.min_b[k] == 0.0f) || !(n.max_b[k] - n.max_b[k] == 0.0f) || !(n.min_b[k] <= n.max_b[k])) return f;
    }
    if (n.skip > span) return f;
    const uint32_t n_end = root + n.skip;
    if (n_end <= i) return f;   // a skip that goes back, or nowhere
    if (depth == 0u) {
      if (i != root) return f;   // a node behind the root's subtree
    } else {
      Open& p = open[depth - 1u];
      if (n_end > p.end) return f;
      const rt_node& pn = blas[p.node];
      for (int k = 0; k < 3; k++)
        if (!(pn.min_b[k] <= n.min_b[k]) || !(pn.max_b[k] >= n.max_b[k])) return f;
      p.kids++;
    }
    if (n.data == 0u) {   // inner: the first child is the next node, and a second one needs a node of its own
      if (n_end < i + 3u || depth == 64u) return f;
      open[depth++] = {n_end, i, 0u};
      if (nodes && i - root < kMaxNodeRecords) {   // (a tree of more nodes fails a test further on)
        NodeRecord& r = nodes[i - root];
        for (int k = 0; k < 3; k++) {
          r.lo[k] = n.min_b[k];
          r.hi[k] = n.max_b[k];
        }
        r.div = n.skip;   // n_end - root
        r.data = 0u;
      }
    } else {
      if (n_end != i + 1u) return f;   // nodes behind a leaf, inside its range: never reached
      const uint32_t count = n.data & 7u;
      if (count == 0u || n_leaves >= cap) return f;
      LeafRecord& r = out[n_leaves++];
      for (int k = 0; k < 3; k++) {
        r.lo[k] = n.min_b[k];
        r.hi[k] = n.max_b[k];
      }
      r.div = leaf_divider(count);
      r.data = n.data;
      if (nodes && i - root < kMaxNodeRecords) nodes[i - root] = r;
    }
    while (depth && open[depth - 1u].end == i + 1u) {
      if (open[depth - 1u].kids < 2u) return f;
      depth--;
    }
  }
  if (depth != 0u) return f;
  if (nodes && (span > kMaxNodeRecords || !n_nodes)) return f;   // (unreachable for span: at most 2 * cap - 1 nodes got here)
  f.sweepable = true;
  f.n_leaves = n_leaves;
  if (n_nodes) *n_nodes = span;
  return f;
}

}  // namespace scene_facts

#endif
