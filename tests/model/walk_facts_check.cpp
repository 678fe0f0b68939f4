// C wrapper over the walk facts of csrc/scene_facts.h for tests/test_walk_facts.py: BLAS nodes in, the facts the host would keep
// and the leaf records it would upload out.  Host compiler only.
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../webgpu-raytracer_amd/csrc/scene_facts.h"

extern "C" {

uint64_t wfc_max_nodes() { return (uint64_t)scene_facts::kMaxWalkNodes; }
uint32_t wfc_max_records() { return scene_facts::kMaxLeafRecords; }
uint32_t wfc_default_cap() { return launch_plan::PlanKnobs().leaf_sweep_cap; }
uint32_t wfc_divider(uint32_t count) { return scene_facts::leaf_divider(count); }

// blas: n_blas nodes of 32 bytes; out: wfc_max_records() records of 32 bytes.  Returns known | sweepable << 1 | n_leaves << 8.
int wfc_eval(const void* blas, uint64_t n_blas, uint32_t root, uint32_t cap, void* out) {
  scene_facts::LeafRecord recs[scene_facts::kMaxLeafRecords];
  std::memset(recs, 0, sizeof(recs));
  const launch_plan::WalkFacts f = scene_facts::walk_facts((const rt_node*)blas, (size_t)n_blas, root, cap, recs);
  if (out) std::memcpy(out, recs, sizeof(recs));
  return (f.known ? 1 : 0) | (f.sweepable ? 2 : 0) | (int)(f.n_leaves << 8);
}

// the form persistent_shape picks with these walk facts for a one-instance, one-leaf scene of these sizes and a dispatch of
// n_frames frames: wide | plain << 1 | sweep << 2.  walk: known | sweepable << 1.
int wfc_shape(uint32_t n_nodes, uint32_t n_tris, uint32_t n_verts, uint32_t n_frames, int detailed, int plain, int walk,
              uint32_t n_leaves, int knob) {
  const launch_plan::SceneSize s = {n_nodes, n_nodes / 2u, n_tris, 1u, n_verts, 2u, 1u};
  launch_plan::PlanKnobs k;
  k.leaf_sweep = knob != 0;
  launch_plan::SceneFacts f;
  f.known = f.plain = plain != 0;
  launch_plan::WalkFacts w;
  w.known = (walk & 1) != 0;
  w.sweepable = (walk & 2) != 0;
  w.n_leaves = n_leaves;
  const launch_plan::PersistentShape P = launch_plan::persistent_shape(s, k, n_frames, detailed != 0, f, w);
  const launch_plan::PersistentShape Q = launch_plan::persistent_shape(s, k, n_frames, detailed != 0, f);
  // the walk facts change the kernel alone: workgroups, LDS layout and size are those of the wide form
  if (P.lds != Q.lds || P.one_inst != Q.one_inst || P.wide != Q.wide || P.waves != Q.waves || P.dyn != Q.dyn || P.plain != Q.plain ||
      Q.sweep)
    return -1;
  return (P.wide ? 1 : 0) | (P.plain ? 2 : 0) | (P.sweep ? 4 : 0);
}

}  // extern "C"
