// C wrapper over csrc/scene_facts.h for tests/test_scene_facts.py: topology records in, the facts the host would keep out.
// Host compiler only.
#include <cstddef>
#include <cstdint>

#include "../../webgpu-raytracer_amd/csrc/scene_facts.h"

extern "C" {

// the most triangles an upload may have and still be looked at
uint64_t sfc_max_tris() { return (uint64_t)scene_facts::kMaxTris; }

// topo: n_tris records of 80 bytes (rt_topology); returns known | plain << 1
int sfc_eval(const void* topo, uint64_t n_tris) {
  const launch_plan::SceneFacts f = scene_facts::topology_facts((const rt_topology*)topo, (size_t)n_tris);
  return (f.known ? 1 : 0) | (f.plain ? 2 : 0);
}

// the form persistent_shape picks with these facts for a one-instance, one-leaf scene of these sizes and a dispatch of
// n_frames frames: wide | plain << 1
int sfc_shape(uint32_t n_nodes, uint32_t n_tris, uint32_t n_verts, uint32_t n_frames, int detailed, int facts, int knob) {
  const launch_plan::SceneSize s = {n_nodes, n_nodes / 2u, n_tris, 1u, n_verts, 2u, 1u};
  launch_plan::PlanKnobs k;
  k.plain_materials = knob != 0;
  launch_plan::SceneFacts f;
  f.known = (facts & 1) != 0;
  f.plain = (facts & 2) != 0;
  const launch_plan::PersistentShape P = launch_plan::persistent_shape(s, k, n_frames, detailed != 0, f);
  const launch_plan::PersistentShape Q = launch_plan::persistent_shape(s, k, n_frames, detailed != 0);
  // the facts change the kernel alone: workgroups, LDS layout and size are those of the wide form
  if (P.lds != Q.lds || P.one_inst != Q.one_inst || P.wide != Q.wide || P.waves != Q.waves || P.dyn != Q.dyn || Q.plain) return -1;
  return (P.wide ? 1 : 0) | (P.plain ? 2 : 0);
}

}  // extern "C"
