// scene_facts.h — what the host knows about the materials of the uploaded scene, worked out once from the caller's topology
// bytes when they are uploaded (rt_upload(RT_KIND_TOPOLOGY)).  launch_plan.h persistent_shape reads it to choose the plain
// form of the wide one-leaf path tracer (k_pathtrace_persistent_plain), which carries no code for GGX, dielectrics, textures
// or emissive non-light triangles.  Functions of pure values, host-only C++17 over the shared math header, nothing of HIP:
// tests/test_scene_facts.py runs them without a GPU.
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

}  // namespace scene_facts

#endif
