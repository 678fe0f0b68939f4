// launch_plan.h — what the host decides for every kernel launched with dynamic LDS: which form of the kernel runs, how many
// threads a workgroup has, what each workgroup stages in LDS and how many bytes of dynamic LDS the launch asks for.
// Functions of pure values (the scene's sizes, the context's knobs), host-only C++17 over lds_sizes.h and the standard
// library, nothing of HIP: a kernel that stages more than `dyn` covers writes past its LDS allocation, so this is the part
// tests/test_launch_plan.py runs without a GPU.  rt_api.hip keeps the function-pointer tables, resident_blocks and the launches.
#ifndef MI355RT_LAUNCH_PLAN_H
#define MI355RT_LAUNCH_PLAN_H

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "lds_sizes.h"

namespace launch_plan {

using rtk::LdsPlan;
using rtk::PairPlan;

// Element counts of the uploaded scene: n_nodes = TLAS ++ BLAS, of which n_tlas in the TLAS; n_pairs = their inner nodes.
struct SceneSize {
  uint32_t n_nodes, n_pairs, n_tris, n_inst, n_verts, n_lights, n_tlas;
};
// What a context lets the environment or the caller set (rt_create, rt_set_walk).
struct PlanKnobs {
  size_t lds_per_cu = 160 * 1024;
  bool no_lds_staging = false;   // MI355RT_NO_LDS_STAGING=1 (test hook): every record through the global-memory paths
  long treelet_cap = -1;         // MI355RT_TREELET_MAX (plan_lds); < 0: unset
  int walk = 2;                  // traversal of the wavefront trace kernels: 1 = child-pair records, 0 = single nodes, 2 = auto
                                 // (MI355RT_WALK): pairs for a scene of ONE instance (measured: the 263 k-triangle hall -9 % per
                                 // batch; glass blob, 2 instances and short walks: +7 %; 1 001 instances of 8 triangles: +20 %)
  int wf_block = 0;              // threads per workgroup of the wavefront trace kernels (0 = default; MI355RT_WF_BLOCK)
  int wf_blocks_per_cu = 0;      // 0 = default for the block size (MI355RT_WF_BLOCKS_PER_CU)
  int wf_rayreg = -1;            // node-walk trace kernels: -1 = by scene, 0 / 1 = MI355RT_WF_RAYREG
  bool plain_materials = true;   // MI355RT_PLAIN_MATERIALS=0: a scene of plain materials runs the generic wide form all the same
  bool leaf_sweep = true;        // MI355RT_LEAF_SWEEP=0: a sweepable one-leaf scene keeps the node walk in the wide forms all the same
  uint32_t leaf_sweep_cap = 16;  // the most BLAS leaves a scene may have and still be swept (scene_facts.h walk_facts)
  bool leaf_sweep_guard = false; // MI355RT_LEAF_SWEEP_GUARD=1 (test hook): every walk of a sweep form sweeps the node records
                                 // instead of the leaf records (k_traverse.hip.h traverse_leaves), as the wave of a ray with
                                 // a non-finite slab operand does
  uint32_t n_cus = 256;          // compute units of the device (rt_create; the MI355X has 256)
  uint32_t primary_rounds = 0;   // MI355RT_PRIMARY_ROUNDS=n (test hook, sweeps): the LDS form of the primary kernel casts n
                                 // tiles per wave whatever the dispatch's size; 0 = primary_shape chooses
};
// What the host knows of the uploaded scene's materials (scene_facts.h works it out from the bytes of a topology upload).
// plain: every triangle is Lambertian or a light, untextured, and emits only if it is a light.  known = false: the host has
// not seen the bytes the device holds (a device-resident world update, an upload too large to matter), and nothing is assumed.
struct SceneFacts {
  bool known = false, plain = false;
};
// What the host knows of the BLAS the one TLAS leaf of a one-leaf scene names (scene_facts.h walk_facts works it out from the
// caller's bytes of rt_upload_bvh).  sweepable: the tree is a canonical pre-order tree of finite, nested boxes with at most
// PlanKnobs::leaf_sweep_cap leaves of 1-7 triangles, so that a walk over its n_leaves leaf boxes alone visits the triangles
// the node walk visits (k_traverse.hip.h traverse_leaves).  known = false: the nodes were written on the device, or are too
// many to belong to a one-leaf LDS scene.
struct WalkFacts {
  bool known = false, sweepable = false;
  uint32_t n_leaves = 0;
};

// ---- byte sizes of the arrays a walk stages, each whole or not at all
struct StagedBytes {
  size_t recs, tris, inst;   // node or pair records; triangle records; instance rows + roots
  size_t all() const { return recs + tris + inst; }
};
// node walk: tnodes, tri_geom, inst_trav + inst_root (one u32 per instance, in 16-byte slots)
inline StagedBytes node_walk_bytes(const SceneSize& s) {
  return {(size_t)32 * s.n_nodes, (size_t)16 * RT_TRI_STRIDE * s.n_tris, (size_t)64 * s.n_inst + (((size_t)s.n_inst + 3) / 4) * 16};
}
// pair walk: pairs, tri_geom, inst_trav + root_rec
inline StagedBytes pair_walk_bytes(const SceneSize& s) {
  return {(size_t)64 * s.n_pairs, (size_t)16 * RT_TRI_STRIDE * s.n_tris, (size_t)96 * s.n_inst};
}

// ---- slot counts of the forms that stage more than traversal records (16-byte LDS slots)
// number of 16-byte LDS slots the whole scene needs (traversal records + shading arrays), in the order stage_whole_scene
// (k_pathtrace.hip.h) stages them
inline size_t scene_lds_slots(const SceneSize& s) {
  // tnodes, tri_geom, inst_trav, inst_root | tri_shade | topo, pos, uv (light_pdf / light sampling of emissive hits), inst,
  // lights, light_rec
  return node_walk_bytes(s).all() / 16 + (size_t)8 * s.n_tris + (size_t)5 * s.n_tris + (size_t)s.n_verts + ((size_t)s.n_verts + 1) / 2 +
         (size_t)9 * s.n_inst + ((size_t)s.n_lights + 1) / 2 + (size_t)4 * s.n_lights;
}
// What the one-leaf forms (ONE_INST) really stage: no topo, pos, uv or inst, and two slots of world record per triangle
// (k_prepare_world_tris).  The launch asks for this much; the host still chooses between the 256-thread and the wide form,
// and decides whether a scene fits LDS at all, on scene_lds_slots, so that the scenes on either side of those lines stay
// where they were measured.
inline size_t one_leaf_lds_slots(const SceneSize& s) {
  // tnodes, tri_geom, inst_trav, inst_root | tri_shade | tri_world | lights, light_rec
  return node_walk_bytes(s).all() / 16 + (size_t)8 * s.n_tris + (size_t)2 * s.n_tris + ((size_t)s.n_lights + 1) / 2 + (size_t)4 * s.n_lights;
}
// 16-byte LDS slots of the records k_primary_visibility reads (nodes, triangle records, instance rows, per-triangle shading
// records)
inline size_t primary_lds_slots(const SceneSize& s) {
  const StagedBytes b = node_walk_bytes(s);
  return (b.recs + b.tris) / 16 + (size_t)4 * s.n_inst + (size_t)8 * s.n_tris;
}

inline size_t scene_lds_bytes(const SceneSize& s) { return scene_lds_slots(s) * 16; }
// the whole scene fits one workgroup's LDS beside four wave queues (the persistent kernel's LDS forms)
inline bool scene_fits_lds(const SceneSize& s, const PlanKnobs& k) {
  return !k.no_lds_staging && scene_lds_bytes(s) + (size_t)4 * RT_WORK_BYTES_PER_WAVE <= 64 * 1024;
}
// ... and its TLAS is one node, which is a leaf (k_validate_scene, or the world update's builder): the one-leaf forms, which
// read the per-triangle world records
// The forms chosen on this (the ONE_INST forms of the path tracer, k_primary_visibility_tiles) do not test the node's leaf
// word again: a TLAS of one node that is not a leaf naming an instance never reaches a launch (k_validate_scene refuses it).
inline bool one_leaf_lds(const SceneSize& s, const PlanKnobs& k) { return scene_fits_lds(s, k) && s.n_tlas == 1; }
// the trace kernels walk child-pair records, not single nodes (rt_set_walk; auto: a scene of one instance).  prepare_scene
// builds the records this says a launch will read.
inline bool walks_pairs(const SceneSize& s, const PlanKnobs& k) { return k.walk == 1 || (k.walk == 2 && s.n_inst == 1); }

// ---- plans: what one workgroup stages
// The LDS left for records beside the workgroup's `queue_bytes` of wave blocks, given `budget` bytes of LDS per workgroup: in
// bytes, whole 16-byte slots.
inline size_t lds_avail(size_t budget, size_t queue_bytes) {
  budget &= ~(size_t)2047;   // LDS is allocated in granules: leave room so that the intended number of workgroups fits a CU
  const size_t avail = budget > queue_bytes ? budget - queue_bytes : 0;
  return avail & ~(size_t)15;
}
// every record of the scene staged
inline LdsPlan full_lds_plan(const SceneSize& s) { return {s.n_nodes, 1, 1, 0}; }
// an array goes to LDS whole or not at all: 1 and `bytes` less in *avail when it fits
inline uint32_t stage_whole(size_t bytes, size_t* avail) {
  if (bytes > *avail) return 0;
  *avail -= bytes;
  return 1;
}
// What one workgroup stages in LDS behind its wave queues, given `budget` bytes of LDS per workgroup: the tnodes, the
// triangle records and the instance rows + BLAS roots, each if it fits whole.
// *dyn_bytes = dynamic LDS size of the launch.
inline LdsPlan plan_lds(const SceneSize& s, const PlanKnobs& k, size_t budget, size_t queue_bytes, size_t* dyn_bytes) {
  LdsPlan P = {};
  *dyn_bytes = queue_bytes;
  if (k.no_lds_staging) return P;
  const StagedBytes b = node_walk_bytes(s);
  const size_t room = lds_avail(budget, queue_bytes);
  size_t avail = room;
  // Nodes: all of them or none.  A partial treelet (the most visited nodes in LDS, the rest behind the L1) was measured
  // at 350 ... 3 200 nodes and never paid; MI355RT_TREELET_MAX = n stages min(n, what fits) for sweeps.
  size_t n = b.recs <= avail ? s.n_nodes : 0;
  if (k.treelet_cap >= 0) n = std::min<size_t>(std::min<size_t>(s.n_nodes, avail / 32), (size_t)k.treelet_cap);
  P.k_nodes = (uint32_t)n;
  avail -= n * 32;
  P.stage_tri = stage_whole(b.tris, &avail);
  P.stage_inst = stage_whole(b.inst, &avail);
  *dyn_bytes += room - avail;
  return P;
}
// The same for the child-pair walk of the trace kernels: pair records, triangle records, instance rows + root records.
inline PairPlan plan_pairs(const SceneSize& s, const PlanKnobs& k, size_t budget, size_t queue_bytes, size_t* dyn_bytes) {
  PairPlan P = {};
  *dyn_bytes = queue_bytes;
  if (k.no_lds_staging) return P;
  const StagedBytes b = pair_walk_bytes(s);
  const size_t room = lds_avail(budget, queue_bytes);
  size_t avail = room;
  P.stage_pairs = stage_whole(b.recs, &avail);
  P.stage_tri = stage_whole(b.tris, &avail);
  P.stage_inst = stage_whole(b.inst, &avail);
  *dyn_bytes += room - avail;
  return P;
}

// ---- the persistent path tracer and the path queries
struct PersistentShape {
  bool lds;            // the whole scene in LDS (template argument LDS); else `plan`
  bool one_inst;       // ... in a one-leaf form (ONE_INST)
  bool wide;           // ... in 512-thread workgroups (k_pathtrace_persistent_wide)
  uint32_t waves;      // per workgroup
  size_t dyn;          // dynamic LDS per workgroup: work queues + records
  LdsPlan plan;
  bool plain = false;  // ... the wide form without the code of the materials the scene does not have (k_pathtrace_persistent_plain)
  bool sweep = false;  // ... the wide form (plain or not) whose walks sweep the BLAS leaves (k_pathtrace_sweep_wide / _plain)
};
// The 256-thread forms of the persistent kernel (and the radiance query, which runs its path loop): the whole scene in LDS
// when it fits beside four wave queues (scene_fits_lds), else six workgroups per CU (6 waves per SIMD), each
// with its share of the CU's LDS for the top of the tree.
inline PersistentShape persistent_plan(const SceneSize& s, const PlanKnobs& k) {
  const size_t queue_bytes = (size_t)4 * RT_WORK_BYTES_PER_WAVE;
  PersistentShape P = {scene_fits_lds(s, k), false, false, 4u, 0, full_lds_plan(s), false};
  if (P.lds)
    P.dyn = queue_bytes + scene_lds_bytes(s);
  else
    P.plan = plan_lds(s, k, k.lds_per_cu / 6, queue_bytes, &P.dyn);
  return P;
}
// What compute() launches the persistent kernel in, for a dispatch of n_frames frames; detailed: the counting build.
inline PersistentShape persistent_shape(const SceneSize& s, const PlanKnobs& k, uint32_t n_frames, bool detailed,
                                        const SceneFacts& facts = SceneFacts(), const WalkFacts& walk = WalkFacts()) {
  PersistentShape P = persistent_plan(s, k);
  // LDS form of a scene whose TLAS is one node, which is a leaf (k_validate_scene, or the world update's builder): the walks skip the TLAS
  // half of the node step (k_traverse.hip.h traverse<.., ONE_INST>)
  P.one_inst = one_leaf_lds(s, k);
  if (!P.one_inst) return P;
  // These forms stage less than scene_lds (one_leaf_lds_slots): the launch asks for what they stage, while the
  // choice of the form, here and below, stays on scene_lds, the size the two sides of each line were measured at
  const size_t staged_lds = one_leaf_lds_slots(s) * 16;
  // the product build of that form in 512-thread workgroups (k_pathtrace_persistent_wide, 6 waves per SIMD) when three of
  // them, each with eight wave queues, eight waves' parked sample sums and one copy of the scene, fit the CU's LDS, and the
  // dispatch carries more than one frame: a single 1080p frame gives its 6 144 waves 1.3 tickets each, and there the
  // slower waves of the wide form lose more in the tail than the sixth wave gains (Cornell live loop, one dispatch per
  // frame: 0.906 -> 0.945 ms per frame)
  const size_t wide_blocks = (size_t)8 * (RT_WORK_BYTES_PER_WAVE + RT_PT_COL_BYTES_PER_WAVE);
  P.wide = !detailed && n_frames > 1 && wide_blocks + scene_lds_bytes(s) <= k.lds_per_cu / 3;
  P.waves = P.wide ? 8u : 4u;
  P.dyn = (P.wide ? wide_blocks : (size_t)4 * RT_WORK_BYTES_PER_WAVE) + staged_lds;
  // the wide form of a scene whose materials are known to be plain: the same workgroups, the same LDS layout and `dyn`
  P.plain = P.wide && facts.known && facts.plain && k.plain_materials;
  // the wide form of a scene whose BLAS the host knows to be sweepable: again the same workgroups, LDS layout and `dyn` (the
  // leaf records are read from global memory through the scalar cache)
  P.sweep = P.wide && walk.known && walk.sweepable && walk.n_leaves >= 1 && walk.n_leaves <= k.leaf_sweep_cap && k.leaf_sweep;
  return P;
}

// ---- the primary kernel
struct PrimaryShape {
  bool lds;   // small scene: records staged in LDS, four tiles at a time per workgroup
  int block;
  uint32_t tiles_per_workgroup;   // at a time: one per wave
  size_t dyn;
  uint32_t rounds = 1;   // tiles each wave casts, one after the other, behind the one staging of its workgroup
  bool tiles = false;    // ... in the LDS form that does so (k_primary_visibility_tiles) when rounds > 1: an
                         // unstriped dispatch of a one-leaf scene with tiles enough
};
// The most rounds the planner chooses on its own (sweep of 1 / 2 / 4 / 8 / 16 on the headline: profiles/r15_primary_tiles.txt).
constexpr uint32_t PRIMARY_ROUNDS_MAX = 8;
// ... and the fewest workgroups it leaves the grid, in units of what the chip keeps resident (eight 256-thread workgroups
// per CU at 8 waves per SIMD): longer workgroups quantise the end of the grid more coarsely.  Measured at 1080p (32 400
// tiles a frame): one frame in two rounds, 4 050 workgroups or 2.0 times the resident 2 048, is 0.9 % slower per frame of
// the live loop than one round; the 32-frame batch in 16 rounds, 7.9 times, is slower than in 8 rounds, 15.8 times.
constexpr uint32_t PRIMARY_MIN_RESIDENT_ROUNDS = 12;
// tile_frames: the tiles the dispatch casts, this rank's tiles x its frames (0: not said, one round); striped: the rank
// renders some of the image's rows only.  The form of many tiles per wave stages the scene once per workgroup, so fewer and
// longer workgroups stage less.  rounds = the largest power of two, PRIMARY_ROUNDS_MAX at most, that leaves the grid
// PRIMARY_MIN_RESIDENT_ROUNDS x 8 workgroups per CU: up to four 1080p frames keep one round, eight get 2, a 32-frame batch
// gets 8.  With one round the form of one tile per wave runs: the other one pays its once-per-wave part for a single tile
// (Cornell headline forced to one round: 21.92 ms per image against the parent's 21.65).
inline PrimaryShape primary_shape(const SceneSize& s, const PlanKnobs& k, uint64_t tile_frames = 0, bool striped = false) {
  const size_t plds = primary_lds_slots(s) * 16;
  if (plds > 32 * 1024 || k.no_lds_staging) return {false, 64, 1u, 0, 1u, false};
  if (!one_leaf_lds(s, k) || striped) return {true, 256, 4u, plds, 1u, false};
  uint32_t rounds = 1;
  if (k.primary_rounds)
    rounds = k.primary_rounds;
  else
    while (rounds < PRIMARY_ROUNDS_MAX && tile_frames / ((uint64_t)8 * rounds) >= (uint64_t)PRIMARY_MIN_RESIDENT_ROUNDS * 8 * k.n_cus) rounds *= 2;
  return {true, 256, 4u, plds, rounds, rounds > 1};
}
// x size of the primary kernel's grid for a rank that owns own_tiles (> 0) tiles; y is the number of frames
inline uint32_t primary_grid_x(const PrimaryShape& p, uint32_t own_tiles) {
  const uint64_t per_wg = (uint64_t)p.tiles_per_workgroup * p.rounds;
  return (uint32_t)((own_tiles + per_wg - 1) / per_wg);
}

// ---- the trace kernels
// Form and workgroup shape of the trace kernels for the uploaded scene: what launch_wavefront runs k_wf_trace /
// k_wf_trace_pairs in and rt_trace_rays its k_ray_query.  wf_block: threads per workgroup where not everything fits LDS
// (0 = 256; the ray query has 256-thread forms only).
struct TraceShape {
  bool pairs, trace_lds, rayreg;
  int block, blocks_per_cu;
  size_t dyn;              // dynamic LDS per workgroup
  PairPlan plan;           // pair walk: what a workgroup stages (troot: the caller's, rt_api.hip keeps it with the scene)
  LdsPlan nplan;           // node walk
  int rq_form;             // the form of k_ray_query that walks like this (RT_RQ_*, lds_sizes.h)
};
inline TraceShape trace_shape(const SceneSize& s, const PlanKnobs& k, int wf_block) {
  TraceShape T;
  T.pairs = walks_pairs(s, k);
  // Workgroup shape of the trace kernels.  Every wave owns `wave_bytes` of LDS: the triangle work queue, and for the pair walk
  // the stack of deferred right children.  Everything fits beside four wave blocks in 64 KB: 256-thread workgroups, all records
  // in LDS.  Otherwise 256-thread workgroups, each staging what fits whole in its share of the LDS (plan_pairs / plan_lds): the
  // pair walk as many per CU as the wave blocks allow (4 at K = 8), the node walk six (6 waves per SIMD).
  // MI355RT_WF_BLOCK / MI355RT_WF_BLOCKS_PER_CU override the shape for sweeps.
  const size_t wave_bytes = T.pairs ? RT_PW_BYTES_PER_WAVE : RT_WORK_BYTES_PER_WAVE;
  const size_t lds_records = (T.pairs ? pair_walk_bytes(s) : node_walk_bytes(s)).all();
  T.trace_lds = scene_fits_lds(s, k) && lds_records + (size_t)4 * wave_bytes <= 64 * 1024;
  T.block = 256;
  T.blocks_per_cu = 0;
  if (!T.trace_lds) {
    T.block = wf_block ? wf_block : 256;
    T.blocks_per_cu = k.wf_blocks_per_cu ? k.wf_blocks_per_cu
                      : T.pairs ? std::max(1, std::min((int)(k.lds_per_cu / ((size_t)(T.block / 64) * wave_bytes)), (RT_WF_WAVES * 256) / T.block))
                                : (T.block == 1024 ? 1 : (T.block == 512 ? 2 : 6));
  }
  const size_t queue_bytes = (size_t)(T.block / 64) * wave_bytes;
  T.dyn = queue_bytes + lds_records;
  T.plan = {};
  T.plan.stage_pairs = T.plan.stage_inst = T.plan.stage_tri = 1;
  T.nplan = full_lds_plan(s);
  if (!T.trace_lds) {
    const size_t budget = k.lds_per_cu / (size_t)T.blocks_per_cu;
    if (T.pairs)
      T.plan = plan_pairs(s, k, budget, queue_bytes, &T.dyn);
    else
      T.nplan = plan_lds(s, k, budget, queue_bytes, &T.dyn);
  }
  // few instances with deep trees (glass blob: 3 instances, 400 k nodes): a ray enters an instance once and then waits at
  // many leaves; measured, the form that keeps its instance-space origin / direction in registers is the faster one there,
  // the other one where rays enter many small instances (k_traverse.hip.h, trav_post_at_entry; MI355RT_WF_RAYREG=0/1 overrides)
  T.rayreg = !T.pairs && (k.wf_rayreg < 0 ? (size_t)s.n_nodes >= (size_t)1024 * std::max<size_t>(1, s.n_inst) : k.wf_rayreg != 0);
  T.rq_form = T.pairs ? (T.trace_lds ? rtk::RT_RQ_PAIR_LDS : rtk::RT_RQ_PAIR_GLOBAL)
                      : (T.trace_lds ? rtk::RT_RQ_NODE_LDS : (T.rayreg ? rtk::RT_RQ_NODE_RAYREG : rtk::RT_RQ_NODE_MIXED));
  return T;
}

}  // namespace launch_plan

#endif
