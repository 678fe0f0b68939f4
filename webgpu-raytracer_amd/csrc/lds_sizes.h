// lds_sizes.h — what the kernels and the host's launch planner (launch_plan.h) must agree on: the LDS a wave owns in each
// kernel family and the records that tell a workgroup what to stage behind those wave blocks.  Nothing of HIP in here.
#ifndef MI355RT_LDS_SIZES_H
#define MI355RT_LDS_SIZES_H

#include <stdint.h>

// 16-byte slots per triangle record.  4 (one aligned 64-byte line per triangle; a 48-byte record straddles two lines
// 37 % of the time) was measured: no gain on any scene, 33 % more memory
#ifndef RT_TRI_STRIDE
#define RT_TRI_STRIDE 3
#endif

// a wave's triangle work queue (WaveWork, k_traverse.hip.h): 64 x 2 ray slots, up to 64 * 7 items, 64 results
#define RT_WORK_BYTES_PER_WAVE (64 * 32 + 64 * 7 * 4 + 64 * 8)

#ifndef RT_PW_STACK_K
#define RT_PW_STACK_K 7   // deferred right children a lane can hold (8 bytes each in LDS).  Fall-back rate measured on the
                          // host model (tests/test_pairwalk_model.py, random rays): K = 8: 0.3 % of the rays of the 263 k-
                          // triangle scene leave the stack, +0.5 % record fetches; K = 6: 2.7 %, +3 %; K = 4: 14 %, +15 %
#endif
#define RT_PW_STACK_BYTES_PER_WAVE (RT_PW_STACK_K * 64 * 8)
#define RT_PW_BYTES_PER_WAVE (RT_WORK_BYTES_PER_WAVE + RT_PW_STACK_BYTES_PER_WAVE)

#define RT_PT_COL_BYTES_PER_WAVE (64 * 12)   // the wide form's parked sample sums (launch_plan.h sizes its LDS with it)

#ifndef RT_WF_WAVES
#define RT_WF_WAVES 5   // waves per SIMD of the trace kernels: what the per-wave LDS block (work queue + stack, 8.3 KB at K = 8) leaves room for
#endif

namespace rtk {

// What a workgroup stages in LDS behind its wave queues (decided on the host from the scene's size, launch_plan.h plan_lds):
// the first k_nodes records of tnodes, and — when they fit as a whole — the instance rows + BLAS roots and the triangle
// records.  LDS = true (the whole scene fits, shading arrays included) ignores it.
struct LdsPlan {
  uint32_t k_nodes, stage_inst, stage_tri, pad;
};

struct TlasRoot {       // the TLAS root's box and word, by value in the kernel arguments (rt_api.hip fills it at upload)
  float lo[3];
  uint32_t word;
  float hi[3];
  uint32_t pad;
};

// What a workgroup stages in LDS behind its wave blocks (decided on the host, launch_plan.h plan_pairs): each array whole or
// not at all.
struct PairPlan {
  uint32_t stage_pairs, stage_inst, stage_tri, pad;
  TlasRoot troot;
};

// The 8x8 tile that wave `wave` (0-3) of workgroup `wg` casts in round `r` of the LDS form of k_primary_visibility, whose
// workgroups stage the scene once and then walk `rounds` tiles per wave: contiguous, so that a workgroup's tiles are
// neighbours and the tiles at or above the dispatch's count are the last ones of the last workgroup (launch_plan.h
// primary_shape chooses rounds, primary_grid_x the grid).  constexpr: the kernel and the host's tests call the same function.
constexpr uint32_t primary_tile(uint32_t wg, uint32_t rounds, uint32_t r, uint32_t wave) { return (wg * rounds + r) * 4u + wave; }

// FORM of k_ray_query: the five forms of the 256-thread trace kernels (launch_plan.h trace_shape picks as it does for
// k_wf_trace / k_wf_trace_pairs)
enum { RT_RQ_NODE_LDS = 0, RT_RQ_NODE_MIXED = 1, RT_RQ_NODE_RAYREG = 2, RT_RQ_PAIR_LDS = 3, RT_RQ_PAIR_GLOBAL = 4 };

}  // namespace rtk

#endif
