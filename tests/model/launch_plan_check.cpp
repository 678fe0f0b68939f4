// C wrapper over csrc/launch_plan.h for tests/test_launch_plan.py: one scene size and one set of knobs in, every plan and
// launch shape the host would choose out, as a flat array of integers in the order lpc_fields() names.  Host compiler only.
#include <cstdint>

#include "../../webgpu-raytracer_amd/csrc/launch_plan.h"

namespace lp = launch_plan;

static const char* const kFields =
    "fits_lds,one_leaf,walks_pairs,"
#define TS(T) T ".pairs," T ".trace_lds," T ".rayreg," T ".block," T ".blocks_per_cu," T ".dyn," T ".plan.stage_pairs," \
              T ".plan.stage_inst," T ".plan.stage_tri," T ".nplan.k_nodes," T ".nplan.stage_inst," T ".nplan.stage_tri," T ".rq_form,"
    TS("trace") TS("query")   // trace_shape as launch_wavefront asks (the context's wf_block) and as the ray query does (0)
#undef TS
    "persistent_plan.k_nodes,persistent_plan.stage_inst,persistent_plan.stage_tri,persistent_plan.dyn,"
#define PS(T) T ".lds," T ".one_inst," T ".wide," T ".waves," T ".dyn," T ".plan.k_nodes," T ".plan.stage_inst," T ".plan.stage_tri,"
    PS("persistent_shape.n1") PS("persistent_shape.n1.detailed") PS("persistent_shape.n2") PS("persistent_shape.n2.detailed")
#undef PS
    "primary.lds,primary.block,primary.tiles_per_workgroup,primary.dyn";

static int64_t* put(int64_t* o, const lp::TraceShape& T) {
  const int64_t v[] = {T.pairs, T.trace_lds, T.rayreg, T.block, T.blocks_per_cu, (int64_t)T.dyn, T.plan.stage_pairs, T.plan.stage_inst,
                       T.plan.stage_tri, T.nplan.k_nodes, T.nplan.stage_inst, T.nplan.stage_tri, T.rq_form};
  for (int64_t x : v) *o++ = x;
  return o;
}
static int64_t* put(int64_t* o, const lp::PersistentShape& P) {
  const int64_t v[] = {P.lds, P.one_inst, P.wide, P.waves, (int64_t)P.dyn, P.plan.k_nodes, P.plan.stage_inst, P.plan.stage_tri};
  for (int64_t x : v) *o++ = x;
  return o;
}

extern "C" {

const char* lpc_fields() { return kFields; }

// in: n_nodes n_pairs n_tris n_inst n_verts n_lights n_tlas | lds_per_cu no_lds_staging treelet_cap walk wf_block
// wf_blocks_per_cu wf_rayreg; returns the number of values written to out (at most 128)
int lpc_eval(const int64_t* in, int64_t* out) {
  const lp::SceneSize s = {(uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], (uint32_t)in[4], (uint32_t)in[5], (uint32_t)in[6]};
  lp::PlanKnobs k;
  k.lds_per_cu = (size_t)in[7];
  k.no_lds_staging = in[8] != 0;
  k.treelet_cap = (long)in[9];
  k.walk = (int)in[10];
  k.wf_block = (int)in[11];
  k.wf_blocks_per_cu = (int)in[12];
  k.wf_rayreg = (int)in[13];
  int64_t* o = out;
  *o++ = lp::scene_fits_lds(s, k);
  *o++ = lp::one_leaf_lds(s, k);
  *o++ = lp::walks_pairs(s, k);
  o = put(o, lp::trace_shape(s, k, k.wf_block));
  o = put(o, lp::trace_shape(s, k, 0));
  const lp::PersistentShape pp = lp::persistent_plan(s, k);
  *o++ = pp.plan.k_nodes;
  *o++ = pp.plan.stage_inst;
  *o++ = pp.plan.stage_tri;
  *o++ = (int64_t)pp.dyn;
  for (uint32_t n = 1; n <= 2; n++)
    for (int detailed = 0; detailed < 2; detailed++) o = put(o, lp::persistent_shape(s, k, n, detailed != 0));
  const lp::PrimaryShape pr = lp::primary_shape(s, k);
  *o++ = pr.lds;
  *o++ = pr.block;
  *o++ = pr.tiles_per_workgroup;
  *o++ = (int64_t)pr.dyn;
  return (int)(o - out);
}

}  // extern "C"
