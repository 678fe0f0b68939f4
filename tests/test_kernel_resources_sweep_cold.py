"""Register budget of the two sweep forms once the walk of a wave with a non-finite slab operand is a sweep over the node
records (csrc/k_traverse.hip.h traverse_leaves) and no node walk is inlined into them.

k_pathtrace_sweep_plain must be what the leaf sweep alone was measured at: 80 VGPRs, no spilled VGPR, no scratch, six waves
per SIMD, no dynamic stack (with the node walk inlined it spilled 27 VGPRs to 48 bytes of scratch per lane).
k_pathtrace_sweep_wide spills for its materials, as its node-walk twin does (13 VGPRs, 28 bytes): 19 VGPRs and 44 bytes per
lane is what the cross-compiler for gfx950 gives at this commit (36 and 64 with the node walk inlined), and the ceiling here.
(That is its one-loop form, traverse_leaves<.., ONE_LOOP = true>; with a loop per record array, as the plain form has them, it
spills 20 VGPRs, which is why it does not: profiles/r14_sweep_cold.txt.)
Reads the compiler's resource report of tests/test_kernel_resources.py.  No GPU needed; skipped where hipcc is absent."""
from test_kernel_resources import resource_report
from test_kernel_resources_leaf_sweep import SWEEP_PLAIN, SWEEP_WIDE, _one

WIDE_SPILLS, WIDE_SCRATCH = 19, 44   # as measured at this commit


def test_the_plain_sweep_form_has_no_spill_and_no_scratch(tmp_path):
    _, res = _one(resource_report(tmp_path), SWEEP_PLAIN)
    assert int(res["VGPRs"]) == 80, res
    assert int(res["VGPRs Spill"]) == 0, res
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["Occupancy [waves/SIMD]"]) == 6, res
    assert res["Dynamic Stack"] == "False", res


def test_the_generic_sweep_form_spills_no_more_than_measured(tmp_path):
    assert WIDE_SPILLS <= 19 and WIDE_SCRATCH <= 44
    _, res = _one(resource_report(tmp_path), SWEEP_WIDE)
    assert int(res["VGPRs"]) <= 80, res
    assert int(res["VGPRs Spill"]) <= WIDE_SPILLS, res
    assert int(res["ScratchSize [bytes/lane]"]) <= WIDE_SCRATCH, res
    assert int(res["Occupancy [waves/SIMD]"]) >= 6, res
    assert res["Dynamic Stack"] == "False", res
