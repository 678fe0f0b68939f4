"""Register budget of the two sweep forms of the wide one-leaf path tracer (k_pathtrace_sweep_plain, k_pathtrace_sweep_wide,
csrc/k_pathtrace.hip.h: the walks test the BLAS leaves alone, csrc/k_traverse.hip.h traverse_leaves).  Both must fit six waves
per SIMD, 80 VGPRs, like the forms they replace, and share their launch (no static LDS).

The sweep alone holds the plain form at 80 VGPRs without a spill and without scratch (measured with the guard's branch
compiled out).  The node walk that a wave takes when one of its rays has a non-finite reciprocal direction is inlined into
the same kernel, and with it the compiler spills: the plain sweep form 27 VGPRs to 48 bytes of scratch per lane, the generic
one 36 VGPRs to 64 bytes (its node-walk twin: 13 VGPRs, 28 bytes).  Those are the figures of the cross-compiler for gfx950
at this commit, and the ceilings here; the form was kept on its timing (profiles/r13_leaf_sweep.txt).  Reads the compiler's
resource report of tests/test_kernel_resources.py.  No GPU needed; skipped where hipcc is absent."""
import pytest

from test_kernel_resources import resource_report

SWEEP_PLAIN = "_ZN3rtk23k_pathtrace_sweep_plain"
SWEEP_WIDE = "_ZN3rtk22k_pathtrace_sweep_wide"
# form -> (spilled VGPRs, scratch bytes per lane) as measured
CEILINGS = {SWEEP_PLAIN: (27, 48), SWEEP_WIDE: (36, 64)}


def _one(kernels, prefix):
    names = [n for n in kernels if n.startswith(prefix)]
    assert len(names) == 1, sorted(kernels)
    return names[0], kernels[names[0]]


@pytest.mark.parametrize("prefix", [SWEEP_PLAIN, SWEEP_WIDE])
def test_sweep_forms_are_product_one_leaf_instances_alone(tmp_path, prefix):
    name, _ = _one(resource_report(tmp_path), prefix)
    assert name.startswith(prefix + "ILb0ELb1ELb1E"), name


@pytest.mark.parametrize("prefix", [SWEEP_PLAIN, SWEEP_WIDE])
def test_sweep_forms_run_at_six_waves_within_their_measured_spills(tmp_path, prefix):
    _, res = _one(resource_report(tmp_path), prefix)
    spills, scratch = CEILINGS[prefix]
    assert int(res["Occupancy [waves/SIMD]"]) >= 6, res
    assert int(res["VGPRs"]) <= 80, res
    assert int(res["VGPRs Spill"]) <= spills, res
    assert int(res["ScratchSize [bytes/lane]"]) <= scratch, res
    assert res["Dynamic Stack"] == "False", res   # the guard's node walk is inlined, not called


@pytest.mark.parametrize("prefix", [SWEEP_PLAIN, SWEEP_WIDE])
def test_sweep_forms_share_the_wide_forms_launch(tmp_path, prefix):
    _, res = _one(resource_report(tmp_path), prefix)
    assert int(res["LDS Size [bytes/block]"]) == 0, res
