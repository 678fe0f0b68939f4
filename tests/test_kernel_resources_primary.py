"""Register budget of the LDS forms of k_primary_visibility (csrc/k_prepare_primary.hip.h).  The kernel is bound by
instruction issue at low throughput per SIMD, so it wants all eight waves: at most 64 VGPRs, no spilled VGPR, no scratch,
eight waves per SIMD (which also means at most 96 SGPRs) and no dynamic stack, in the product build of both LDS forms: the
one that casts many tiles per wave (k_primary_visibility_tiles: the tile loop keeps what it reads once per wave in scalar registers) and
the one of one tile per wave.  The global-memory form and the counting builds keep eight waves too.
Reads the compiler's resource report of tests/test_kernel_resources.py.  No GPU needed; skipped where hipcc is absent."""
import pytest

from test_kernel_resources import resource_report

PRIMARY = "_ZN3rtk20k_primary_visibility"        # <DETAIL, LDS>: one tile per wave
TILES = "_ZN3rtk26k_primary_visibility_tiles"     # <DETAIL>: many tiles per wave, an LDS form
FORMS = {"global": PRIMARY + "ILb0ELb0E", "lds": PRIMARY + "ILb0ELb1E", "lds_tiles": TILES + "ILb0E",
         "global_counting": PRIMARY + "ILb1ELb0E", "lds_counting": PRIMARY + "ILb1ELb1E", "lds_tiles_counting": TILES + "ILb1E"}


def _form(kernels, form):
    names = [n for n in kernels if n.startswith(FORMS[form])]
    assert len(names) == 1, sorted(n for n in kernels if n.startswith(PRIMARY))
    return kernels[names[0]]


def test_the_primary_kernel_has_these_six_forms(tmp_path):
    kernels = resource_report(tmp_path)
    assert len([n for n in kernels if n.startswith(PRIMARY)]) == 4 and len([n for n in kernels if n.startswith(TILES)]) == 2


@pytest.mark.parametrize("form", ["lds_tiles", "lds"])
def test_lds_product_forms_fit_eight_waves_without_spills(tmp_path, form):
    res = _form(resource_report(tmp_path), form)
    assert int(res["VGPRs"]) <= 64, res
    assert int(res["VGPRs Spill"]) == 0, res
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["Occupancy [waves/SIMD]"]) == 8, res
    assert res["Dynamic Stack"] == "False", res
    assert int(res["TotalSGPRs"]) <= 96, res   # more would cost the eighth wave whatever the VGPRs


@pytest.mark.parametrize("form", ["global", "global_counting", "lds_counting", "lds_tiles_counting"])
def test_the_other_forms_keep_eight_waves(tmp_path, form):
    res = _form(resource_report(tmp_path), form)
    assert int(res["VGPRs"]) <= 64, res
    assert int(res["VGPRs Spill"]) == 0, res
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["Occupancy [waves/SIMD]"]) == 8, res
    assert res["Dynamic Stack"] == "False", res
