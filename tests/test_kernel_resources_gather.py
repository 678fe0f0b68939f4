"""Register budget of the irradiance-gather kernels (k_irradiance_gather<DETAIL, LDS>, csrc/k_gather.hip.h): the four
instantiations exist, and in the same compiler report each uses no more scratch memory per lane, spills no more VGPRs and
runs at no fewer waves per SIMD than its twin k_pathtrace_persistent<DETAIL, LDS, false>, whose launch bounds it shares.
No GPU needed."""
import pytest

from test_kernel_resources import resource_report


def _b(x):
    return "Lb1E" if x else "Lb0E"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("gather_resources"))


def _one(kernels, prefix):
    names = [n for n in kernels if n.startswith(prefix)]
    assert len(names) == 1, (prefix, names)
    return kernels[names[0]]


def test_all_four_instantiations_exist(kernels):
    assert len([n for n in kernels if n.startswith("_ZN3rtk19k_irradiance_gatherI")]) == 4


@pytest.mark.parametrize("lds", [False, True])
@pytest.mark.parametrize("detail", [False, True])
def test_gather_kernel_budget_against_its_twin(kernels, detail, lds):
    res = _one(kernels, "_ZN3rtk19k_irradiance_gatherI%s%sEE" % (_b(detail), _b(lds)))
    twin = _one(kernels, "_ZN3rtk22k_pathtrace_persistentI%s%sLb0EEE" % (_b(detail), _b(lds)))
    print(detail, lds, res, twin)
    assert int(res["ScratchSize [bytes/lane]"]) <= int(twin["ScratchSize [bytes/lane]"]), (res, twin)
    assert int(res["VGPRs Spill"]) <= int(twin["VGPRs Spill"]), (res, twin)
    assert int(res["Occupancy [waves/SIMD]"]) >= int(twin["Occupancy [waves/SIMD]"]), (res, twin)
