"""Register budget of the reflection-probe kernels (csrc/k_reflection.hip.h): each exists once in the compiler's resource
report of the gfx950 code object - k_reflection_filter once per build, for 4, 16 and 64 samples per lane - uses no scratch
memory, spills no register and declares no LDS; the filter's builds keep the occupancy their register arrays were sized for.
The path work of a capture is the radiance query's, which tests/test_kernel_resources_radiance.py holds to its budget.  No GPU
needed."""
import pytest

from test_kernel_resources import resource_report

PLAIN = ("k_reflection_rays", "k_reflection_texels", "k_reflection_copy")
FILTER_BUILDS = {4: 8, 16: 4, 64: 2}      # samples per lane -> waves per SIMD the build must keep


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("reflection_resources"))


def _clean(res):
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0 and int(res["SGPRs Spill"]) == 0, res
    assert int(res["LDS Size [bytes/block]"]) == 0, res


@pytest.mark.parametrize("name", PLAIN)
def test_capture_kernel_has_no_scratch_no_spills_and_no_lds(kernels, name):
    names = [n for n in kernels if n.startswith("_ZN3rtk%d%sE" % (len(name), name))]
    assert len(names) == 1, (name, sorted(kernels))
    print(name, kernels[names[0]])
    _clean(kernels[names[0]])


@pytest.mark.parametrize("ns", sorted(FILTER_BUILDS))
def test_filter_build_has_no_scratch_no_spills_and_keeps_its_occupancy(kernels, ns):
    names = [n for n in kernels if n.startswith("_ZN3rtk19k_reflection_filterILi%dEEE" % ns)]
    assert len(names) == 1, (ns, [n for n in kernels if "k_reflection_filter" in n])
    res = kernels[names[0]]
    print(ns, res)
    _clean(res)
    assert int(res["Occupancy [waves/SIMD]"]) >= FILTER_BUILDS[ns], res


def test_there_are_no_other_filter_builds(kernels):
    assert len([n for n in kernels if "k_reflection_filter" in n]) == len(FILTER_BUILDS)
