"""Register budget of the directional-gather kernels (k_dir_rays / k_dir_project / k_dir_scatter, csrc/k_directional.hip.h):
each exists once in the compiler's resource report of the gfx950 code object, uses no scratch memory, spills no VGPR and has
no LDS.  The trace between the first two is k_radiance_query itself, which tests/test_kernel_resources_radiance.py and
_gather.py hold to their budgets.  No GPU needed."""
import pytest

from test_kernel_resources import resource_report

KERNELS = ("k_dir_rays", "k_dir_project", "k_dir_scatter")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("directional_resources"))


@pytest.mark.parametrize("name", KERNELS)
def test_directional_kernel_has_no_scratch_and_no_spills(kernels, name):
    names = [n for n in kernels if n.startswith("_ZN3rtk%d%sE" % (len(name), name))]
    assert len(names) == 1, (name, sorted(kernels))
    res = kernels[names[0]]
    print(name, res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0, res
    assert int(res["LDS Size [bytes/block]"]) == 0, res
