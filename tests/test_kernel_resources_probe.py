"""Register budget of the probe-gather kernels (k_probe_rays / k_probe_project, csrc/k_probe.hip.h): each exists once in the
compiler's resource report of the gfx950 code object, uses no scratch memory and spills no VGPR.  The trace between them is
k_radiance_query itself, which tests/test_kernel_resources_radiance.py and _gather.py hold to their budgets.  No GPU needed."""
import pytest

from test_kernel_resources import resource_report

KERNELS = ("k_probe_rays", "k_probe_project")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("probe_resources"))


@pytest.mark.parametrize("name", KERNELS)
def test_probe_kernel_has_no_scratch_and_no_spills(kernels, name):
    names = [n for n in kernels if n.startswith("_ZN3rtk%d%sE" % (len(name), name))]
    assert len(names) == 1, (name, sorted(kernels))
    res = kernels[names[0]]
    print(name, res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0, res
    assert int(res["LDS Size [bytes/block]"]) == 0, res
