"""Register budget of the atlas-bake kernels (k_atlas_items / _scan / _owner / _count / _emit / _scatter, csrc/k_bake.hip.h):
each exists in the compiler's resource report exactly once, uses no scratch memory and spills no VGPR.  No GPU needed."""
import pytest

from test_kernel_resources import resource_report

KERNELS = ("k_atlas_items", "k_atlas_scan", "k_atlas_owner", "k_atlas_count", "k_atlas_emit", "k_atlas_scatter")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("atlas_bake_resources"))


@pytest.mark.parametrize("name", KERNELS)
def test_atlas_kernel_has_no_scratch_and_no_spills(kernels, name):
    names = [n for n in kernels if n.startswith("_ZN3rtk%d%sE" % (len(name), name))]
    assert len(names) == 1, (name, sorted(kernels))
    res = kernels[names[0]]
    print(name, res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0, res
