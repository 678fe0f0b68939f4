"""Register budget of the lightmap-bake kernels (k_bake_owner / _count / _emit / _scatter, csrc/k_bake.hip.h, and the
k_scan_counts of csrc/k_block_scan.hip.h between count and emit): each exists in the compiler's resource report, uses no
scratch memory and spills no VGPR.  No GPU needed."""
import pytest

from test_kernel_resources import resource_report

KERNELS = ("k_bake_owner", "k_bake_count", "k_scan_counts", "k_bake_emit", "k_bake_scatter")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("bake_resources"))


@pytest.mark.parametrize("name", KERNELS)
def test_bake_kernel_has_no_scratch_and_no_spills(kernels, name):
    names = [n for n in kernels if n.startswith("_ZN3rtk%d%sE" % (len(name), name))]
    assert len(names) == 1, (name, sorted(kernels))
    res = kernels[names[0]]
    print(name, res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0, res
