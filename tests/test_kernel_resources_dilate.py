"""Register budget of the atlas-dilation kernels (k_dilate_mask / k_dilate_source / k_dilate_apply, csrc/k_dilate.hip.h): each
exists once in the compiler's resource report of the gfx950 code object, uses no scratch memory and spills no VGPR.
k_dilate_source keeps its 64-row window and four wave counts in LDS; the other two use none.  No GPU needed."""
import pytest

from test_kernel_resources import resource_report

KERNELS = ("k_dilate_mask", "k_dilate_source", "k_dilate_apply")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("dilate_resources"))


@pytest.mark.parametrize("name", KERNELS)
def test_dilate_kernel_has_no_scratch_and_no_spills(kernels, name):
    names = [n for n in kernels if n.startswith("_ZN3rtk%d%sE" % (len(name), name))]
    assert len(names) == 1, (name, sorted(kernels))
    res = kernels[names[0]]
    print(name, res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0, res
    if name != "k_dilate_source":
        assert int(res["LDS Size [bytes/block]"]) == 0, res
