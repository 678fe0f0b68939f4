"""Register and LDS budget of the encode kernel (k_encode_atlas, csrc/k_encode.hip.h): it exists once in the compiler's
resource report of the gfx950 code object, uses no scratch memory, spills nothing and - a streaming kernel, one load and one
store per texel - uses no LDS.  No GPU needed."""
import pytest

from test_kernel_resources import resource_report

KERNEL = "k_encode_atlas"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("encode_resources"))


def test_encode_kernel_has_no_scratch_no_spills_and_no_lds(kernels):
    names = [n for n in kernels if n.startswith("_ZN3rtk%d%sE" % (len(KERNEL), KERNEL))]
    assert len(names) == 1, (KERNEL, sorted(kernels))
    res = kernels[names[0]]
    print(KERNEL, res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0, res
    assert int(res["SGPRs Spill"]) == 0, res
    assert int(res["LDS Size [bytes/block]"]) == 0, res
    assert int(res["Occupancy [waves/SIMD]"]) >= 8, res
