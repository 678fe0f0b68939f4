"""Register and LDS budget of the atlas-denoise kernels (k_denoise_index / k_denoise_pass, csrc/k_denoise.hip.h): each exists
once in the compiler's resource report of the gfx950 code object, uses no scratch memory and spills no VGPR.  k_denoise_pass
keeps its eleven window planes in LDS, at most the figure DESIGN.md section 4.1k states for it; k_denoise_index uses none.  No
GPU needed."""
import os
import re

import pytest

from test_kernel_resources import REPO, resource_report

KERNELS = ("k_denoise_index", "k_denoise_pass")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("denoise_resources"))


def stated_lds():
    """the LDS bytes of k_denoise_pass in the resource table of DESIGN.md 4.1k: | `k_denoise_pass` | VGPRs | ... | LDS | """
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    m = re.search(r"^\| `k_denoise_pass` \|.*?\| (\d+) B \|", text, flags=re.M)
    assert m, "DESIGN.md has no resource row for k_denoise_pass"
    return int(m.group(1))


@pytest.mark.parametrize("name", KERNELS)
def test_denoise_kernel_has_no_scratch_and_no_spills(kernels, name):
    names = [n for n in kernels if n.startswith("_ZN3rtk%d%sE" % (len(name), name))]
    assert len(names) == 1, (name, sorted(kernels))
    res = kernels[names[0]]
    print(name, res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0, res
    assert int(res["SGPRs Spill"]) == 0, res
    lds = int(res["LDS Size [bytes/block]"])
    if name == "k_denoise_index":
        assert lds == 0, res
    else:
        assert 0 < lds <= stated_lds(), (lds, stated_lds())
        assert 160 * 1024 // lds >= 3, "three workgroups per CU"
