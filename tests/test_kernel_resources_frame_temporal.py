"""Register and LDS budget of the temporal stage's kernel (csrc/k_frame_temporal.hip.h): k_frame_temporal exists once in the
compiler's resource report of the gfx950 code object, uses no scratch memory, spills no register and takes no LDS; its register
count is the one the resource table of DESIGN.md section 4.3c states.  No GPU needed."""
import os
import re

import pytest

from test_kernel_resources import REPO, resource_report

NAME = "k_frame_temporal"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("frame_temporal_resources"))


def test_the_kernel_has_no_scratch_no_spills_and_no_lds(kernels):
    names = [n for n in kernels if n.startswith("_ZN3rtk%d%sE" % (len(NAME), NAME))]
    assert len(names) == 1, sorted(kernels)
    res = kernels[names[0]]
    print(NAME, res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0, res
    assert int(res["SGPRs Spill"]) == 0, res
    assert int(res["LDS Size [bytes/block]"]) == 0, res
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    m = re.search(r"^\| `k_frame_temporal` \| (\d+) \|", text, flags=re.M)
    assert m, "DESIGN.md has no resource row for k_frame_temporal"
    assert int(res["VGPRs"]) == int(m.group(1)), (res["VGPRs"], m.group(1))
    assert int(res["VGPRs"]) <= 128, "at least four waves per SIMD"
