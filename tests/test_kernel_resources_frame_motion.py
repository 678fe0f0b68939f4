"""Register and LDS budget of frame motion's kernels (csrc/k_frame_motion.hip.h and the second instantiation of the temporal
stage's body in csrc/k_frame_temporal.hip.h): each exists once in the compiler's resource report of the gfx950 code object, uses
no scratch memory, spills no register and takes no LDS; the register counts are those of the resource table of DESIGN.md section
4.3d; and k_frame_temporal, the instantiation without the flag, has the count section 4.3c has stated since before the flag
existed.  No GPU needed."""
import os
import re

import pytest

from test_kernel_resources import REPO, resource_report

NAMES = ("k_frame_motion", "k_frame_motion_scatter", "k_frame_temporal_motion")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("frame_motion_resources"))


def _one(kernels, name):
    names = [n for n in kernels if n.startswith("_ZN3rtk%d%sE" % (len(name), name))]
    assert len(names) == 1, (name, sorted(kernels))
    return kernels[names[0]]


@pytest.mark.parametrize("name", NAMES)
def test_no_scratch_no_spills_no_lds_and_the_documented_registers(kernels, name):
    res = _one(kernels, name)
    print(name, res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0, res
    assert int(res["SGPRs Spill"]) == 0, res
    assert int(res["LDS Size [bytes/block]"]) == 0, res
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    sec = text[text.index("4.3d"):]
    m = re.search(r"^\| `%s` \| (\d+) \|" % name, sec, flags=re.M)
    assert m, "DESIGN.md 4.3d has no resource row for " + name
    assert int(res["VGPRs"]) == int(m.group(1)), (res["VGPRs"], m.group(1))
    assert int(res["VGPRs"]) <= 128, "at least four waves per SIMD"


def test_the_instantiation_without_the_flag_keeps_the_parents_count(kernels):
    res = _one(kernels, "k_frame_temporal")
    assert int(res["VGPRs"]) == 79, "DESIGN.md 4.3c, measured before the body became a template"
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    m = re.search(r"^\| `k_frame_temporal` \| (\d+) \|", text, flags=re.M)
    assert m and int(m.group(1)) == 79
    assert int(res["ScratchSize [bytes/lane]"]) == 0 and int(res["LDS Size [bytes/block]"]) == 0
