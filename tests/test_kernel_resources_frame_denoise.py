"""Register and LDS budget of the frame-denoise kernels (csrc/k_frame_denoise.hip.h): each exists once in the compiler's resource
report of the gfx950 code object - k_frame_pass_lds once per spacing 1 .. 4 - uses no scratch memory and spills no register.
The LDS of each staged instantiation is the window of ITS spacing, (32 + 4 S) * (8 + 4 S) cells of twelve words: the figure of
the resource table of DESIGN.md section 4.3b; the other kernels use none.  No GPU needed."""
import os
import re

import pytest

from test_kernel_resources import REPO, resource_report

PLAIN = ("k_frame_prepare", "k_frame_pass_direct", "k_frame_finish")
STEPS = (1, 2, 3, 4)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("frame_denoise_resources"))


def stated_lds(step):
    """the LDS bytes of k_frame_pass_lds<step> in the resource table of DESIGN.md 4.3b: | `k_frame_pass_lds<S>` | ... | N B |"""
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    m = re.search(r"^\| `k_frame_pass_lds<%d>` \|.*?\| (\d+) B \|" % step, text, flags=re.M)
    assert m, "DESIGN.md has no resource row for k_frame_pass_lds<%d>" % step
    return int(m.group(1))


def clean(res):
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0, res
    assert int(res["SGPRs Spill"]) == 0, res


@pytest.mark.parametrize("name", PLAIN)
def test_unstaged_kernels_have_no_scratch_no_spills_and_no_lds(kernels, name):
    names = [n for n in kernels if n.startswith("_ZN3rtk%d%sE" % (len(name), name))]
    assert len(names) == 1, (name, sorted(kernels))
    res = kernels[names[0]]
    print(name, res)
    clean(res)
    assert int(res["LDS Size [bytes/block]"]) == 0, res


@pytest.mark.parametrize("step", STEPS)
def test_staged_instantiations_take_the_lds_of_their_window(kernels, step):
    names = [n for n in kernels if n.startswith("_ZN3rtk16k_frame_pass_ldsILi%dEE" % step)]
    assert len(names) == 1, (step, sorted(kernels))
    res = kernels[names[0]]
    print(step, res)
    clean(res)
    lds = int(res["LDS Size [bytes/block]"])
    assert lds == (32 + 4 * step) * (8 + 4 * step) * 48 == stated_lds(step), (lds, stated_lds(step))
    assert 160 * 1024 // lds >= 2, "two workgroups per CU at the largest window"
