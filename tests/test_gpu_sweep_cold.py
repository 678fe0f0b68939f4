"""The node sweep of the sweep forms (k_pathtrace_sweep_plain, k_pathtrace_sweep_wide; csrc/k_traverse.hip.h traverse_leaves):
the walk a wave takes over the node records of csrc/scene_facts.h walk_facts when one of its rays has a non-finite reciprocal
direction or origin term, in place of the node walk that used to be inlined for it.  MI355RT_LEAF_SWEEP_GUARD=1 sends every
walk of a dispatch through it; without the variable the waves take it only when such a ray turns up.  Either way every image
and every ray counter must equal the oracle's bit for bit, and equal what the node-walk form gives (MI355RT_LEAF_SWEEP=0), and
rt_debug_pt_form must report a sweep form.

Cornell runs the plain sweep form, Cornell with one metal triangle the generic one; the uploaded BVHs are the shapes of
tests/sweep_trees.py over a small random mesh: a root that is a leaf, a root over two leaves, an inner node of three children
under a root of three, and the 31 nodes of a complete tree of 16 leaves.

A render cannot be made to produce a truly non-finite bounce ray on demand.  The arithmetic of such rays is pinned on the host
(tests/test_node_sweep_model.py: the node sweep against the reference's walk for zero, negative-zero and denormal direction
components, origins on box faces and faces at 0); the device loop is pinned here by the forced runs, where every ray of every
walk goes through it."""
import numpy as np
import pytest

import parity_util as pu
import sweep_trees
from test_gpu_leaf_sweep import _scene
from test_gpu_plain_materials import FRAMES, _check, _render

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (8, 8)]
DEPTHS = [1, 8]
BATCH = 2


def _sweep_and_node_walk(W, oracle_lib, monkeypatch, b, w, h, depth, guard, form=None):
    """`b` through a sweep form (every walk through the node sweep if `guard`) and through the node-walk form: both equal the
    oracle, and each other."""
    cpu = oracle_lib.OracleRenderer()
    pu.drive(cpu, W, b, w, h, depth, 1, FRAMES, present=False)
    W._build.build_rt()
    if guard:
        monkeypatch.setenv("MI355RT_LEAF_SWEEP_GUARD", "1")
    images = []
    for knob, want in ((None, "sweep"), ("0", "nodes")):
        if knob is not None:
            monkeypatch.setenv("MI355RT_LEAF_SWEEP", knob)
        r = _render(W, b, w, h, depth, 1, BATCH)
        try:
            assert r.debugPtWalk() == want
            got = r.debugPtForm()
            assert got == form if form else got in ("plain", "generic")
            images.append(_check(r, cpu, got, h))
        finally:
            r.destroy()
    assert np.array_equal(pu.bits(images[0]), pu.bits(images[1]))


@pytest.mark.parametrize("guard", [True, False], ids=["forced", "as_it_comes"])
@pytest.mark.parametrize("material", ["plain", "generic"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("w,h", SIZES)
def test_cornell_through_the_node_sweep(W, oracle_lib, monkeypatch, w, h, depth, material, guard):
    _sweep_and_node_walk(W, oracle_lib, monkeypatch, _scene(W, oracle_lib, material), w, h, depth, guard, form=material)


@pytest.mark.parametrize("guard", [True, False], ids=["forced", "as_it_comes"])
@pytest.mark.parametrize("kind", ["one", "three", "triple", "full16"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("w,h", SIZES)
def test_uploaded_trees_through_the_node_sweep(W, oracle_lib, monkeypatch, w, h, depth, kind, guard):
    _sweep_and_node_walk(W, oracle_lib, monkeypatch, sweep_trees.scene(kind), w, h, depth, guard)
