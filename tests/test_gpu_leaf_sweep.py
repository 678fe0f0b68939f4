"""The sweep forms of the wide one-leaf path tracer (k_pathtrace_sweep_plain, k_pathtrace_sweep_wide, csrc/k_pathtrace.hip.h).
When the host has seen in the BLAS bytes of rt_upload_bvh a canonical pre-order tree of finite, nested boxes (csrc/scene_facts.h
walk_facts), both walks of a trip test the BLAS leaves alone, in wave lock-step (csrc/k_traverse.hip.h traverse_leaves).  Per
ray that is the node walk's arithmetic on the leaves the node walk reaches, so every image and every ray counter must equal the
oracle's bit for bit, and equal what the node-walk form gives when MI355RT_LEAF_SWEEP=0 switches the choice off;
rt_debug_pt_form says which form a dispatch took.

Cornell runs the plain sweep form, Cornell with one metal triangle the generic one.  MI355RT_LEAF_SWEEP_GUARD=1 sends every
walk through the branch a ray with a non-finite reciprocal direction takes.  A BVH that breaks a clause of the condition, and
a node array written on the device, must keep the node walk and still equal the oracle."""
import numpy as np
import pytest

import odd_bvh
import parity_util as pu
from test_gpu_plain_materials import FRAMES, _check, _cornell_with, _lambertian_in_view, _render
from test_gpu_world_records import _both, _same_images, _trace

pytestmark = pytest.mark.gpu


class _Rebuilt:
    """The bridge `b` with another BLAS array."""
    def __init__(self, b, blas):
        self._b = b
        self.blas = blas

    def __getattr__(self, name):
        return getattr(self._b, name)


def _cornell_blas(W):
    n = np.array(pu.bridge_for(W, "cornell").blas, np.float32).reshape(-1, 8).copy()
    return n, n.view(np.uint32)


def _scene(W, oracle_lib, material):
    b = pu.bridge_for(W, "cornell")
    return b if material == "plain" else _cornell_with(W, 7, 1.0, _lambertian_in_view(W, oracle_lib))


def _both_walks(W, oracle_lib, monkeypatch, b, w, h, depth, spp, batch, stripes=None, material="plain", walk="sweep"):
    """`b` through a context with the choice on (which must walk as `walk` says) and one created with the knob off."""
    cpu = oracle_lib.OracleRenderer()
    if stripes:
        cpu.setStripes(*stripes)
    pu.drive(cpu, W, b, w, h, depth, spp, FRAMES, present=False)
    W._build.build_rt()
    images = []
    for knob, want in ((None, walk), ("0", "nodes")):
        if knob is not None:
            monkeypatch.setenv("MI355RT_LEAF_SWEEP", knob)
        r = _render(W, b, w, h, depth, spp, batch, stripes)
        try:
            assert r.debugPtWalk() == want
            images.append(_check(r, cpu, material, h, stripes))
        finally:
            r.destroy()
    assert np.array_equal(pu.bits(images[0]), pu.bits(images[1]))


# 8 x 8 and 5 x 3 are one tile, 37 x 29 twenty; every size with depth 1, 2 and 8, both sample counts and both batch sizes
CASES = [(8, 8, 8, 1, 2), (8, 8, 1, 2, 4), (8, 8, 2, 2, 2), (5, 3, 8, 2, 2), (5, 3, 2, 1, 4), (5, 3, 1, 1, 2),
         (37, 29, 8, 1, 4), (37, 29, 8, 2, 2), (37, 29, 1, 1, 2), (37, 29, 2, 2, 4)]


@pytest.mark.parametrize("material", ["plain", "generic"])
@pytest.mark.parametrize("w,h,depth,spp,batch", CASES)
def test_cornell_sweep_forms_equal_the_oracle_and_the_node_walk(W, oracle_lib, monkeypatch, w, h, depth, spp, batch, material):
    _both_walks(W, oracle_lib, monkeypatch, _scene(W, oracle_lib, material), w, h, depth, spp, batch, material=material)


@pytest.mark.parametrize("material", ["plain", "generic"])
def test_cornell_sweep_forms_on_a_striped_rank(W, oracle_lib, monkeypatch, material):
    _both_walks(W, oracle_lib, monkeypatch, _scene(W, oracle_lib, material), 21, 67, 8, 1, 2, stripes=(8, 1, 3), material=material)


@pytest.mark.parametrize("material", ["plain", "generic"])
def test_every_walk_through_the_guards_branch(W, oracle_lib, monkeypatch, material):
    monkeypatch.setenv("MI355RT_LEAF_SWEEP_GUARD", "1")
    _both_walks(W, oracle_lib, monkeypatch, _scene(W, oracle_lib, material), 37, 29, 8, 2, 2, material=material)


def test_the_diamond_scene_keeps_the_node_walk(W, oracle_lib, gpu_renderer):
    """Two instances under a three-node TLAS: not a one-leaf scene, whatever its BLASes look like."""
    b = pu.bridge_for(W, "viewer_diamond")
    cpu = oracle_lib.OracleRenderer()
    pu.drive(cpu, W, b, 9, 9, 8, 1, FRAMES, present=False)
    r = gpu_renderer
    r.setKernelVariant(1)
    r.buildPipeline(8, 1)
    W.upload_scene(r, b, 9, 9)
    r.setCounting(False)
    r.resetCounters()
    _trace(r, FRAMES, 4)
    assert r.debugPtWalk() == "nodes" and r.debugPtForm() == "generic"
    _same_images(r, cpu, "viewer_diamond")


def _single_child(W):
    n, u = _cornell_blas(W)
    assert odd_bvh._make_single(u, 0, 0, False)   # the root keeps its first child alone
    return n


def _empty_leaf(W):
    n, u = _cornell_blas(W)
    u[9, 7] &= ~np.uint32(7)
    assert u[9, 7] != 0
    return n


def _shrunk_inner_box(W):
    n, u = _cornell_blas(W)
    assert u[1, 7] == 0 and n[1, 4] > n[1, 0]
    n[1, 4] = n[1, 0] + np.float32(0.75) * (n[1, 4] - n[1, 0])   # cuts into its children's boxes
    kids = [i for i in range(2, int(u[1, 3])) if n[i, 4] > n[1, 4]]
    assert kids
    return n


@pytest.mark.parametrize("make", [_single_child, _empty_leaf, _shrunk_inner_box])
def test_a_bvh_that_breaks_the_condition_keeps_the_node_walk(W, oracle_lib, monkeypatch, make):
    b = _Rebuilt(pu.bridge_for(W, "cornell"), make(W).reshape(-1))
    _both_walks(W, oracle_lib, monkeypatch, b, 37, 29, 8, 1, 4, walk="nodes")


def test_the_walk_facts_follow_the_scene(W, oracle_lib, gpu_renderer):
    """Cornell (sweep), its BLAS again with a count-0 leaf (nodes), the first BLAS again (sweep), then a device-resident world
    update, whose nodes the host never sees (nodes): one renderer, one oracle, the same sequence."""
    w, h, depth, batch = 40, 30, 8, 4
    b = pu.bridge_for(W, "cornell")
    gpu, cpu = gpu_renderer, oracle_lib.OracleRenderer()
    gpu.setKernelVariant(1)
    for r in (gpu, cpu):
        r.buildPipeline(depth, 1)
        W.upload_scene(r, b, w, h)
    gpu.setCounting(False)
    _both(gpu, cpu, lambda r: r.resetCounters())

    def trace(walk, what):
        _both(gpu, cpu, lambda r: _trace(r, FRAMES, batch))
        assert gpu.debugPtWalk() == walk, what
        assert gpu.debugPtLaunch()["threads"] == 512, what
        _same_images(gpu, cpu, what)

    def upload(bridge):
        _both(gpu, cpu, lambda r: (W.upload_scene(r, bridge, w, h), r.resetAccumulation()))

    trace("sweep", "cornell")
    upload(_Rebuilt(b, _empty_leaf(W).reshape(-1)))
    trace("nodes", "a leaf of no triangles")
    upload(b)
    trace("sweep", "cornell again")

    dev_b, host_b = W.WorldBridge(), W.WorldBridge()
    dev_b.setDeviceUpdater(gpu)
    dev_b.loadScene("cornell")
    host_b.loadScene("cornell")
    dev_b.update(0.25)
    host_b.update(0.25)
    assert dev_b.deviceResident, dev_b.deviceWarning
    assert len(gpu.worldRead("tlas")) // 8 == 1, "not a one-leaf world"
    W.upload_scene(cpu, host_b, w, h)   # the host path's arrays for the oracle; the renderer already holds its own
    dev_b.updateCamera(w, h)
    gpu.updateSceneUniforms(dev_b.cameraData, 0, dev_b.lightCount)
    gpu.resetAccumulation()
    trace("nodes", "after the device world update")
