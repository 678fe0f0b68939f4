"""One surface-frame pass per trip in the one-leaf forms of the persistent path tracer (csrc/k_pathtrace_persistent.hip.h).
A lane whose extension ray found a hit only records the hit; a lane that starts a sample only makes its camera ray and loads
its G-buffer words; then one call of setup_surface serves both kinds, with `from_gbuffer` a lane condition.  Per lane the
arithmetic is what the two separate calls did, so everything must stay bit-identical to the oracle: accumulation buffer, the
three G-buffer planes and the counters (all six in the counting build, the three ray counters in the product build).

The shapes are the smallest at which the pass can go wrong: 37 x 29 (partial tiles on both edges, few tickets, so waves
drain while others still refill), 8 x 8 and 5 x 3 (one wave: its first trip has new samples only, its last trips new hits
only), depth 1 (no extension ray at all: only G-buffer lanes), several samples per pixel (a sample restarts on a pixel the
lane keeps), views with few live pixels per tile or none, a textured scene under a rotation and a non-uniform scale (texture
coordinates interpolated for both kinds of lane in the one pass, the normal map for the new hits), and a striped rank.
Each case asserts the launch shape, so the intended form (512 threads for a batch in the product build, else 256) ran."""
import numpy as np
import pytest

import parity_util as pu
from test_gpu_one_leaf_occupancy import dyn_lds
from test_gpu_one_leaf_wide import COL_PARK, LDS_PER_CU, WAVE_QUEUE
from test_gpu_world_records import _one_leaf, _rotated_scaled

pytestmark = pytest.mark.gpu

FRAMES = (1, 2, 3, 4)
RAYS = pu.RAY_COUNTERS
_scenes = {}
_oracle = {}   # case -> (accum, gbuffer planes, counters) of the oracle, computed once and left unchanged


def _camera(b, view):
    """The bridge's camera (24 floats: origin, lower_left, horizontal, vertical, u, v), moved as the view says."""
    cam = np.array(b.cameraData, dtype=np.float32).reshape(6, 4).copy()
    o, ll, h, v = cam[0, :3].copy(), cam[1, :3].copy(), cam[2, :3].copy(), cam[3, :3].copy()
    if view == "mixed":        # half a box width to the right: one side wall and the open side cut through the tiles
        cam[0, 0] += np.float32(0.6)
        cam[1, 0] += np.float32(0.6)
    elif view == "away":       # every ray reversed: each pixel is background
        cam[1, :3] = 2 * o - ll
        cam[2, :3] = -h
        cam[3, :3] = -v
    return cam.reshape(-1)


def _textured(W):
    """One instance of 30 triangles with texture indices, under a rotation times a non-uniform scale."""
    if "textured" not in _scenes:
        b = _rotated_scaled(_one_leaf(1, 30, with_textures=True), 12)
        tex = np.asarray(b.mesh_topology, np.uint32).reshape(-1, 20).view(np.float32)[:, 12:16]
        assert (tex[:, 0] > -0.5).any() and (tex[:, 2] > -0.5).any(), "no base-colour or no normal-map texture in the scene"
        _scenes["textured"] = b
    return _scenes["textured"]


def _bridge(W, scene):
    return pu.bridge_for(W, "cornell") if scene == "cornell" else _textured(W)


def _drive(r, W, b, scene, view, w, h, spp, depth, stripes, batch, counting):
    if stripes:
        r.setStripes(*stripes)
    if hasattr(r, "setKernelVariant"):
        r.setKernelVariant(1)
    r.buildPipeline(depth, spp)
    W.upload_scene(r, b, w, h)
    if scene == "cornell" and view != "stock":
        r.updateSceneUniforms(_camera(b, view), 0, b.lightCount)
        r.resetAccumulation()
    if hasattr(r, "setCounting"):
        r.setCounting(counting)
    r.resetCounters()
    for i in range(0, len(FRAMES), batch):
        if batch == 1:
            r.compute(FRAMES[i])
        else:
            r.computeBatch(list(FRAMES[i:i + batch]))
    r.sync()


def _want(W, oracle_lib, scene, view, w, h, spp, depth, stripes):
    key = (scene, view, w, h, spp, depth, stripes)
    if key not in _oracle:
        cpu = oracle_lib.OracleRenderer()
        _drive(cpu, W, _bridge(W, scene), scene, view, w, h, spp, depth, stripes, 1, True)
        acc, gbuf = cpu.readAccum().copy(), [np.array(g).copy() for g in cpu.readGBuffer()]
        for a in [acc] + gbuf:
            a.setflags(write=False)
        bg = gbuf[2].reshape(h, w) >= 1.0
        if not stripes:            # (a rank's G-buffer holds its own rows only)
            if view == "away":
                assert bg.all()
            elif view == "mixed":
                tiles = np.pad(bg, ((0, -h % 8), (0, -w % 8)), constant_values=True)
                per_tile = tiles.reshape(-(-h // 8), 8, -(-w // 8), 8).sum(axis=(1, 3))
                assert 0.1 < bg.mean() < 0.9 and int(((per_tile > 0) & (per_tile < 64)).sum()) >= 4, bg.mean()
            else:
                assert not bg.all(), "the view sees nothing"
        _oracle[key] = (acc, gbuf, dict(cpu.getCounters()))
    return _oracle[key]


def _compare(W, oracle_lib, scene, view, w, h, spp, depth, stripes, batch, counting, wide_fits=True):
    want, gbuf, cc = _want(W, oracle_lib, scene, view, w, h, spp, depth, stripes)
    r = W.WebGPURenderer(0)
    try:
        _drive(r, W, _bridge(W, scene), scene, view, w, h, spp, depth, stripes, batch, counting)
        L = r.debugPtLaunch()
        assert L["threads"] == (512 if (batch > 1 and not counting and wide_fits) else 256), L
        gc = r.getCounters()
        if counting:
            assert gc == cc
        else:
            assert {k: gc[k] for k in RAYS} == {k: cc[k] for k in RAYS}
        part = r.readAccum()
        if stripes:
            rows, rank, count = stripes
            owned = (np.arange(h) // rows) % count == rank
            assert not part[~owned].any(), "rank %d wrote outside its rows" % rank
            assert np.array_equal(pu.bits(part[owned]), pu.bits(want[owned])), \
                pu.describe_mismatch("rank %d owned rows" % rank, part[owned], want[owned])
        else:
            assert np.array_equal(pu.bits(part), pu.bits(want)), pu.describe_mismatch("accumulation buffer", part, want)
            for name, g, c in zip(("albedo", "normal_id", "depth"), r.readGBuffer(), gbuf):
                assert np.array_equal(pu.bits(g), pu.bits(c)), pu.describe_mismatch("G-buffer " + name, g, c)
    finally:
        r.destroy()


MODES = pytest.mark.parametrize("counting", [True, False], ids=["counting", "product"])
BATCH = pytest.mark.parametrize("batch", [4, 1], ids=["batch4", "single"])


@MODES
@BATCH
@pytest.mark.parametrize("depth", [8, 2, 1])
@pytest.mark.parametrize("spp", [1, 3])
def test_cornell_odd_size(W, oracle_lib, spp, depth, batch, counting):
    _compare(W, oracle_lib, "cornell", "stock", 37, 29, spp, depth, None, batch, counting)


@MODES
@BATCH
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("w,h", [(8, 8), (5, 3)])
def test_cornell_one_wave(W, oracle_lib, w, h, spp, batch, counting):
    _compare(W, oracle_lib, "cornell", "stock", w, h, spp, 8, None, batch, counting)


@MODES
@BATCH
@pytest.mark.parametrize("view", ["mixed", "away"])
def test_cornell_sparse_views(W, oracle_lib, view, batch, counting):
    _compare(W, oracle_lib, "cornell", view, 37, 29, 1, 8, None, batch, counting)


@MODES
@BATCH
def test_textured_transformed_instance(W, oracle_lib, batch, counting):
    b = _textured(W)
    wide = dyn_lds(b) + 4 * WAVE_QUEUE + 8 * COL_PARK <= LDS_PER_CU // 3
    assert wide, "the scene was meant to take the wide form"
    _compare(W, oracle_lib, "textured", "stock", 37, 29, 1, 8, None, batch, counting, wide_fits=wide)


@BATCH
def test_striped_rank(W, oracle_lib, batch):
    _compare(W, oracle_lib, "cornell", "stock", 37, 29, 1, 8, (8, 1, 3), batch, False)
