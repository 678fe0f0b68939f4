"""Background pixels in the persistent path tracer (csrc/k_pathtrace_persistent.hip.h).  A lane that takes a pixel reads its
G-buffer depth in the refill; a background pixel (or every pixel at MAX_DEPTH = 0) is finished there with colour +0 and the
lane takes the next slot, so no lane trip carries a background sample.  Cornell seen three ways: the stock view at an odd
size, a view moved sideways so that the box edges cut through many 8x8 tiles, and a view facing away from the box (every
pixel background).  Each runs as a batch of 4 frames (the 512-thread form in the product build) and one frame per dispatch
(the 256-thread form), in the counting and the product build, against the oracle bit for bit: accumulation buffer,
G-buffer and the counters (all six in the counting build, the three ray counters in the product build)."""
import numpy as np
import pytest

import parity_util as pu

pytestmark = pytest.mark.gpu

W_, H_ = 203, 117
FRAMES = (1, 2, 3, 4)
RAYS = pu.RAY_COUNTERS
VIEWS = ("stock", "mixed", "away")
# (spp, depth, stripes): stripes = (rows, rank, count); 8 rows is the tile-aligned form, 1 row the per-row test
CASES = [(1, 8, None), (3, 8, None), (1, 0, None), (3, 8, (8, 1, 3)), (1, 8, (1, 0, 2))]


def _camera(b, view):
    """24 floats: origin, lower_left, horizontal, vertical, u, v (4 each) of the bridge's camera at W_ x H_."""
    cam = np.array(b.cameraData, dtype=np.float32).reshape(6, 4).copy()
    o, ll, h, v = cam[0, :3].copy(), cam[1, :3].copy(), cam[2, :3].copy(), cam[3, :3].copy()
    if view == "mixed":        # half a box width to the right: one side wall and the open side cut through the tiles
        shift = np.float32(0.6)
        cam[0, 0] += shift
        cam[1, 0] += shift
    elif view == "away":       # every ray reversed: d'(u, v) = -d(u, v)
        cam[1, :3] = 2 * o - ll
        cam[2, :3] = -h
        cam[3, :3] = -v
    return cam.reshape(-1)


def _drive(r, W, b, view, spp, depth, stripes, batch, counting):
    if stripes:
        r.setStripes(*stripes)
    if hasattr(r, "setKernelVariant"):
        r.setKernelVariant(1)
    r.buildPipeline(depth, spp)
    W.upload_scene(r, b, W_, H_)
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


def _check_view(view, depth_plane):
    """The view is what its name says (the oracle's G-buffer of the last frame)."""
    bg = np.asarray(depth_plane).reshape(H_, W_) >= 1.0
    if view == "away":
        assert bg.all()
        return
    tiles = np.pad(bg, ((0, -H_ % 8), (0, -W_ % 8)), constant_values=True).reshape(-(-H_ // 8), 8, -(-W_ // 8), 8)
    per_tile = tiles.sum(axis=(1, 3))
    mixed = int(((per_tile > 0) & (per_tile < 64)).sum())
    assert 0.1 < bg.mean() < 0.9 and mixed >= 20, (bg.mean(), mixed)


@pytest.mark.parametrize("counting", [True, False], ids=["counting", "product"])
@pytest.mark.parametrize("batch", [4, 1], ids=["batch4", "single"])
@pytest.mark.parametrize("spp,depth,stripes", CASES)
@pytest.mark.parametrize("view", VIEWS)
def test_background_pixels(W, oracle_lib, view, spp, depth, stripes, batch, counting):
    b = pu.bridge_for(W, "cornell")
    cpu = oracle_lib.OracleRenderer()
    _drive(cpu, W, b, view, spp, depth, stripes, 1, True)
    gbuf = cpu.readGBuffer()
    if not stripes:            # (a rank's G-buffer holds its own rows only)
        _check_view(view, gbuf[2])
    r = W.WebGPURenderer(0)
    try:
        _drive(r, W, b, view, spp, depth, stripes, batch, counting)
        L = r.debugPtLaunch()
        assert L["threads"] == (512 if (batch > 1 and not counting) else 256), L
        gc, cc = r.getCounters(), cpu.getCounters()
        if counting:
            assert gc == cc
        else:
            assert {k: gc[k] for k in RAYS} == {k: cc[k] for k in RAYS}
        part, want = r.readAccum(), cpu.readAccum()
        if stripes:
            rows, rank, count = stripes
            owned = (np.arange(H_) // rows) % count == rank
            assert not part[~owned].any(), "rank %d wrote outside its rows" % rank
            assert np.array_equal(pu.bits(part[owned]), pu.bits(want[owned])), \
                pu.describe_mismatch("rank %d owned rows" % rank, part[owned], want[owned])
        else:
            assert np.array_equal(pu.bits(part), pu.bits(want)), pu.describe_mismatch("accumulation buffer", part, want)
            for name, g, c in zip(("albedo", "normal_id", "depth"), r.readGBuffer(), gbuf):
                assert np.array_equal(pu.bits(g), pu.bits(c)), pu.describe_mismatch("G-buffer " + name, g, c)
    finally:
        r.destroy()
