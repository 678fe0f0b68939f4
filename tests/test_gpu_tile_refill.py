"""The tile prepass of the wide one-leaf persistent path tracer (csrc/k_pathtrace_persistent.hip.h, PREPASS). A wave that
takes a ticket tests the depth of all 64 slots of the 8x8 tile at once, lane i for slot i, finishes the background pixels there and
keeps the ballot of the others; a refill hands the r-th set bit to the r-th needy lane. Cornell at the smallest shapes where
that can go wrong: 8x8 (exactly one tile), 5x3 (one tile, mostly outside the image), 9x9 (four tiles, three of them an edge
row or column), 37x29 (ragged on both edges, several tiles per wave). Views: stock; "mixed" and "away" of
tests/test_gpu_background_tiles.py (tiles with both kinds of pixel; all background, so no ticket leaves a live slot);
"inside", the camera moved into the box so that no pixel is background; "one", moved sideways until some tile keeps exactly
one live pixel. Each runs as a batch of 3 frames (the 512-thread form in the product build) and one frame per dispatch (the
256-thread form, which keeps the cursor refill), in the counting and the product build, some with stripes (tile-aligned, and
per row, where the ownership test cuts inside a tile), against the oracle bit for bit: accumulation buffer, G-buffer and the
counters (all six in the counting build, the three ray counters in the product build). Sizes are paired with views, not
multiplied: 28 cases, four GPU runs each."""
import numpy as np
import pytest

import parity_util as pu
from test_gpu_background_tiles import RAYS, _camera

pytestmark = pytest.mark.gpu

FRAMES = (1, 2, 3)
PIPES = [(1, 8), (3, 2), (1, 0), (2, 1)]            # (spp, depth)
STRIPES = [(8, 1, 3), (1, 0, 2)]                    # (rows, rank, count): tile-aligned; per row
ONE_SHIFT = {(9, 9): 1.5, (37, 29): 1.45}           # sideways move that leaves some tile one live pixel (asserted below)
# (size, view, index into PIPES): every pipeline case at every size, depth 8 where one tile or one pixel is the point
PAIRS = [((8, 8), "stock", 0), ((8, 8), "away", 2), ((8, 8), "inside", 1), ((8, 8), "stock", 3),
         ((5, 3), "stock", 3), ((5, 3), "mixed", 0), ((5, 3), "away", 1), ((5, 3), "mixed", 2),
         ((9, 9), "stock", 1), ((9, 9), "mixed", 3), ((9, 9), "one", 0), ((9, 9), "inside", 2),
         ((37, 29), "stock", 0), ((37, 29), "away", 0), ((37, 29), "inside", 1), ((37, 29), "one", 0),
         ((37, 29), "mixed", 0), ((37, 29), "mixed", 1), ((37, 29), "mixed", 2), ((37, 29), "mixed", 3)]
STRIPED = [((9, 9), "mixed"), ((37, 29), "stock"), ((37, 29), "mixed"), ((37, 29), "one")]


def _cases():
    out = [(size, view, PIPES[k], None) for size, view, k in PAIRS]
    for i, (size, view) in enumerate(STRIPED):      # both stripe forms where tiles hold both kinds of pixel
        for j, st in enumerate(STRIPES):
            out.append((size, view, PIPES[(i + j) % 2], st))   # (1, 8) or (3, 2): a depth that traces
    return out


CASES = _cases()


def _case_id(c):
    (w, h), view, (spp, depth), st = c
    return "%dx%d-%s-spp%d-d%d-%s" % (w, h, view, spp, depth, "x".join(map(str, st)) if st else "whole")


def _view_camera(b, size, view):
    """24 floats of the camera of `view` at the size the bridge was last uploaded at."""
    if view in ("stock", "mixed", "away"):
        return _camera(b, view)
    cam = np.array(b.cameraData, dtype=np.float32).reshape(6, 4).copy()
    if view == "inside":     # 1.5 along the viewing axis (the stock origin is 2.4 in front of the box's centre)
        o, ll, h, v = (cam[k, :3].copy() for k in range(4))
        fwd = ll + h / 2 + v / 2 - o
        step = (np.float32(1.5) * fwd / np.linalg.norm(fwd)).astype(np.float32)
        cam[0, :3] += step
        cam[1, :3] += step
    else:                    # "one"
        shift = np.float32(ONE_SHIFT[size])
        cam[0, 0] += shift
        cam[1, 0] += shift
    return cam.reshape(-1)


def _drive(r, W, b, size, view, spp, depth, stripes, batch, counting):
    if stripes:
        r.setStripes(*stripes)
    if hasattr(r, "setKernelVariant"):
        r.setKernelVariant(1)
    r.buildPipeline(depth, spp)
    W.upload_scene(r, b, size[0], size[1])
    r.updateSceneUniforms(_view_camera(b, size, view), 0, b.lightCount)
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


def _live_per_tile(depth_plane, size):
    w, h = size
    live = ~(np.asarray(depth_plane).reshape(h, w) >= 1.0)
    tiles = np.pad(live, ((0, -h % 8), (0, -w % 8)), constant_values=False).reshape(-(-h // 8), 8, -(-w // 8), 8)
    return live, tiles.sum(axis=(1, 3))


def _check_view(size, view, depth_plane):
    """The view is what its name says (the oracle's depth plane of the last frame, whole image)."""
    live, per_tile = _live_per_tile(depth_plane, size)
    if view == "away":
        assert not live.any()
    elif view == "inside":
        assert live.all()
    elif view == "mixed":
        assert live.any() and not live.all(), live.mean()
    elif view == "one":
        w, h = size
        inside = np.pad(np.ones((h, w), bool), ((0, -h % 8), (0, -w % 8)))
        in_image = inside.reshape(-(-h // 8), 8, -(-w // 8), 8).sum(axis=(1, 3))
        assert ((per_tile == 1) & (in_image >= 2)).any(), per_tile


_oracle = {}   # case -> (counters, accumulation buffer, G-buffer): computed once, shared by the four GPU runs of the case


def _reference(W, oracle_lib, b, case):
    key = _case_id(case)
    if key not in _oracle:
        size, view, (spp, depth), stripes = case
        whole = oracle_lib.OracleRenderer()
        _drive(whole, W, b, size, view, 1, 1, None, 1, True)
        _check_view(size, view, whole.readGBuffer()[2])
        cpu = oracle_lib.OracleRenderer()
        _drive(cpu, W, b, size, view, spp, depth, stripes, 1, True)
        acc = cpu.readAccum().copy()
        acc.setflags(write=False)
        _oracle[key] = (cpu.getCounters(), acc, [np.array(g) for g in cpu.readGBuffer()])
    return _oracle[key]


@pytest.mark.parametrize("counting", [True, False], ids=["counting", "product"])
@pytest.mark.parametrize("batch", [3, 1], ids=["batch3", "single"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_tile_refill(W, oracle_lib, case, batch, counting):
    size, view, (spp, depth), stripes = case
    b = pu.bridge_for(W, "cornell")
    cc, want, gbuf = _reference(W, oracle_lib, b, case)
    r = W.WebGPURenderer(0)
    try:
        _drive(r, W, b, size, view, spp, depth, stripes, batch, counting)
        L = r.debugPtLaunch()
        assert L["threads"] == (512 if (batch > 1 and not counting) else 256), L
        gc = r.getCounters()
        if counting:
            assert gc == cc
        else:
            assert {k: gc[k] for k in RAYS} == {k: cc[k] for k in RAYS}
        part = r.readAccum()
        if stripes:
            rows, rank, count = stripes
            owned = (np.arange(size[1]) // rows) % count == rank
            assert not part[~owned].any(), "rank %d wrote outside its rows" % rank
            assert np.array_equal(pu.bits(part[owned]), pu.bits(want[owned])), \
                pu.describe_mismatch("rank %d owned rows" % rank, part[owned], want[owned])
        else:
            assert np.array_equal(pu.bits(part), pu.bits(want)), pu.describe_mismatch("accumulation buffer", part, want)
            for name, g, c in zip(("albedo", "normal_id", "depth"), r.readGBuffer(), gbuf):
                assert np.array_equal(pu.bits(g), pu.bits(c)), pu.describe_mismatch("G-buffer " + name, g, c)
    finally:
        r.destroy()
