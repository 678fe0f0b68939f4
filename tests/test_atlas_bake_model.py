"""The yardstick of the atlas bakes held to paper: atlas_bake_util.compose - identity (B) of include/mi355rt.h, the
composition of single-instance model bakes - on the hand-worked case "quad_diagonal" of bake_util.hand_cases, whose owner
map is written out there.  No GPU needed."""
import numpy as np
import pytest

import atlas_bake_util as au
import bake_util as bu
import random_scene

W_ATLAS, H_ATLAS, PAD = 20, 9, 700


@pytest.fixture(scope="module")
def scene(W):
    b = random_scene.make(1)
    return b, bu.model_for(W, b)


def _quad(scene):
    """(override layout, the written 8 x 8 owner map in global triangle indices)"""
    bridge, _ = scene
    tri_uvs, width, height, want = bu.hand_cases()["quad_diagonal"]
    assert (width, height) == (8, 8)
    first, _ = bu.instance_triangles(bridge, 0)
    return bu.hand_uv(bridge, 0, tri_uvs), np.asarray(want) + first


def test_two_disjoint_rectangles(scene):
    _, model = scene
    uv, quad = _quad(scene)
    entries = [(0, 1, 0, 8, 8), (0, 11, 1, 8, 8)]
    points, texels, owner, contested = au.compose(model, entries, W_ATLAS, H_ATLAS, t_max=2.0, pad_base=PAD, atlas_uv=uv)
    want = np.full((H_ATLAS, W_ATLAS, 2), -1, np.int64)
    for e, (_, x, y, w, h) in enumerate(entries):
        want[y:y + h, x:x + w, 0] = e
        want[y:y + h, x:x + w, 1] = quad
    assert owner.tolist() == want.tolist()
    assert contested == 0
    ys, xs = np.nonzero(want[:, :, 0] >= 0)
    assert np.array_equal(texels, ys * W_ATLAS + xs) and len(texels) == 128
    assert np.array_equal(points.view(np.uint32)[:, 7], PAD + ys * W_ATLAS + xs)      # pad_base + Y * W + X
    assert (points[:, 3] == np.float32(2.0)).all()
    # the two rectangles hold the same points, their pads apart
    local = model.bakePoints(0, 8, 8, t_max=2.0, pad_base=0, atlas_uv=uv)[0]
    for e in (0, 1):
        mine = points[owner.reshape(-1, 2)[texels, 0] == e]
        assert np.array_equal(mine.view(np.uint32)[:, 0:7], local.view(np.uint32)[:, 0:7])


def test_two_overlapping_rectangles(scene):
    _, model = scene
    uv, quad = _quad(scene)
    entries = [(0, 6, 1, 8, 8), (0, 2, 0, 8, 8)]      # columns 6 .. 9 of rows 1 .. 7 lie in both
    points, texels, owner, contested = au.compose(model, entries, W_ATLAS, H_ATLAS, pad_base=PAD, atlas_uv=uv)
    want = np.full((H_ATLAS, W_ATLAS, 2), -1, np.int64)
    for e in (1, 0):                                   # entry 0 written last: it wins
        _, x, y, w, h = entries[e]
        want[y:y + h, x:x + w, 0] = e
        want[y:y + h, x:x + w, 1] = quad
    assert owner.tolist() == want.tolist()
    assert (owner[1:8, 6:10, 0] == 0).all()
    assert contested == 7 * 4
    assert np.array_equal(points.view(np.uint32)[:, 7], PAD + texels)


def test_a_single_whole_atlas_entry_is_bake_points(scene):
    bridge, model = scene
    for inst, uv in ((0, None), (1, bu.grid_uv(bridge, 1))):
        want = model.bakePoints(inst, 37, 19, t_max=3.0, pad_base=11, atlas_uv=uv)
        points, texels, owner, contested = au.compose(model, [(inst, 0, 0, 37, 19)], 37, 19, t_max=3.0, pad_base=11, atlas_uv=uv)
        assert len(texels) > 0.1 * 37 * 19 and contested == 0
        assert np.array_equal(texels, want[1]) and np.array_equal(points.view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(owner[:, :, 1], want[2])
        assert np.array_equal(owner[:, :, 0], np.where(want[2] >= 0, 0, -1))


def test_bleed_layout_runs_over_the_unit_square(scene):
    bridge, _ = scene
    n = au.instance_count(bridge)
    insts = [e[0] for e in au.small_entries(n)]
    grid, bleed = au.merged_grid_uv(bridge, insts), au.merged_grid_uv(bridge, insts, bleed=True)
    placed = (grid != -1.0).any(axis=1)
    assert placed.any() and np.array_equal(placed, (bleed != -1.0).any(axis=1))
    assert grid[placed].min() >= 0 and grid[placed].max() <= 1
    assert bleed[placed].min() < 0 and bleed[placed].max() > 1
