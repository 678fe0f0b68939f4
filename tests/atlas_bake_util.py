"""Shared pieces of the atlas-bake tests (rt_bake_atlas_points / rt_bake_atlas_irradiance).  The yardstick is identity (B) of
include/mi355rt.h, built from what is already trusted: an atlas bake is the composition of its entries' single-instance
bakes - bake_util.BakeModel.bakePoints per entry, placed at the rectangle, the lowest entry winning, the pads re-based.
Also the override layouts of the tests: grid_uv of one instance per distinct geometry, merged, and its "bleed" variant
whose charts run outside [0, 1]."""
import numpy as np

import bake_util as bu


def compose(model, entries, width, height, t_max=1e30, pad_base=0, atlas_uv=None):
    """-> (points (n, 8) f32, texels (n,) u32 ascending, owner (height, width, 2) i32 {entry, triangle} with {-1, -1} for
    none, contested: the number of atlas texels more than one entry covers).  model: anything with BakeModel's bakePoints."""
    owner = np.full((height * width, 2), -1, np.int32)
    points = np.zeros((height * width, 8), np.float32)
    times = np.zeros(height * width, np.int64)
    for e, (inst, x, y, w, h) in enumerate(entries):
        p, t, o = model.bakePoints(inst, w, h, t_max=t_max, pad_base=0, atlas_uv=atlas_uv)
        t = t.astype(np.int64)
        at = (y + t // w) * width + (x + t % w)          # the atlas texel of every local texel
        times[at] += 1
        free = owner[at, 0] < 0                          # entries come in ascending order: the first to cover a texel owns it
        at, t, p = at[free], t[free], p[free].copy()
        p.view(np.uint32)[:, 7] = (pad_base + at).astype(np.uint32)
        points[at] = p
        owner[at, 0] = e
        owner[at, 1] = o.ravel()[t]
    texels = np.flatnonzero(owner[:, 0] >= 0)
    return points[texels], texels.astype(np.uint32), owner.reshape(height, width, 2), int((times > 1).sum())


def merged_grid_uv(bridge, insts, bleed=False):
    """grid_uv of one instance per distinct geometry among insts, merged: every vertex a grid placed keeps its place, all
    others lie at (-1, -1).  bleed: uv * 1.3 - 0.15 on the placed vertices - every chart grid runs 15 % of the atlas over
    each edge of [0, 1], so a local bake that were not clipped to its rectangle would reach its neighbours."""
    uv = None
    seen = set()
    for inst in insts:
        tris = bu.instance_triangles(bridge, inst)
        if tris in seen:
            continue
        seen.add(tris)
        g = bu.grid_uv(bridge, inst)
        uv = g if uv is None else np.where((g != -1.0).any(axis=1)[:, None], g, uv)
    placed = (uv != -1.0).any(axis=1)
    if bleed:
        uv = np.where(placed[:, None], uv * np.float32(1.3) - np.float32(0.15), np.float32(-1.0)).astype(np.float32)
    return uv


def small_entries(n_inst):
    """the five entries of the small composition case in a 45 x 37 atlas: rectangles off the 8-texel grid, two instances of
    one geometry (instanced1000: 1 and 3), an overlap (entries 2 and 3), a repeated instance (entries 0 and 4) and a 1 x 1"""
    n = n_inst
    return [(1 % n, 0, 0, 19, 17), (3 % n, 19, 0, 26, 17), (0, 3, 17, 33, 20), (2 % n, 20, 25, 25, 12), (1 % n, 0, 36, 1, 1)]


SMALL_W, SMALL_H = 45, 37


def instance_count(bridge):
    return np.asarray(bridge.draw_commands).size // 4


def check_atlas_points(got, want, tag):
    """(points, texels, owner) word for word; in rows where the MODEL has a NaN, NaNs compare as a class (check_points' rule)"""
    gp, gt, go = got
    wp, wt, wo = want[:3]
    assert go.shape == wo.shape and np.array_equal(go, wo), (tag, "owner maps differ at", np.argwhere(go != wo)[:8].tolist())
    assert len(gt) == len(wt) and np.array_equal(gt, wt), (tag, "texel indices", len(gt), len(wt))
    g, w = gp.view(np.uint32), wp.view(np.uint32)
    bad = g != w
    model_nan_row = np.isnan(wp).any(axis=1)
    bad &= ~(np.isnan(gp) & np.isnan(wp) & model_nan_row[:, None])
    rows = np.nonzero(bad.any(axis=1))[0]
    assert rows.size == 0, (tag, "points that differ", int(rows.size), rows[:8].tolist(), gp[rows[:4]].tolist(), wp[rows[:4]].tolist())
