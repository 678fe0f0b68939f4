"""Shared pieces of the atlas-denoise tests (rt_denoise_atlas): the reference model (tests/model/denoise_model.cpp, one pass in
plain loops with the six tap counts), built with the flags of oracle/Makefile as dilate_util builds its model, and its
composition into a call; the synthetic guide generator "two walls"; the named patterns with their written-out counts; and the
hand-worked cases with written-out answers."""
import ctypes
import functools
import os

import numpy as np

import dilate_util
import model_build
import radiance_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "model", "denoise_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libdenoise_model.so")
NAN, INF = float("nan"), float("inf")
COUNTS = ("accepted", "outside", "unguided", "normal", "plane", "distance")
# the parameters of the synthetic patterns: world units of two_walls()
CELL = 0.1
PARAMS = dict(normal_cos=0.9, plane_eps=0.02, max_dist=0.5)


@functools.lru_cache(maxsize=None)
def model_lib():
    L = ctypes.CDLL(model_build.build(SRC, LIB, ru.FLAGS + ["-I", os.path.join(REPO, "include"), "-shared"]))
    vp, u32, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
    L.denoise_model_pass.argtypes = [vp, u32, u32, u32, f32, f32, f32, vp, vp, u32, vp, vp]
    L.denoise_model_pass.restype = None
    return L


def as_f32(atlas):
    """an (H, W, 4) f32 array or an (H, W) array of 16-byte records -> (H, W, 4) f32, the same bytes"""
    a = np.ascontiguousarray(atlas)
    if a.dtype != np.float32:
        a = a.view(np.float32).reshape(a.shape[0], a.shape[1], 4)
    assert a.ndim == 3 and a.shape[2] == 4
    return a


words = dilate_util.words   # any 16-byte-texel atlas -> (H, W, 4) u32


def model_pass(atlas, points, texels, step, *, plane_eps, max_dist, normal_cos=0.9):
    """one pass at `step` -> (out (H, W, 4) f32, the six counts as a tuple in the order of COUNTS)"""
    a = as_f32(atlas)
    H, W = a.shape[:2]
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 8)
    tex = np.ascontiguousarray(texels, np.uint32).reshape(-1)
    assert len(pts) == len(tex)
    out = np.empty_like(a)
    counts = np.zeros(6, np.uint64)
    model_lib().denoise_model_pass(a.ctypes.data, W, H, int(step), float(normal_cos), float(plane_eps), float(max_dist),
                                   pts.ctypes.data if len(pts) else None, tex.ctypes.data if len(tex) else None, len(tex),
                                   out.ctypes.data, counts.ctypes.data)
    return out, tuple(int(c) for c in counts)


def denoise_model(atlas, points, texels, *, plane_eps, max_dist, normal_cos=0.9, passes=3, step=1):
    """a call: pass p at step << p, each on the result of the one before -> (out (H, W, 4) f32, [counts of every pass])"""
    a, counts = as_f32(atlas), []
    for p in range(passes):
        a, c = model_pass(a, points, texels, step << p, plane_eps=plane_eps, max_dist=max_dist, normal_cos=normal_cos)
        counts.append(c)
    return a, counts


def make_points(positions, normals, texels):
    """(n, 3), (n, 3), (n,) -> (n, 8) f32 in the rt_gather_point layout: t_max 1e30, pad = the texel index"""
    texels = np.asarray(texels, np.uint32)
    pts = np.zeros((len(texels), 8), np.float32)
    pts[:, 0:3] = positions
    pts[:, 3] = 1e30
    pts[:, 4:7] = normals
    pts[:, 7] = texels.view(np.float32)
    return pts


def two_walls(width, height, p, seed):
    """The synthetic guides: the left half of the atlas (x < width // 2) is a floor, z = 0 with normal +z, the right half a wall
    with normal +x that stands on the floor's right edge; texel (x, y) lies at its place on a regular world grid of CELL units
    plus a seeded jitter - +-0.03 out of its plane, so that with plane_eps 0.02 the plane stop accepts and rejects, and
    in its plane +-0.03, with every tenth point thrown up to 0.6 further, so that with max_dist 0.5 the distance stop does both
    at step 1 as at step 4.  A texel is covered with probability p.  Colours are ordinary finite values: rgb in [0, 4), the
    fourth in [0, 1].  -> (atlas (H, W, 4) f32, points (n, 8) f32, texels (n,) u32 ascending)"""
    rng = np.random.default_rng(seed)
    cover = rng.random((height, width)) < p
    ys, xs = np.mgrid[0:height, 0:width]
    half = width // 2
    out_of_plane = rng.uniform(-0.03, 0.03, (height, width))
    in_plane = rng.uniform(-0.03, 0.03, (height, width, 2))
    thrown = rng.random((height, width)) < 0.1
    in_plane[thrown] += rng.uniform(-0.6, 0.6, (int(thrown.sum()), 2))
    floor = xs < half
    pos = np.empty((height, width, 3))
    pos[..., 0] = np.where(floor, xs * CELL + in_plane[..., 0], half * CELL + out_of_plane)
    pos[..., 1] = ys * CELL + in_plane[..., 1]
    pos[..., 2] = np.where(floor, out_of_plane, (xs - half) * CELL + in_plane[..., 0])
    nrm = np.where(floor[..., None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    atlas = np.empty((height, width, 4), np.float32)
    atlas[..., 0:3] = rng.uniform(0.0, 4.0, (height, width, 3))
    atlas[..., 3] = rng.uniform(0.0, 1.0, (height, width))
    texels = np.flatnonzero(cover.reshape(-1)).astype(np.uint32)
    points = make_points(pos.reshape(-1, 3)[texels], nrm.reshape(-1, 3)[texels], texels)
    return atlas, points, texels


def special_values(atlas, seed):
    """a copy of the atlas with a fifth of its words replaced by infinities, NaNs (quiet and signalling, both signs), denormals
    and both zeros"""
    rng = np.random.default_rng(seed)
    w = words(np.array(atlas, np.float32)).copy()
    special = np.array([0x7fc00000, 0x7f800001, 0xffc12345, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x00400000, 0x0,
                        0x80000000], np.uint32)
    pick = rng.random(w.shape) < 0.2
    w[pick] = special[rng.integers(0, len(special), size=int(pick.sum()))]
    return w.view(np.float32)


def same_words(got, want):
    """(H, W) bool: the texels in which some word differs - where the model's word is a NaN the other's need only be a NaN"""
    g, w = words(got), words(want)
    with np.errstate(invalid="ignore"):
        both_nan = np.isnan(as_f32(got)) & np.isnan(as_f32(want))
    return ((g != w) & ~both_nan).any(axis=2)


# (width, height, p, seed, step) of two_walls under PARAMS -> (accepted, outside, unguided, normal, plane, distance) of ONE
# pass, from the numpy restatement below (numpy_counts)
PATTERNS = {
    (37, 21, 0.6, 3, 1): (2818, 955, 4047, 196, 2910, 354),
    (37, 21, 0.6, 3, 4): (476, 3875, 2935, 676, 1690, 1628),
    (17, 33, 0.6, 4, 1): (1810, 783, 2957, 286, 1506, 170),
    (17, 33, 0.6, 4, 4): (268, 3046, 1994, 1054, 624, 526),
}


def numpy_counts(atlas, points, texels, step, *, plane_eps, max_dist, normal_cos=0.9):
    """the six counts of one pass by array arithmetic in f32: one shifted comparison per tap, no loop over texels"""
    H, W = atlas.shape[:2]
    guide = np.full(H * W, -1, np.int64)
    tex = np.asarray(texels, np.int64)
    j = np.flatnonzero(tex < H * W)[::-1]
    guide[tex[j]] = j                      # descending j: the lowest is assigned last and stays
    guide = guide.reshape(H, W)
    guided = guide >= 0
    P = np.zeros((H, W, 3), np.float32)
    N = np.zeros((H, W, 3), np.float32)
    P[guided] = points[guide[guided], 0:3]
    N[guided] = points[guide[guided], 4:7]
    f = np.float32
    md2 = f(max_dist) * f(max_dist)
    counts = [0] * 6
    ys, xs = np.nonzero(guided)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dx == 0 and dy == 0:
                continue
            qx, qy = xs + dx * step, ys + dy * step
            inside = (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
            counts[1] += int((~inside).sum())
            x, y, qx, qy = xs[inside], ys[inside], qx[inside], qy[inside]
            g = guided[qy, qx]
            counts[2] += int((~g).sum())
            x, y, qx, qy = x[g], y[g], qx[g], qy[g]
            n, nq, d = N[y, x], N[qy, qx], P[qy, qx] - P[y, x]
            with np.errstate(invalid="ignore"):
                a = (n[:, 0] * nq[:, 0] + n[:, 1] * nq[:, 1]) + n[:, 2] * nq[:, 2] >= f(normal_cos)
                b = np.abs((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]) <= f(plane_eps)
                c = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= md2
            counts[3] += int((~a).sum())
            counts[4] += int((a & ~b).sum())
            counts[5] += int((a & b & ~c).sum())
            counts[0] += int((a & b & c).sum())
    return tuple(counts)


def coplanar(width, height, colour=1.0, z=0.0):
    """a fully guided floor: texel (x, y) at (x * CELL, y * CELL, z), normal +z, every colour word `colour`"""
    ys, xs = np.mgrid[0:height, 0:width]
    pos = np.stack([xs * CELL, ys * CELL, np.full_like(xs, z, dtype=np.float64)], axis=-1).reshape(-1, 3)
    texels = np.arange(width * height, dtype=np.uint32)
    atlas = np.full((height, width, 4), colour, np.float32)
    return atlas, make_points(pos, np.tile([0.0, 0.0, 1.0], (len(texels), 1)), texels), texels


def _row(positions, normals=None):
    """a fully guided 1-row atlas' guides: texel x at positions[x] with normals[x] (default +z)"""
    n = len(positions)
    normals = np.tile([0.0, 0.0, 1.0], (n, 1)) if normals is None else normals
    texels = np.arange(n, dtype=np.uint32)
    return make_points(np.asarray(positions, np.float64), normals, texels), texels


def hand_cases():
    """name -> (atlas (H, W, 4) f32, points, texels, keyword arguments of one call, expected (H, W, 4) f32 written out by hand).
    Every expected word is exact: the weights are dyadic, so the sums of the chosen colours are exact in f32 and the one
    division is a correctly rounded ratio of two small integers."""
    f = np.float32
    wide = dict(plane_eps=1.0, max_dist=100.0, normal_cos=0.9, passes=1, step=1)
    cases = {}
    # a fully guided coplanar 5 x 5 of colour 1.0: acc == wsum in every texel, whichever taps fall outside
    a, pts, tex = coplanar(5, 5, 1.0)
    cases["coplanar_5x5"] = (a, pts, tex, wide, np.full((5, 5, 4), 1.0, f))
    cases["coplanar_5x5_three_passes"] = (a, pts, tex, dict(wide, passes=3), np.full((5, 5, 4), 1.0, f))
    # a single guided texel: only the centre tap, h = 0.375 * 0.375 = 0.140625
    a = np.zeros((5, 5, 4), f)
    a[..., 3] = -1.0
    a[2, 3] = (0.3, 1.7, 2.9, 0.5)
    want = a.copy()
    want[2, 3] = (f(0.140625) * a[2, 3]) / f(0.140625)
    cases["single_texel"] = (a, make_points([[0.3, 0.2, 0.0]], [[0.0, 0.0, 1.0]], [13]), np.array([13], np.uint32), wide, want)
    # a column and a row of 9 whose colour is the texel's number: inside, the symmetric kernel returns the number; at the ends
    # 0: (0.25 * 1 + 0.0625 * 2) / 0.6875 = 6 / 11, 1: (0.375 + 0.25 * 2 + 0.0625 * 3) / 0.9375 = 17 / 15, and 8 minus those
    ramp = np.array([6 / 11, 17 / 15, 2, 3, 4, 5, 6, 103 / 15, 82 / 11], f)
    v = np.arange(9, dtype=f)
    pts, tex = _row([[0.0, y * CELL, 0.0] for y in range(9)])
    cases["1x9"] = (np.repeat(v, 4).reshape(9, 1, 4), pts, tex, wide, np.repeat(ramp, 4).reshape(9, 1, 4))
    pts, tex = _row([[x * CELL, 0.0, 0.0] for x in range(9)])
    cases["9x1"] = (np.repeat(v, 4).reshape(1, 9, 4), pts, tex, wide, np.repeat(ramp, 4).reshape(1, 9, 4))
    # the row again at step 4: the taps are the texels x - 8, x - 4, x, x + 4, x + 8 that exist.  0: (0.25 * 4 + 0.0625 * 8) /
    # 0.6875 = 24 / 11, 1: (0.375 * 1 + 0.25 * 5) / 0.625 = 2.6, 4: (0.25 * 0 + 0.375 * 4 + 0.25 * 8) / 0.875 = 4
    far = np.array([24 / 11, 5 * 0.25 / 0.625 + 1 * 0.375 / 0.625, 2 * 0.6 + 6 * 0.4, 3 * 0.6 + 7 * 0.4, 4.0, 5 * 0.6 + 1 * 0.4,
                    6 * 0.6 + 2 * 0.4, 7 * 0.6 + 3 * 0.4, 64 / 11], np.float64)
    cases["9x1_step_4"] = (np.repeat(v, 4).reshape(1, 9, 4), pts, tex, dict(wide, step=4), np.repeat(far.astype(f), 4).reshape(1, 9, 4))
    # a floor of colour 1 beside a wall of colour 3, every position within reach: only the normals tell them apart
    a = np.empty((5, 8, 4), f)
    a[:, :4], a[:, 4:] = 1.0, 3.0
    ys, xs = np.mgrid[0:5, 0:8]
    pos = np.stack([np.minimum(xs, 4) * CELL, ys * CELL, np.maximum(xs - 4, 0) * CELL], axis=-1).reshape(-1, 3)
    nrm = np.where((xs < 4).reshape(-1, 1), [0.0, 0.0, 1.0], [1.0, 0.0, 0.0])
    tex = np.arange(40, dtype=np.uint32)
    cases["floor_and_wall"] = (a, make_points(pos, nrm, tex), tex, dict(wide, passes=3), a.copy())
    # two coplanar charts 10 units apart with max_dist 0.5, an unguided texel between them
    a = np.empty((1, 9, 4), f)
    a[0, :4], a[0, 4], a[0, 5:] = 1.0, (7.0, -7.0, 0.5, -1.0), 5.0
    tex = np.array([0, 1, 2, 3, 5, 6, 7, 8], np.uint32)
    pos = [[(x + (100 if x > 4 else 0)) * CELL, 0.0, 0.0] for x in tex]
    cases["two_charts"] = (a, make_points(pos, np.tile([0.0, 0.0, 1.0], (8, 1)), tex), tex,
                           dict(wide, max_dist=0.5, passes=2), a.copy())
    # texel 2 is named twice: the first entry lies in the row, the second 100 units above it.  Guided by the first it takes
    # 0.0625 + 0.25 + 0.375 * 9 + 0.25 + 0.0625 = 4 (over 1); its neighbours take it in: 0: (0.375 + 0.25 + 0.0625 * 9) /
    # 0.6875 = 19 / 11, 1: (0.25 + 0.375 + 0.25 * 9 + 0.0625) / 0.9375 = 47 / 15.  A second row without guides keeps the
    # number of entries within the number of texels, and is copied.
    a = np.ones((2, 5, 4), f)
    a[0, 2] = 9.0
    a[1] = 7.0
    tex = np.array([0, 1, 2, 2, 3, 4], np.uint32)
    pos = [[0, 0, 0], [CELL, 0, 0], [2 * CELL, 0, 0], [2 * CELL, 0, 100.0], [3 * CELL, 0, 0], [4 * CELL, 0, 0]]
    want = a.copy()
    want[0] = np.repeat(np.array([19 / 11, 47 / 15, 4.0, 47 / 15, 19 / 11], f), 4).reshape(5, 4)
    tight = dict(wide, plane_eps=0.01)
    cases["duplicate_texel"] = (a, make_points(pos, np.tile([0.0, 0.0, 1.0], (6, 1)), tex), tex, tight, want)
    # ... and entries past the atlas (10, 0xffffffff) are ignored, wherever they stand in the list
    tex2 = np.array([10, 0, 1, 2, 0xffffffff, 2, 3, 4], np.uint32)
    pos2 = [[0, 0, 0]] + pos[0:3] + [[CELL, 0, 0]] + pos[3:]
    cases["out_of_range_texel"] = (a, make_points(pos2, np.tile([0.0, 0.0, 1.0], (8, 1)), tex2), tex2, tight, want)
    # unguided texels keep their bits whatever they hold: -1, -2, NaNs with payloads, an infinity
    a = np.ones((1, 5, 4), f)
    w = a.view(np.uint32)
    w[0, 1] = (0x7fc00123, 0xff800001, 0x7f800000, 0xbf800000)
    w[0, 3] = (0x00000001, 0x80000000, 0xffc00000, 0xc0000000)
    tex = np.array([0, 2, 4], np.uint32)
    cases["unguided_bits"] = (a, make_points([[x * CELL, 0, 0] for x in tex], np.tile([0.0, 0.0, 1.0], (3, 1)), tex), tex, wide,
                              a.copy())
    # a NaN normal in texel 2 of the ramp 0 .. 4: it accepts only its centre, and no neighbour accepts it.  0: (0.25 * 1) /
    # 0.625 = 0.4, 1: (0.25 * 0 + 0.375 * 1 + 0.0625 * 3) / 0.6875 = 9 / 11, 3 and 4 by symmetry: 4 - 9 / 11, 4 - 0.4
    v = np.arange(5, dtype=f)
    nrm = np.tile([0.0, 0.0, 1.0], (5, 1))
    nrm[2] = (NAN, 0.0, 1.0)
    pts, tex = _row([[x * CELL, 0.0, 0.0] for x in range(5)], nrm)
    want = np.repeat(np.array([0.4, 9 / 11, 2.0, 35 / 11, 3.6], f), 4).reshape(1, 5, 4)
    cases["nan_normal"] = (np.repeat(v, 4).reshape(1, 5, 4), pts, tex, wide, want)
    return cases
