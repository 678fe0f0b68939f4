"""The reference model of probe visibility maps (tests/model/volume_visibility_model.cpp, mi355rt.h "THE VISIBILITY RULE") on
known answers, without a GPU: (a) where every probe sees every point the visible sampler is the plain one word for word;
(b) behind a wall, zero-variance maps shut the lit probes out exactly; (c) the fetch is as good across the octahedral fold as
inside the map; (d) the f32 sampler against a float64 restatement; (e) every border texel of an exported tile is the wrapped
texel.  The figures of (c) and (d) are printed and recorded in tests/volume_visibility_util.py."""
import numpy as np
import pytest

import volume_util as vu
import volume_visibility_util as vv

GRIDS = ((1, 1, 1), (2, 1, 3), (3, 4, 5))


def _R():
    from webgpu_raytracer_amd import renderer
    return renderer


def _desc(dims):
    return _R().volume_desc((-1.25, 0.5, 2.0), (0.75, 1.5, 0.3), dims, max_hit_fraction=0.5)


@pytest.mark.parametrize("dims", GRIDS)
@pytest.mark.parametrize("min_visibility,crush", [(0.0, 0.0), (0.3, 0.7), (1.0, 1.0)])
def test_identity_where_every_probe_sees_every_point(W, dims, min_visibility, crush):
    """(a): flags = 0 and maps of {D, D * D} with D beyond every corner distance plus the bias: vis = 1 at every corner, and
    the visible sample is volume_model_sample word for word - invalid, NaN and infinite probes, points outside, NaN positions
    and zero normals included.  (An infinite position has no finite distance, so it is not among the points.)"""
    R = _R()
    d = _desc(dims)
    g = GRIDS.index(dims)
    vol = vu.random_volume(d, 500 + g)
    pts = vu.parity_points(d, 400, 600 + g)
    pts = pts[~np.isinf(pts[:, 0:3]).any(axis=1)]
    bias = 0.25
    nodes = vu.numpy_probes(d)[:, 0:3].astype(np.float64)
    finite = pts[np.isfinite(pts[:, 0:3]).all(axis=1), 0:3].astype(np.float64)
    far = np.sqrt(((finite[:, None, :] - nodes[None, :, :]) ** 2).sum(axis=2)).max() + bias
    D = 2.0 * far + 1.0
    v = R.volume_visibility_desc(8, 4.0 * D, normal_bias=bias, min_visibility=min_visibility, crush_threshold=crush)
    maps = vv.constant_maps(d, v, D)
    assert (vv.model_weights(d, v, maps, pts) == 1.0).all()
    got = vv.model_sample(d, v, vol, maps, pts)
    want = vu.model_sample(d, vol, pts)
    assert (want[:, 3] > 0).any() and np.isnan(pts[:, 0:3]).any()
    vu.check_samples(got, want, "identity %s" % (dims,))


X_WALL = 1.5


def _wall_case(size, max_distance, pos):
    """a 4 x 2 x 2 grid of unit cells cut by the plane x = 1.5: probes x <= 1 are lit (band-0 irradiance 1), probes x >= 2 dark"""
    R = _R()
    d = R.volume_desc((0, 0, 0), (1, 1, 1), (4, 2, 2), max_hit_fraction=0.5)
    v = R.volume_visibility_desc(size, max_distance)
    probes = vu.numpy_probes(d)
    vol = np.zeros((16, 28), np.float32)
    vol[probes[:, 0] < X_WALL, 0:3] = 1.0
    maps = vv.plane_maps(d, v, X_WALL)
    assert np.array_equal(maps[..., 1], maps[..., 0] * maps[..., 0])                       # zero variance, texel by texel
    pts = vu.make_points(pos, np.random.default_rng(12).normal(size=(len(pos), 3)))
    return d, v, probes, vol, maps, pts


def _lit_corner_taps(v, probes, maps, pts):
    """per lit corner c (dx = 0) of the cell x in [1, 2]: (c, len (m,), the four taps' mean distances (m, 4)), by the float64
    restatement of the fetch's indices"""
    size = int(v["size"])
    pos = pts[:, 0:3].astype(np.float64)
    for c in (0, 2, 4, 6):
        corner = np.array([1, (c >> 1) & 1, c >> 2])
        p = (corner[2] * 2 + corner[1]) * 4 + corner[0]
        e = pos - probes[p, 0:3].astype(np.float64)
        length = np.linalg.norm(e, axis=1)
        u = (vv.pack_f64(e / length[:, None]) * 0.5 + 0.5) * size - 0.5
        i0 = np.clip(np.floor(u), -1, size - 1).astype(np.int64)
        taps = []
        for di in (0, 1):
            for dj in (0, 1):
                i, j, _ = vv.wrap_f64(i0[:, 0] + di, i0[:, 1] + dj, size)
                taps.append(maps[p, j, i, 0].astype(np.float64))
        yield c, length, np.stack(taps, axis=1)


def test_a_wall_shuts_the_lit_probes_out(W):
    """(b): zero-variance maps of the plane alone, min_visibility = crush_threshold = flags = 0, points on the dark side: every
    lit corner has len > m1 at all four of its taps (asserted here, on the inputs), so its Chebyshev weight is exactly 0 and
    the rgb is exactly +0, where the plain sampler leaks.

    The rule interpolates the two moments separately, so between taps that hold DIFFERENT distances the fetched variance is
    positive (Jensen) and the weight a tiny positive number, not 0 - the next test bounds it.  Exactly 0 needs the four taps
    to agree.  Here they do: max_distance = 0.51 clamps every texel of a lit probe further than 11.4 degrees from the +x axis
    (the plane is 0.5 away), and the points see the lit probe (1, 0, 0) 22 .. 27 degrees off that axis - four texels of the 32
    x 32 map, 5.6 degrees each, off the unclamped cone - from beside the grid (y, z <= 0, where the trilinear weight of the
    other six corners is exactly 0) and within 0.5 of the dark probe (2, 0, 0), which therefore sees them."""
    rng = np.random.default_rng(11)
    n = 200
    x = rng.uniform(1.96, 1.98, n)
    theta, phi = np.radians(rng.uniform(22.0, 27.0, n)), rng.uniform(0.0, 0.5 * np.pi, n)
    r = np.tan(theta) * (x - 1.0)
    pos = np.stack([x, -r * np.cos(phi), -r * np.sin(phi)], axis=1)
    d, v, probes, vol, maps, pts = _wall_case(32, 0.51, pos)
    assert (maps[probes[:, 0] < X_WALL][..., 0] < 0.51).any(), "the lit probes' maps hold the wall"
    for c, length, taps in _lit_corner_taps(v, probes, maps, pts):
        assert (length[:, None] > taps * (1.0 + 1e-5)).all(), c
    weights = vv.model_weights(d, v, maps, pts)
    assert (weights[:, 0] == 0.0).all() and (weights[:, 1] == 1.0).all(), (weights[:, 0].max(), weights[:, 1].min())
    got = vv.model_sample(d, v, vol, maps, pts)
    assert (vu.words(got[:, 0:3]) == 0).all()                                             # exactly +0
    assert (got[:, 3] > 0).all()
    plain = vu.model_sample(d, vol, pts)
    assert (plain[:, 0:3] > 0).all(), "the plain sampler leaks on these points"
    print("leak of the plain sampler: rgb", float(plain[:, 0].min()), "..", float(plain[:, 0].max()))


def test_a_wall_between_unequal_taps_leaks_no_more_than_their_spread_allows(W):
    """(b) on points inside the cells, max_distance 4, where the four taps of a lit corner hold different distances to the
    plane: the fetched variance is at most (spread / 2)^2 (Popoviciu), the gap at least len - the largest tap, so vis <=
    (V / (V + g^2))^3 with those two - a bound from the inputs alone.  The dark corners see the points: vis = 1."""
    rng = np.random.default_rng(13)
    pos = np.stack([rng.uniform(1.85, 1.97, 200), rng.uniform(0.3, 0.7, 200), rng.uniform(0.3, 0.7, 200)], axis=1)
    d, v, probes, vol, maps, pts = _wall_case(16, 4.0, pos)
    weights = vv.model_weights(d, v, maps, pts)
    worst = 0.0
    for c, length, taps in _lit_corner_taps(v, probes, maps, pts):
        assert (length[:, None] > taps * (1.0 + 1e-5)).all(), c
        V = ((taps.max(axis=1) - taps.min(axis=1)) / 2.0) ** 2
        g = length - taps.max(axis=1)
        bound = (V / (V + g * g)) ** 3
        assert (weights[:, c] <= bound * (1.0 + 1e-3) + 1e-30).all(), (c, float((weights[:, c] / bound).max()))
        worst = max(worst, float(weights[:, c].max()))
    assert (weights[:, 1::2] == 1.0).all()
    got = vv.model_sample(d, v, vol, maps, pts)
    plain = vu.model_sample(d, vol, pts)
    print("largest lit-corner weight", worst, "largest rgb", float(got[:, 0].max()), "the plain sampler's smallest",
          float(plain[:, 0].min()))
    assert worst < 1e-3 and (got[:, 0:3] <= 1e-3 * plain[:, 0:3]).all()


def _smooth(dirs):
    return 1.0 + 0.5 * dirs[..., 0] + 0.3 * dirs[..., 1] - 0.2 * dirs[..., 2]


def test_the_fetch_is_continuous_across_the_seam(W):
    """(c): a smooth function of direction stored at texel centres, fetched at 20000 random directions in float64 and by the
    model, against the function itself.  The worst error over directions whose four taps needed a wrap is at most twice the
    worst over directions that needed none (the factor is for the stronger curvature of the mapping at the fold); a wrong fold
    reads a texel from the other side of the sphere and fails this by orders of magnitude."""
    size = 16
    centres = vv.texel_directions(size)
    map64 = np.stack([_smooth(centres), _smooth(centres) ** 2], axis=-1)
    map32 = map64.astype(np.float32)
    rng = np.random.default_rng(3)
    dirs = rng.normal(size=(20000, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    dirs32 = dirs.astype(np.float32)
    truth = _smooth(dirs32.astype(np.float64))
    got64, wrapped64 = vv.fetch_f64(map64, dirs32.astype(np.float64))
    got32, wrapped32 = vv.model_fetch(map32, dirs32)
    assert wrapped64.sum() > 500 and (~wrapped64).sum() > 500
    assert (wrapped64 != wrapped32).sum() <= 2                           # a tap index may differ where u is an integer
    for name, got, wrapped in (("float64 fetch", got64, wrapped64), ("model", got32.astype(np.float64), wrapped32)):
        err = np.abs(got[:, 0] - truth)
        seam, inside = err[wrapped].max(), err[~wrapped].max()
        print("%s: worst error with a wrapped tap %.3g, without %.3g" % (name, seam, inside))
        assert seam <= 2.0 * inside, (name, seam, inside)


def _f64_cases():
    R = _R()
    out = []
    for g, dims in enumerate(GRIDS):
        d = _R().volume_desc((-1.25, 0.5, 2.0), (0.75, 1.5, 0.3), dims, max_hit_fraction=2.0)
        vol = vu.random_volume(d, 700 + g, invalid=False)
        rng = np.random.default_rng(800 + g)
        origin, step = np.asarray(d["origin"], np.float64), np.asarray(d["step"], np.float64)
        hi = origin + (np.array(dims) - 1) * step
        pos = rng.uniform(origin - 0.5 * step, hi + 0.5 * step, (1500, 3))
        pts = vu.make_points(pos, rng.normal(size=(1500, 3)))
        for size, backface, crush, min_vis, bias in ((4, False, 0.0, 0.0, 0.0), (8, True, 0.4, 0.05, 0.1), (16, False, 0.6, 0.0, 0.05),
                                                     (8, True, 0.0, 0.2, 0.0)):
            v = R.volume_visibility_desc(size, 10.0, normal_bias=bias, min_visibility=min_vis, crush_threshold=crush,
                                         backface=backface)
            out.append((d, v, vol, vv.random_maps(d, v, 900 + g + size, hostile=False), pts))
    return out


def test_the_model_against_float64(W):
    """(d): the model's visible sampler against the float64 restatement on valid volumes, maps of positive variance, every
    option of the descriptor.  The gate is four times the largest error measured on the development host."""
    worst = 0.0
    for d, v, vol, maps, pts in _f64_cases():
        got = vv.model_sample(d, v, vol, maps, pts).astype(np.float64)
        want, W64 = vv.sample_f64(d, v, vol, maps, pts)
        assert (W64 > 0).all()
        err = np.abs(got[:, 0:3] - want) / np.maximum(1.0, np.abs(want))
        errW = np.abs(got[:, 3] - W64) / np.maximum(1.0, W64)
        worst = max(worst, float(err.max()), float(errW.max()))
    print("largest |model - f64| / max(1, |f64|): %.3g" % worst)
    assert worst <= vv.FLOAT_TOLERANCE, worst


@pytest.mark.parametrize("size", (4, 8, 32))
def test_every_border_texel_of_a_tile_is_the_wrapped_texel(W, size):
    """(e): the tiles of a (3, 2, 2) grid, f32 and f16: the interior of tile p is map p, and border texel (a, b) holds texel
    wrap(a - 1, b - 1) of the same map - an edge's mirror image, a corner's diagonal opposite."""
    R = _R()
    d = R.volume_desc((0, 0, 0), (1, 1, 1), (3, 2, 2))
    v = R.volume_visibility_desc(size, 1.0)
    maps = np.arange(12 * size * size * 2, dtype=np.float32).reshape(12, size, size, 2) * np.float32(0.25)
    tiles = vv.model_tiles(d, v, maps, False)
    tile = size + 2
    assert tiles.shape == (4 * tile, 3 * tile, 2)
    for p in range(12):
        t = tiles[(p // 3) * tile:(p // 3 + 1) * tile, (p % 3) * tile:(p % 3 + 1) * tile]
        assert np.array_equal(t[1:-1, 1:-1], maps[p])
        for b in range(tile):
            for a in range(tile):
                if 0 < a < tile - 1 and 0 < b < tile - 1:
                    continue
                at = vv.model_wrap(size, a - 1, b - 1)
                i, j, _ = vv.wrap_f64(a - 1, b - 1, size)
                assert at == int(j) * size + int(i)
                assert np.array_equal(t[b, a], maps[p].reshape(-1, 2)[at]), (p, a, b)
        # the rule's folds in words: the left border is the first column upside down, the top border the first row reversed
        assert np.array_equal(t[1:-1, 0], maps[p][::-1, 0]) and np.array_equal(t[0, 1:-1], maps[p][0, ::-1])
        assert np.array_equal(t[0, 0], maps[p][size - 1, size - 1])
    half = vv.model_tiles(d, v, maps, True)
    assert np.array_equal(half.view(np.float16).astype(np.float32), tiles.astype(np.float16).astype(np.float32))
