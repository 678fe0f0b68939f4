"""The reference model of irradiance volumes (tests/model/volume_model.cpp) on the CPU: its sampler against a float64 numpy
restatement (the trilinear blend of sh9_basis evaluations); the known answers of the rule - grid nodes, constant volumes, clamps,
NaN positions, one-probe axes, invalid corners; its bake tied to the probe model: the grid probes are word for word what
make_probes gives, and probe_model_gather on them followed by the numpy finish is the model's volume.  No GPU needed."""
import numpy as np

import parity_util as pu
import probe_util as prb
import volume_util as vu

GRIDS = ((1, 1, 1), (2, 1, 3), (3, 4, 5), (5, 2, 2), (7, 6, 5))


def _desc(W, dims, **kw):
    from webgpu_raytracer_amd import renderer as R
    args = dict(origin=(-1.25, 0.5, 2.0), step=(0.75, 1.5, 0.3))
    args.update(kw)
    return R.volume_desc(dims=dims, **args)


def _valid_cases(W):
    """(desc, volume, points) of the float comparison: every grid, all probes valid, 4 096 random points in and around it"""
    for g, dims in enumerate(GRIDS):
        d = _desc(W, dims)
        v = vu.random_volume(d, 100 + g, invalid=False)
        rng = np.random.default_rng(200 + g)
        step = np.asarray(d["step"], np.float64)
        lo = np.asarray(d["origin"], np.float64) - step
        hi = np.asarray(d["origin"], np.float64) + np.array(dims) * step
        nrm = rng.normal(size=(4096, 3))
        yield d, v, vu.make_points(rng.uniform(lo, hi, (4096, 3)), nrm * rng.uniform(0.1, 10.0, (4096, 1)))


def test_sampler_against_float64(W):
    """Measured on the development host (g++ 11, glibc 2.35): the largest |f32 - f64| / max(1, |f64|) of the model over
    these inputs is 1.16e-6 (the grids 1x1x1 .. 7x6x5, 4 096 points each: 8 x 27 products of O(1) values summed in f32, a
    division and nine more products - a few dozen roundings of 6e-8).  The gate is four times that,
    volume_util.FLOAT_TOLERANCE; the margin is for other libm / compiler versions, not for the code under test."""
    worst = 0.0
    for d, v, pts in _valid_cases(W):
        got = vu.model_sample(d, v, pts)
        want = vu.sample_f64(d, v, pts)
        err = np.abs(got[:, :3].astype(np.float64) - want) / np.maximum(1.0, np.abs(want))
        worst = max(worst, float(err.max()))
        assert np.abs(got[:, 3].astype(np.float64) - 1.0).max() <= 5e-7      # W: eight products summed, all probes valid
        assert (want > 0).any(axis=1).mean() > 0.9                    # not a comparison of clamped zeros
    print("largest relative error of the model's sampler", worst)
    assert worst <= vu.FLOAT_TOLERANCE, worst
    assert worst > 0.0


def _eval_probe(W, rec, normal):
    """what the rule gives for a single probe with weight 1, in float32 by hand"""
    n = np.asarray(normal, np.float32)
    inv = np.float32(1.0) / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])     # rt_normalize: a * (1 / sqrt(dot))
    assert inv.dtype == np.float32
    Y = prb.sh9_basis_f32(n * inv)
    sh = rec[:27].reshape(9, 3)                                                    # coef = (0 + 1 * sh) / 1 = sh
    E = np.zeros(3, np.float32)
    for k in range(9):
        E = E + sh[k] * Y[k]
    return np.maximum(np.float32(0.0), E)


def test_a_point_on_a_probe_returns_that_probe(W):
    d = _desc(W, (3, 4, 5), origin=(-1.0, 0.5, 2.0), step=(0.5, 0.25, 2.0))     # nodes are exact in f32
    v = vu.random_volume(d, 7, invalid=False)
    nodes = vu.numpy_probes(d)[:, 0:3]
    rng = np.random.default_rng(8)
    nrm = rng.normal(size=(len(nodes), 3)).astype(np.float32)
    got = vu.model_sample(d, v, vu.make_points(nodes, nrm))
    assert np.array_equal(got[:, 3], np.ones(len(nodes), np.float32))
    for p in range(len(nodes)):
        assert np.array_equal(got[p, :3], _eval_probe(W, v[p], nrm[p])), p


def test_a_constant_volume_is_constant_everywhere(W):
    for dims in ((3, 4, 5), (1, 1, 1), (1, 3, 1), (2, 1, 1)):
        d = _desc(W, dims, origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0))
        rec = vu.random_volume(_desc(W, (1, 1, 1)), 3, invalid=False)[0]
        rec[:] = np.round(rec * 64) / 64                                        # a few mantissa bits: weights of 1/2^k blend exactly
        v = np.tile(rec, (vu.probe_count(d), 1))
        normal = np.array([0.0, 0.0, 2.0], np.float32)
        want = _eval_probe(W, rec, normal)
        pos = np.array([[0.5, 0.25, 0.75], [1.5, 2.5, 3.25], [-1e6, 0.5, 0.5], [1e30, 1e30, 1e30], [-np.inf, np.inf, 0.0],
                        [np.nan, np.nan, np.nan], [0.25, np.nan, 0.5], [2.0, 3.0, 4.0]], np.float32)
        got = vu.model_sample(d, v, vu.make_points(pos, np.tile(normal, (len(pos), 1))))
        assert np.array_equal(got[:, 3], np.ones(len(pos), np.float32)), dims
        for row in got:
            assert np.array_equal(row[:3], want), (dims, row, want)
    # a NaN position lands in cell 0: with distinct probes it is exactly probe (0, 0, 0)
    d = _desc(W, (3, 4, 5))
    v = vu.random_volume(d, 9, invalid=False)
    got = vu.model_sample(d, v, vu.make_points([[np.nan] * 3], [[0.0, 1.0, 0.0]]))
    assert np.array_equal(got[0, :3], _eval_probe(W, v[0], [0.0, 1.0, 0.0])) and got[0, 3] == 1.0
    # far outside on the high side: the last probe
    got = vu.model_sample(d, v, vu.make_points([[1e9, 1e9, np.inf]], [[0.0, 1.0, 0.0]]))
    assert np.array_equal(got[0, :3], _eval_probe(W, v[-1], [0.0, 1.0, 0.0])) and got[0, 3] == 1.0


def test_invalid_corners(W):
    d = _desc(W, (2, 2, 2), origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), max_hit_fraction=0.5)
    v = vu.random_volume(d, 11, invalid=False)
    pts = vu.make_points([[0.25, 0.5, 0.75]], [[1.0, 2.0, 3.0]])
    wx, wy, wz = (np.float32(0.75), np.float32(0.25)), (np.float32(0.5), np.float32(0.5)), (np.float32(0.25), np.float32(0.75))
    w = np.array([(wx[c & 1] * wy[(c >> 1) & 1]) * wz[c >> 2] for c in range(8)], np.float32)
    # all eight invalid: four +0
    bad = v.copy()
    bad[:, 27] = 0.75
    assert np.array_equal(vu.words(vu.model_sample(d, bad, pts)), np.zeros(4, np.uint32))
    bad[:, 27] = np.nan
    assert np.array_equal(vu.words(vu.model_sample(d, bad, pts)), np.zeros(4, np.uint32))
    # one invalid corner full of NaN: no NaN comes out, W is the sum of the other seven weights in corner order
    for c in range(8):
        one = v.copy()
        one[c, :27] = np.nan
        one[c, 27] = 0.5000001
        got = vu.model_sample(d, one, pts)[0]
        W_want = np.float32(0.0)
        for k in range(8):
            W_want = W_want + (w[k] if k != c else np.float32(0.0))
        assert not np.isnan(got).any() and got[3] == W_want and (got[:3] > 0).any(), (c, got)
        # ... and the blend is the renormalised one: the same as the valid seven weighted in float64
        keep = [k for k in range(8) if k != c]
        blend = (w[keep, None].astype(np.float64) * v[keep, :27]).sum(axis=0) / float(W_want)
        n = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
        from webgpu_raytracer_amd import renderer as R
        want = np.maximum(0.0, R.sh9_basis(n[None])[0] @ blend.reshape(9, 3))
        assert np.abs(got[:3] - want).max() <= vu.FLOAT_TOLERANCE * max(1.0, np.abs(want).max())
    # a zero-weight corner holding NaN in a VALID probe is skipped too: the point sits on probe 0
    one = v.copy()
    one[1:, :27] = np.nan
    got = vu.model_sample(d, one, vu.make_points([[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]]))[0]
    assert not np.isnan(got).any() and got[3] == 1.0
    # max_hit_fraction = 1 admits hit_fraction == 1; just below 1 does not
    full = v.copy()
    full[:, 27] = 1.0
    d1 = _desc(W, (2, 2, 2), origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), max_hit_fraction=1.0)
    assert vu.model_sample(d1, full, pts)[0, 3] == 1.0
    d099 = _desc(W, (2, 2, 2), origin=(0.0, 0.0, 0.0), step=(1.0, 1.0, 1.0), max_hit_fraction=np.float32(1.0) - np.float32(2.0 ** -24))
    assert np.array_equal(vu.words(vu.model_sample(d099, full, pts)), np.zeros(4, np.uint32))


def test_numpy_restatements_equal_the_model(W):
    for g, dims in enumerate(GRIDS):
        d = _desc(W, dims, window=(1.0, 0.5, 0.0) if g % 2 else tuple(_hanning(W, 3.0)), pad_first=1000 + g, t_max=12.5)
        assert np.array_equal(vu.words(vu.numpy_probes(d)), vu.words(vu.model_probes(d))), dims
        v = vu.random_volume(d, 40 + g)
        assert np.array_equal(vu.words(vu.numpy_finish(d, v)), vu.words(vu.model_finish(d, v))), dims
        assert np.array_equal(vu.words(vu.model_finish(d, v)[:, 27]), vu.words(v[:, 27]))     # hit_fraction keeps its bits
        f32, f16 = vu.model_layers(d, v, False), vu.model_layers(d, v, True)
        assert np.array_equal(vu.words(f32), vu.words(v.reshape(-1, 7, 4).transpose(1, 0, 2)))
        import encode_util as eu
        assert np.array_equal(f16.reshape(-1), eu.host_f16(f32))


def _hanning(W, width):
    from webgpu_raytracer_amd import renderer as R
    return R.sh_hanning_window(width)


def test_the_models_bake_is_the_probe_model_behind_grid_probes(W):
    """probe_model_gather on the model's own grid probes, followed by the numpy finish, equals the model's volume bit for bit;
    the grid probes are word for word what probe_util.make_probes gives for the same positions and pads."""
    b = pu.bridge_for(W, "cornell")
    m = prb.model_for(W, b)
    lo, hi = prb.scene_bounds(b)
    dims = (3, 2, 4)
    step = (hi - lo) / (np.array(dims) + 1.0)
    d = _desc(W, dims, origin=lo + step, step=step, window=(1.0, 0.5, 0.0), pad_first=77, t_max=1e30)
    probes = vu.model_probes(d)
    want = prb.make_probes(vu.numpy_probes(d)[:, 0:3], t_max=1e30, pad_step=1, pad_first=77)
    assert np.array_equal(vu.words(probes), vu.words(want))
    sh9, hits, _ = m.gatherProbes(probes, 4, 65, prb.SEED)
    volume = vu.model_finish(d, sh9)
    assert np.array_equal(vu.words(volume), vu.words(vu.numpy_finish(d, sh9)))
    lit = int((np.abs(sh9[:, :27]).max(axis=1) > 0).sum())
    assert 2 * lit >= len(probes), lit
    assert (volume[:, 12:27] == 0).all() and (volume[:, 0:3] > 0).any()           # band 2 is windowed away, band 0 is not
    assert np.array_equal(vu.words(volume[:, 27]), vu.words(sh9[:, 27]))
