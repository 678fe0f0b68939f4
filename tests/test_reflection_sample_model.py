"""The reference model of the reflection sampler (tests/model/reflection_sample_model.cpp) on the CPU: against an independent
float64 restatement of the rule, on constant maps, across the seams of the octahedral map - where a clamp-to-edge fetch is
shown to fail - against a numpy fold, on the known answers of the parallax correction, and on the identities the rule
promises word for word.  No GPU needed."""
import numpy as np
import pytest

import reflection_sample_util as rs
import reflection_util as rf

CASES = [(8, 2), (16, 3)]   # (size, levels)


def _random_chains(rng, size, levels, n_probes):
    maps = rng.uniform(0.0, 4.0, size=(n_probes, size, size, 4)).astype(np.float32)
    return rf.model_filter(rf.desc(size, levels, 1, 64), maps)


def test_the_model_against_float64(W):
    """The yardstick is the float64 restatement (reflection_sample_util.sample_f64); the figure is the largest |model - f64| /
    max(1, |f64|) over 4000 random queries of each of six cases: (size, levels) = (8, 2), (16, 2) and (16, 3) - 8 >> 2 is below
    the smallest level the library takes - with parallax on and off, three probes of random maps in [0, 4] inside their boxes, directions of lengths 0.25 .. 4, positions inside and a
    little outside the boxes, roughness over a little more than [0, 1].  Measured on the development host: 2.95e-06.  The gate
    is four times that, for other compilers and libms: 1.18e-05."""
    from webgpu_raytracer_amd import renderer as R
    MEASURED = 2.95e-6
    worst = 0.0
    for size, levels in ((8, 2), (16, 2), (16, 3)):
        for parallax in (False, True):
            rng = np.random.default_rng(100 * size + 10 * levels + parallax)
            d = R.reflection_sample_desc(size, levels, parallax)
            chains = _random_chains(rng, size, levels, 3)
            probes = rs.make_probes(rng.uniform(-0.3, 0.3, size=(3, 3)))
            boxes = rs.make_boxes(np.full((3, 3), -1.0), np.full((3, 3), 1.0))
            q = rs.random_queries(rng, 4000, 3)
            got = rs.model_sample(d, chains, q, probes, boxes).astype(np.float64)
            want = rs.sample_f64(d, chains, q, probes, boxes)
            dev = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
            print("float64 gate", (size, levels, parallax), "largest deviation", dev)
            worst = max(worst, dev)
            if parallax:   # the correction did something: most queries start inside their box
                plain = rs.model_sample(R.reflection_sample_desc(size, levels), chains, q)
                assert (np.abs(plain - got) > 1e-3).any(axis=1).mean() > 0.25
    print("float64 gate: largest deviation of the model", worst, "measured", MEASURED, "gate", 4 * MEASURED)
    assert worst <= 4 * MEASURED, worst


@pytest.mark.parametrize("size,levels", CASES)
def test_a_constant_map_stays_constant(W, size, levels):
    """Every texel of every level holds c > 0; the result is c (1 + e).  To first order, in units of 2^-24 (half an ulp,
    relative): the two weights of an axis, 1 - f and f, add up to 1 within 1/2 (the subtraction rounds by at most 2^-25),
    both axes 1; the product of two weights 1; its product with the texel 1; the three additions that round 3 (the one to +0
    does not): a level's value within 6.  The mix: 1 - g and g add up to 1 within 1/2; the product with the level's value 1;
    the one addition that rounds 1: 8 1/2 in all.  The bound is 9 * 2^-24; the half covers the second-order terms (~1e-13)."""
    from webgpu_raytracer_amd import renderer as R
    bound = 9 * 2.0 ** -24
    const = np.array([0.75, 3.0, 1e-3, 0.625], np.float32)
    d = R.reflection_sample_desc(size, levels)
    chains = np.broadcast_to(const, (2, int(rf.level_offsets(size, levels)[-1]), 4)).copy()
    q = rs.random_queries(np.random.default_rng(size), 3000, 2)
    out = rs.model_sample(d, chains, q).astype(np.float64)
    rel = np.abs(out / const.astype(np.float64) - 1.0).max(axis=0)
    print("constant map", (size, levels), "largest relative deviation per channel", rel.tolist(), "bound", bound)
    assert rel.max() <= bound, rel


def _pack64(dirs):
    """pack of the rule in float64: (m, 3) -> (m, 2)"""
    v = np.asarray(dirs, np.float64)
    s = 1.0 / np.abs(v).sum(axis=1)
    px, py = v[:, 0] * s, v[:, 1] * s
    ox, oy = (1.0 - np.abs(py)) * np.where(px >= 0, 1.0, -1.0), (1.0 - np.abs(px)) * np.where(py >= 0, 1.0, -1.0)
    return np.stack([np.where(v[:, 2] < 0, ox, px), np.where(v[:, 2] < 0, oy, py)], axis=1)


def _seam_paths(size):
    """(name, directions (m, 3) float64) of five great circles, each 3 texels to either side of where it crosses a seam, in
    steps of 1/16 texel of the map where they cross it: through the half planes {y = 0, +-x} and {x = 0, +-y} of the lower
    hemisphere, which are the four edges of the square, and through the -z pole, which is its four corners."""
    paths = []
    for name, P, T in (("edge +x", (0.8, 0.0, -0.6), (0.0, 1.0, 0.0)), ("edge -x", (-0.6, 0.0, -0.8), (0.0, 1.0, 0.0)),
                       ("edge +y", (0.0, 0.7, -0.714), (1.0, 0.0, 0.0)), ("edge -y", (0.0, -0.5, -0.866), (1.0, 0.0, 0.0)),
                       ("pole -z", (0.0, 0.0, -1.0), (0.8, 0.6, 0.0))):
        P, T = rs.unit(P), rs.unit(T)
        # how fast the packed point moves just behind the crossing, per radian, on the faster axis; a texel is 2 / size of q
        e = np.array([1e-4, 2e-4])
        rate = np.abs(np.diff(_pack64(np.cos(e)[:, None] * P + np.sin(e)[:, None] * T), axis=0)).max() / 1e-4
        step = (2.0 / size) / 16.0 / rate
        theta = np.arange(-3 * 16, 3 * 16 + 1) * step + step * 0.37   # no sample exactly on the seam
        paths.append((name, np.cos(theta)[:, None] * P + np.sin(theta)[:, None] * T))
    return paths


def _near_seam(dirs, size):
    """a tap of the fetch at this direction lies outside the map (float64 pack)"""
    u = (_pack64(dirs) * 0.5 + 0.5) * size - 0.5
    return ((u < 0.0) | (u > size - 1.0)).any(axis=1)


def test_the_fetch_is_continuous_across_the_seams(W):
    """Level 0 holds f(d) = 1 + 0.5 d.x + 0.3 d.y - 0.2 d.z at the texel centres of a size-16 map, sampled at roughness 0 along
    the paths of _seam_paths.  A step is `across a seam` when a tap of either of its two samples is folded.  With the rule's
    fold the largest step across a seam is at most 2x the largest in the interior of the same path; the clamp-to-edge form of
    the model breaks that by about the step ratio (16 steps to a texel).  Measured on the development host, seam / interior:
    fold 0.85 .. 1.87, clamp to edge 9.6 .. 17.3."""
    from webgpu_raytracer_amd import renderer as R
    size = 16
    d = R.reflection_sample_desc(size, 2)
    chain = rs.chain_from_levels(d, rs.affine_map(size), fill=np.nan)   # roughness 0 reads level 0 alone
    for name, dirs in _seam_paths(size):
        q = R.reflection_queries(np.zeros(3), 0, dirs, 0.0)
        seam = _near_seam(dirs, size)
        seam_step = seam[1:] | seam[:-1]
        assert seam_step.sum() >= 8 and (~seam_step).sum() >= 32, (name, int(seam_step.sum()))
        ratio = {}
        for clamp in (False, True):
            v = rs.model_sample(d, chain, q, clamp=clamp)[:, 0].astype(np.float64)
            step = np.abs(np.diff(v))
            ratio[clamp] = step[seam_step].max() / step[~seam_step].max()
        print("seam continuity", name, "largest step across the seam / in the interior: fold %.3f, clamp to edge %.3f"
              % (ratio[False], ratio[True]))
        assert ratio[False] <= 2.0, (name, ratio)
        assert ratio[True] > 4.0, (name, ratio)   # what the fold is for


@pytest.mark.parametrize("S", [4, 8, 16])
def test_the_fold_table(W, S):
    border = [(i, j) for i in range(-1, S + 1) for j in range(-1, S + 1) if i in (-1, S) or j in (-1, S)]
    assert len(border) == 4 * S + 4
    for i, j in border:
        fi, fj = rs.np_fold(S, i, j)
        assert 0 <= fi < S and 0 <= fj < S
        assert rs.model_fold(S, i, j) == fj * S + fi, (S, i, j)
    for i in range(S):
        for j in range(S):
            assert rs.model_fold(S, i, j) == j * S + i
    # the four corners are one another's diagonal neighbours: all four touch the -z pole
    e = S - 1
    assert [rs.model_fold(S, *c) for c in ((-1, -1), (S, S), (-1, S), (S, -1))] == [e * S + e, 0, e, e * S]
    # a tap across an edge is the texel mirrored along that edge
    assert rs.model_fold(S, -1, 1) == (S - 2) * S + 0 and rs.model_fold(S, S, 1) == (S - 2) * S + e
    assert rs.model_fold(S, 1, -1) == 0 * S + (S - 2) and rs.model_fold(S, 1, S) == e * S + (S - 2)


@pytest.mark.parametrize("S", [4, 8, 16])
def test_the_taps_against_numpy(W, S):
    """the four indices and weights the model exports, against the axis arithmetic in numpy float32 on rf.np_pack and np_fold"""
    F = np.float32
    from webgpu_raytracer_amd import renderer as R
    rng = np.random.default_rng(S)
    dirs = np.concatenate([rs.unit(rng.normal(size=(2000, 3))), R.octa_directions(S).reshape(-1, 3),
                           [d for _, p in _seam_paths(S) for d in p[::8]]]).astype(np.float32)
    index, weight = rs.model_taps(S, dirs)
    qx, qy = rf.np_pack(dirs[:, 0], dirs[:, 1], dirs[:, 2])
    ax = []
    for q in (qx, qy):
        u = (q * F(0.5) + F(0.5)) * F(S) - F(0.5)
        u = np.minimum(np.where(u >= F(-0.5), u, F(-0.5)), F(S) - F(0.5))
        fl = np.floor(u)
        assert u.dtype == np.float32
        ax.append((fl.astype(np.int64), u - fl))
    (i0, fx), (j0, fy) = ax
    for k, (a, b) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        i, j = rs.np_fold(S, i0 + a, j0 + b)
        assert np.array_equal(index[:, k], j * S + i), k
        w = (fx if a else F(1.0) - fx) * (fy if b else F(1.0) - fy)
        assert np.array_equal(weight[:, k].view(np.uint32), w.astype(np.float32).view(np.uint32)), k
    assert (index < S * S).all() and (weight >= 0).all() and (weight[:, 0] > 0).all()
    assert ((i0 < 0) | (i0 == S - 1) | (j0 < 0) | (j0 == S - 1)).sum() > 20   # folded taps were among them
    # a texel centre has all its weight on its own texel
    c_index, c_weight = rs.model_taps(S, R.octa_directions(S).reshape(-1, 3))
    assert np.abs(c_weight.max(axis=1) - 1.0).max() <= 1e-5
    assert np.array_equal(c_index[np.arange(S * S), c_weight.argmax(axis=1)], np.arange(S * S))


def test_parallax_known_answers(W):
    """dyadic inputs, every step exact: box [-1, 1]^3, probe at the origin, x = (0.5, 0, 0)"""
    from webgpu_raytracer_amd import renderer as R
    d = R.reflection_sample_desc(8, 2, parallax=True)
    probes, boxes = rs.make_probes([[0.0, 0.0, 0.0]]), rs.make_boxes([[-1.0, -1.0, -1.0]], [[1.0, 1.0, 1.0]])
    dirs = np.array([[1, 0, 0], [0, 1, 0], [0, 0, -2], [-1, 0, 0], [1, 1, 0], [0.5, -1, 0.25]], np.float32)
    want = np.array([[1, 0, 0], [0.5, 1, 0], [0.5, 0, -1], [-1, 0, 0], [1, 0.5, 0], [1, -1, 0.25]], np.float32)
    got = rs.model_direction(d, R.reflection_queries([0.5, 0.0, 0.0], 0, dirs, 0.0), probes, boxes)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), got
    # a probe off the centre of its box: the hit point is the same, the direction is taken from the probe
    probes = rs.make_probes([[0.25, -0.5, 0.0]])
    got = rs.model_direction(d, R.reflection_queries([0.5, 0.0, 0.0], 0, dirs[:2], 0.0), probes, boxes)
    assert got.tolist() == [[0.75, 0.5, 0.0], [0.25, 1.5, 0.0]]
    # without the flag the direction is the query's
    plain = R.reflection_sample_desc(8, 2)
    assert np.array_equal(rs.model_direction(plain, R.reflection_queries([0.5, 0.0, 0.0], 0, dirs, 0.0)), dirs)


def _setup(size=8, levels=2, n_probes=2, seed=7):
    rng = np.random.default_rng(seed)
    chains = _random_chains(rng, size, levels, n_probes)
    probes = rs.make_probes(rng.uniform(-0.25, 0.25, size=(n_probes, 3)))
    boxes = rs.make_boxes(np.full((n_probes, 3), -1.0), np.full((n_probes, 3), 1.0))
    return rng, chains, probes, boxes


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_without_the_flag_position_probes_and_boxes_are_not_read(W):
    from webgpu_raytracer_amd import renderer as R
    rng, chains, probes, boxes = _setup()
    d = R.reflection_sample_desc(8, 2)
    q = rs.random_queries(rng, 500, 2)
    want = rs.model_sample(d, chains, q, probes, boxes)
    q2 = q.copy()
    q2["position"] = np.nan
    assert _same(rs.model_sample(d, chains, q2, None, None), want)


def test_outside_the_box_or_on_a_bad_box_the_direction_is_the_querys(W):
    from webgpu_raytracer_amd import renderer as R
    rng, chains, probes, boxes = _setup()
    plain, par = R.reflection_sample_desc(8, 2), R.reflection_sample_desc(8, 2, parallax=True)
    q = rs.random_queries(rng, 500, 2)
    q["position"] = rng.uniform(-0.9, 0.9, size=(500, 3))
    want = rs.model_sample(plain, chains, q)
    assert not _same(rs.model_sample(par, chains, q, probes, boxes), want)       # inside, the flag matters
    outside = q.copy()
    outside["position"][:, 0] = 1.0 + np.float32(2.0 ** -23)                      # one ulp beyond the face
    assert _same(rs.model_sample(par, chains, outside, probes, boxes), want)
    for name, value in (("lo", np.nan), ("hi", np.nan)):
        bad = boxes.copy()
        bad[name][:, 1] = value
        assert _same(rs.model_sample(par, chains, q, probes, bad), want), name
    swapped = rs.make_boxes(boxes["hi"], boxes["lo"])                             # lo > hi: nothing is inside
    assert _same(rs.model_sample(par, chains, q, probes, swapped), want)
    nan_pos = q.copy()
    nan_pos["position"][:, 2] = np.nan
    assert _same(rs.model_sample(par, chains, nan_pos, probes, boxes), want)


def test_zero_and_nan_directions_are_deterministic_and_in_range(W):
    """pack of a zero or NaN direction is NaN in both coordinates; the clamp sends both to -0.5: the four corner texels, a
    quarter each - for every level."""
    from webgpu_raytracer_amd import renderer as R
    rng, chains, probes, boxes = _setup(16, 3)
    nan = np.nan
    dirs = np.array([[0, 0, 0], [-0.0, 0, -0.0], [nan, nan, nan], [nan, 1, 0], [0, 0, nan]], np.float32)
    for S in (16, 8, 4):
        index, weight = rs.model_taps(S, dirs[:3])
        e = S - 1
        assert index.tolist() == [[e * S + e, e, e * S, 0]] * 3 and weight.tolist() == [[0.25] * 4] * 3
    for parallax in (False, True):
        d = R.reflection_sample_desc(16, 3, parallax)
        for r in (0.0, 0.5, 1.0):
            q = R.reflection_queries([0.1, 0.2, 0.3], 1, dirs, r)
            out = rs.model_sample(d, chains, q, probes, boxes)
            assert np.isfinite(out).all() and _same(out, rs.model_sample(d, chains, q, probes, boxes))
            assert (out >= 0).all() and (out <= 4).all()                         # between the extremes of the maps


def test_a_probe_outside_the_array_gives_four_zero_words(W):
    from webgpu_raytracer_amd import renderer as R
    rng, chains, probes, boxes = _setup()
    for parallax in (False, True):
        d = R.reflection_sample_desc(8, 2, parallax)
        q = rs.random_queries(rng, 64, 2)
        q["probe"] = np.array([2, 3, 0x7fffffff, 0xffffffff], np.uint32)[np.arange(64) % 4]
        out = rs.model_sample(d, chains, q, probes, boxes)
        assert not out.view(np.uint32).any()
        q["probe"][::2] = 1
        out = rs.model_sample(d, chains, q, probes, boxes, n_probes=1)               # the second chain is there, and is not used
        assert not out.view(np.uint32).any()


def test_the_level_of_weight_zero_is_not_read(W):
    """at roughness <= 0, or NaN, levels >= 1 filled with NaN do not change a word; at roughness >= 1 the last level is read
    alone; a tap of weight zero is not read either"""
    from webgpu_raytracer_amd import renderer as R
    rng, chains, probes, boxes = _setup(16, 3)
    d = R.reflection_sample_desc(16, 3)
    off = rf.level_offsets(16, 3)
    q = rs.random_queries(rng, 400, 2)
    for r in (0.0, -0.0, -1.0, -np.inf, np.nan):
        q["roughness"] = r
        want = rs.model_sample(d, chains, q)
        poisoned = chains.copy()
        poisoned[:, off[1]:] = np.nan
        assert _same(rs.model_sample(d, poisoned, q), want), r
        assert np.isfinite(want).all()
    for r in (1.0, 1.5, np.inf):
        q["roughness"] = r
        want = rs.model_sample(d, chains, q)
        poisoned = chains.copy()
        poisoned[:, :off[2]] = np.nan
        assert _same(rs.model_sample(d, poisoned, q), want), r
        assert np.isfinite(want).all()
    # in between both levels count
    q["roughness"] = 0.75
    poisoned = chains.copy()
    poisoned[:, off[1]:off[2]] = np.nan
    assert np.isnan(rs.model_sample(d, poisoned, q)).all()
    # a texel centre has the weight 1 * 1 on its own texel and exactly 0 on the other three: NaNs around it do not reach it
    # (not normalised, so that pack is exact: |x| + |y| + |z| = 1)
    centres = R.reflection_queries(np.zeros(3), 0, [[-0.25, -0.25, 0.5], [0.25, -0.25, 0.5], [-0.25, 0.25, 0.5], [0.25, 0.25, 0.5]], 1.0)
    index, weight = rs.model_taps(4, centres["direction"])
    assert sorted(weight[0].tolist()) == [0.0, 0.0, 0.0, 1.0]
    poisoned = chains.copy()
    last = poisoned[0, off[2]:].reshape(4, 4, 4)
    keep = last[1:3, 1:3].copy()
    last[:] = np.nan
    last[1:3, 1:3] = keep
    out = rs.model_sample(d, poisoned, centres)
    assert _same(out, keep.reshape(4, 4))
