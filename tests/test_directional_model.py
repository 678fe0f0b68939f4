"""The reference model of the directional gathers (tests/model/directional_model.cpp) on the CPU: its directions are the probe
model's on the same pads with the sign flipped exactly where the f32 dot with the normal is negative; a directional gather is
bit for bit the fixed-tree band 0 .. 1 projection of the radiance model's queries on the model's exported directions - on the
plain rays at seed = f and on the pad' rays at seed = 0 alike; in a closed emitting box band 0 is the emitted radiance over the
hemisphere, band 1 points along the normal and sh4_irradiance gives pi * le; sh4_irradiance gives the analytic irradiance of
a constant and of a linear radiance field cut to a hemisphere.  No GPU needed."""
import numpy as np
import pytest

import directional_util as du
import gather_util as gu
import parity_util as pu
import probe_util as prb
import radiance_util as ru
import random_scene
import ray_query_util as rq
from test_bvh_independent import _random_rays
from test_radiometric_kat import furnace_floor_bridge

LE = np.array([2.0, 1.0, 0.5], dtype=np.float32)
RHO = np.array([128, 204, 51], dtype=np.float32) / np.float32(255)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1)[..., None]


def test_directions_are_the_probe_rules_mirrored_into_the_hemisphere():
    """On the same pads: the probe model's direction, negated exactly where (d0.x * N.x + d0.y * N.y) + d0.z * N.z < 0 in f32;
    for unit normals every direction has a dot >= 0; a zero or NaN normal flips nothing."""
    m, pm = du.DirectionalModel(), prb.ProbeModel()
    rng = np.random.default_rng(9)
    n, spp, seed = 64, 257, 5
    normals = _unit(rng.normal(size=(n, 3))).astype(np.float32)
    normals[:3] = [(0, 1, 0), (0, 0, -1), (1, 0, 0)]
    points = du.make_points(rng.normal(size=(n, 3)), normals)
    d0 = pm.probeDirections(points, spp, seed)
    d = m.directions(points, spp, seed)
    N = normals[:, None, :]
    c = (d0[..., 0] * N[..., 0] + d0[..., 1] * N[..., 1]) + d0[..., 2] * N[..., 2]
    assert c.dtype == np.float32
    flip = c < 0
    assert 0.4 < flip.mean() < 0.6, flip.mean()
    want = np.where(flip[..., None], -d0, d0)
    assert np.array_equal(ru.u32(d), ru.u32(want))
    dot = (d.astype(np.float64) * normals.astype(np.float64)[:, None, :]).sum(axis=2)
    assert dot.min() >= 0.0, dot.min()
    assert np.abs((d.astype(np.float64) ** 2).sum(axis=2) - 1.0).max() <= 1e-6
    # normals the dot cannot order: nothing flips
    odd = du.make_points(np.zeros((2, 3)), [(0, 0, 0), (np.nan, 1, 0)])
    assert np.array_equal(ru.u32(m.directions(odd, spp, seed)), ru.u32(pm.probeDirections(odd, spp, seed)))
    # a normal that is not unit flips by its sign alone (a power of two scales every product and the sum exactly)
    big = points.copy()
    big[:, 4:7] *= np.float32(-2.0 ** 100)
    assert np.array_equal(ru.u32(m.directions(big, spp, seed)), ru.u32(np.where((c > 0)[..., None], -d0, d0)))


def _scene(W, which):
    if which == "cornell":
        b = pu.bridge_for(W, "cornell")
        m = du.model_for(W, b)
        return m, gu.scene_points(m, b)[:128]
    b = random_scene.make(2, with_textures=True)
    m = du.model_for(W, b)
    return m, gu.points_from_rays(m, ru.with_pads(rq.to_rt_rays(_random_rays(b, 128, 42))))


@pytest.mark.parametrize("which", ["cornell", "random_textured"])
def test_a_directional_gather_is_the_projection_of_radiance_queries(W, which):
    """... on the plain rays {position, t_max, d, pad} at seed = f, one query per sample, and through a single query on the
    pad' rays at seed = 0: words, hit counts and ray / hit / node counters."""
    m, points = _scene(W, which)
    n = points.shape[0]
    assert n == 128
    for depth, spp, seed in ((4, 3, du.SEED), (4, 80, 2), (6, 1, 11), (0, 65, 1)):
        out, hits, counts = m.gatherDirectional(points, depth, spp, seed)
        dirs = m.directions(points, spp, seed)
        tag = (which, depth, spp)
        want, want_hits, each = du.compose(m.traceRadiance, points, dirs, depth, spp, seed)
        assert np.array_equal(ru.u32(out), ru.u32(want)), (tag, int((ru.u32(out) != ru.u32(want)).any(axis=1).sum()))
        assert np.array_equal(hits, want_hits), tag
        assert np.array_equal(counts, sum(each)), tag            # the stats of a gather are the sums of the composed queries'
        assert np.array_equal(counts[:, 0] >= spp, np.ones(n, bool))   # every first segment is an extension ray
        # the pad' identity: init_rng(pad + f * 719393, 0) == init_rng(pad, f)
        want2, hits2, per_ray = du.compose_pad_prime(m.traceRadiance, points, dirs, depth, spp, seed)
        assert np.array_equal(ru.u32(out), ru.u32(want2)), (tag, "pad'")
        assert np.array_equal(hits, hits2), (tag, "pad'")
        assert np.array_equal(counts, per_ray.reshape(n, spp, 5).sum(axis=1)), (tag, "pad'")
        rows = out.reshape(n, 4, 4)
        assert np.array_equal(ru.u32(rows[:, :, 3]), ru.u32(np.repeat(rows[:, :1, 3], 4, axis=1))), tag   # one hit fraction
        if depth == 4:   # the check must not pass on darkness (the random scenes are sparse: objects in open space)
            some_hit, lit = int((hits > 0).sum()), int((np.abs(rows[:, :, :3]).max(axis=(1, 2)) > 0).sum())
            band1 = int((np.abs(rows[:, 1:, :3]).max(axis=(1, 2)) > 0).sum())
            print(tag, "points with a hit sample", some_hit, "lit", lit, "with a band-1 word", band1, "of", n)
            assert (some_hit >= n // 2 and lit >= n // 4) if which == "cornell" else (some_hit >= 8 and lit >= 2), tag
            assert band1 == lit, tag
        if depth == 0:
            assert not ru.u32(rows[:, :, :3]).any(), tag           # all twelve coefficient words are +0
            assert np.array_equal(counts[:, 0], np.full(n, spp, np.uint64)) and not counts[:, 1:3].any(), tag


def test_closed_emitting_box(W):
    """Every direction ends on an emitter of radiance le, max_depth = 1: every sample is le, so band 0 sums equal values - le
    * 2 pi * Y0 within spp roundings of 2^-24 - and band 1 estimates the integral of le * Y1 w over the hemisphere of n,
    0.488602512 * pi * le * n, with a Monte-Carlo error of at most 2 pi * 0.488602512 * le / sqrt(spp) per component (the
    variance of a direction component is at most 1); bound: six of those.  sh4_irradiance at n is then pi * le."""
    from webgpu_raytracer_amd.renderer import sh4_irradiance
    b = furnace_floor_bridge(RHO, LE, emitting=("floor", "ceiling", "x-", "x+", "z-", "z+"))
    m = du.model_for(W, b)
    spp = 4096
    normals = _unit([(0.0, 1.0, 0.0), (0.3, -0.2, -0.9), (-2.0, 0.5, 1.0)])
    points = du.make_points([[0.1, -0.2, 0.3], [0.0, 0.0, 0.0], [-0.7, 0.6, 0.2]], normals)
    out, hits, counts = m.gatherDirectional(points, 1, spp, du.SEED)
    rows = out.reshape(3, 4, 4)
    assert (hits == spp).all() and np.array_equal(ru.u32(rows[:, :, 3]), ru.u32(np.ones((3, 4), np.float32)))
    sh = rows[:, :, :3].astype(np.float64)
    le = LE.astype(np.float64)
    want0 = le * 2.0 * np.pi * 0.282094792
    rel0 = spp * 2.0 ** -24
    rel = np.abs(sh[:, 0, :] - want0) / want0
    print("band 0 relative error", rel.max(), "bound", rel0)
    assert rel.max() <= rel0
    xyz = np.stack([sh[:, 3, :], sh[:, 1, :], sh[:, 2, :]], axis=1)              # (point, component x y z, colour)
    want1 = 0.488602512 * np.pi * le[None, None, :] * normals[:, :, None]
    bound1 = 6.0 * 2.0 * np.pi * 0.488602512 * le / np.sqrt(spp)
    print("largest band-1 error / bound", (np.abs(xyz - want1) / bound1).max())
    assert (np.abs(xyz - want1) <= bound1).all()
    # the irradiance at n: linear in the coefficients, so its bound follows from the two above
    E = sh4_irradiance(np.moveaxis(rows, 1, 0), normals)
    assert E.shape == (3, 3)
    boundE = (np.pi * 0.282094792 * rel0 * want0)[None, :] + \
        (2.0 * np.pi / 3.0) * 0.488602512 * np.abs(normals).sum(axis=1)[:, None] * bound1[None, :]
    print("largest irradiance error / bound", (np.abs(E - np.pi * le) / boundE).max())
    assert (np.abs(E - np.pi * le) <= boundE).all()


def _hemisphere_coefficients(axis, radiance):
    """The band 0 .. 1 coefficients (4,) of radiance(w) cut to the hemisphere of the unit vector `axis`, by a quadrature that
    is exact for polynomials: Gauss-Legendre in the cosine to the axis, equal steps in the angle around it."""
    mu, wmu = np.polynomial.legendre.leggauss(16)
    mu, wmu = 0.5 * (mu + 1.0), 0.5 * wmu                                      # (0, 1)
    phi = (np.arange(32) + 0.5) * (2.0 * np.pi / 32)
    t = _unit(np.cross(axis, [1.0, 0.0, 0.0] if abs(axis[0]) < 0.9 else [0.0, 1.0, 0.0]))
    u = np.cross(axis, t)
    s = np.sqrt(1.0 - mu * mu)
    w = (mu[:, None, None] * axis + s[:, None, None] * (np.cos(phi)[None, :, None] * t + np.sin(phi)[None, :, None] * u))
    dw = (wmu[:, None] * (2.0 * np.pi / 32)) * np.ones((1, 32))
    L = radiance(w)
    Y = np.stack([np.full(L.shape, 0.282094792), 0.488602512 * w[..., 1], 0.488602512 * w[..., 2], 0.488602512 * w[..., 0]])
    return (Y * L * dw).sum(axis=(1, 2))


def test_sh4_irradiance_of_constant_and_linear_radiance_on_a_hemisphere():
    """L = 1 on the hemisphere of a, 0 below: E(n) = pi / 2 + (pi / 2)(a . n).  L = w . b there: E(n) = (pi / 4)(a . b) + (pi /
    3)(b . n).  (Both are what the band 0 .. 1 reconstruction gives, not the true clamped-cosine integral.)"""
    from webgpu_raytracer_amd.renderer import DIRECTIONAL_DTYPE, IRRADIANCE_DTYPE, sh4_irradiance
    rng = np.random.default_rng(4)
    normals = _unit(rng.normal(size=(64, 3)))
    a = _unit([0.3, -0.5, 0.2])
    bvec = np.array([0.7, 0.1, -0.4])
    c_const = _hemisphere_coefficients(a, lambda w: np.ones(w.shape[:-1]))
    c_lin = _hemisphere_coefficients(a, lambda w: w @ bvec)
    assert np.abs(c_const - np.array([0.282094792 * 2 * np.pi, *(0.488602512 * np.pi * a[[1, 2, 0]])])).max() <= 1e-9
    for c, want in ((c_const, np.pi / 2 + (np.pi / 2) * (normals @ a)),
                    (c_lin, (np.pi / 4) * (a @ bvec) + (np.pi / 3) * (normals @ bvec))):
        coeffs = np.repeat(c[:, None, None], 3, axis=2) * np.ones((1, 64, 1))  # (4, 64, 3): one colour three times
        E = sh4_irradiance(coeffs, normals)
        assert E.shape == (64, 3) and np.abs(E - want[:, None]).max() <= 1e-7, np.abs(E - want[:, None]).max()
        # the same through the two array types of the bindings: four atlas layers, and gather results
        layers = np.zeros((4, 8, 8), IRRADIANCE_DTYPE)
        layers["rgb"] = coeffs.reshape(4, 8, 8, 3)
        layers["hit_fraction"] = 1.0
        assert np.abs(sh4_irradiance(layers, normals.reshape(8, 8, 3)).reshape(64, 3) - want[:, None]).max() <= 1e-6
        res = np.zeros(64, DIRECTIONAL_DTYPE)
        res["layer"][:, :, :3] = np.moveaxis(coeffs, 0, 1)
        assert np.abs(sh4_irradiance(res, normals) - want[:, None]).max() <= 1e-6
