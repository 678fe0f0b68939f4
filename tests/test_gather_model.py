"""The reference model of the irradiance gathers (tests/model/gather_model.cpp) on the CPU: a gather is bit for bit the
composition of the radiance model's queries on the model's exported directions; the directions are unit, in the hemisphere
and cosine-distributed; in a closed emitting box every point gathers the emitted radiance exactly; under a square light the
gathered mean is the point-to-rectangle form factor (the cosine weighting, and no factor pi).  No GPU needed."""
import numpy as np
import pytest

import gather_util as gu
import parity_util as pu
import radiance_util as ru
import random_scene
import ray_query_util as rq
from test_bvh_independent import _random_rays
from test_radiometric_kat import _ceiling_form_factor, furnace_floor_bridge

LE = np.array([2.0, 1.0, 0.5], dtype=np.float32)
RHO = np.array([128, 204, 51], dtype=np.float32) / np.float32(255)


def _floor_points(n, extent, seed):
    """n points on the floor of the box [-1, 1]^3 at y = -1 + 0.01 with |x|, |z| <= extent, normal +y, pads 7 i + 3"""
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 8), np.float32)
    p[:, 0] = rng.uniform(-extent, extent, n)
    p[:, 1] = np.float32(-1.0 + 0.01)
    p[:, 2] = rng.uniform(-extent, extent, n)
    p[:, 3] = np.float32(1e30)
    p[:, 5] = 1.0
    return ru.with_pads(p)


def _scene(W, which):
    if which == "cornell":
        b = pu.bridge_for(W, "cornell")
        m = gu.model_for(W, b)
        return m, gu.scene_points(m, b)[:256]
    b = random_scene.make(2, with_textures=True)
    m = gu.model_for(W, b)
    return m, gu.points_from_rays(m, ru.with_pads(rq.to_rt_rays(_random_rays(b, 256, 42))))


@pytest.mark.parametrize("which", ["cornell", "random_textured"])
def test_a_gather_is_the_composition_of_radiance_queries(W, which):
    m, points = _scene(W, which)
    n = points.shape[0]
    for depth, spp, seed in ((4, 3, gu.SEED), (6, 1, 11), (0, 2, 1)):
        out, hits, counts = m.gatherIrradiance(points, depth, spp, seed)
        dirs = m.gatherDirections(points, spp, seed)
        want, want_hits, each = gu.compose(m.traceRadiance, points, dirs, depth, spp, seed)
        tag = (which, depth, spp)
        assert np.array_equal(ru.u32(out), ru.u32(want)), (tag, int((ru.u32(out) != ru.u32(want)).any(axis=1).sum()))
        assert np.array_equal(hits, want_hits), tag
        assert np.array_equal(counts, sum(each)), tag           # the stats of a gather are the sums of the composed queries'
        assert int(counts[:, 0].min()) >= spp                    # every first segment is an extension ray
        if depth == 4:   # the check must not pass on darkness (the random scenes are sparse: objects in open space)
            some_hit, lit = int((hits > 0).sum()), int((out[:, :3].max(axis=1) > 0).sum())
            print(tag, "points with a hit sample", some_hit, "lit", lit, "of", n)
            assert (some_hit >= n // 2 and lit >= n // 5) if which == "cornell" else (some_hit >= 16 and lit >= 4), tag
        if depth == 0:
            assert not ru.u32(out[:, :3]).any() and np.array_equal(counts[:, 0], np.full(n, spp, np.uint64)), tag
            assert not counts[:, 1:3].any(), tag


@pytest.mark.parametrize("normal", [(0.0, 1.0, 0.0), (0.3, -0.2, -0.9), (-2.0, 0.5, 1.0), (0.0, 0.0, -1.0)])
def test_directions_are_cosine_distributed(normal):
    m = gu.GatherModel()
    spp = 65536
    p = np.zeros((1, 8), np.float32)
    p[0, 4:7] = normal
    p.view(np.uint32)[0, 7] = 12345
    d = m.gatherDirections(p, spp, 3)[0].astype(np.float64)
    n = np.asarray(normal, np.float64)
    n /= np.linalg.norm(n)
    cos = d @ n
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 1e-5
    assert cos.min() >= -1e-6
    assert abs(cos.mean() - 2.0 / 3.0) < 0.01, cos.mean()       # about ten standard errors: 0.2357 / 256
    tangent = d - cos[:, None] * n[None, :]
    assert np.abs(tangent.mean(axis=0)).max() < 0.01, tangent.mean(axis=0)
    # the samples of one point differ from each other and from another stream's
    assert np.unique(d, axis=0).shape[0] > spp - 64
    p.view(np.uint32)[0, 7] = 12346
    assert not np.array_equal(m.gatherDirections(p, 16, 3)[0], d[:16].astype(np.float32))


def test_exact_furnace(W):
    """Every direction of the upper hemisphere ends on an emitter of radiance le: each sample is le, and the mean of eight
    equal samples of (2, 1, 0.5) is exact."""
    b = furnace_floor_bridge(RHO, LE)
    m = gu.model_for(W, b)
    points = _floor_points(64, 0.95, 5)
    out, hits, counts = m.gatherIrradiance(points, 1, 8, gu.SEED)
    assert np.array_equal(ru.u32(out[:, :3]), ru.u32(np.broadcast_to(LE, (64, 3))))
    assert np.array_equal(ru.u32(out[:, 3]), ru.u32(np.ones(64, np.float32))) and (hits == 8).all()
    assert np.array_equal(counts[:, 0], np.full(64, 8, np.uint64))


def test_known_answer_under_a_square_light(W):
    """Only the ceiling emits, max_depth = 1: a sample is le when its direction reaches the ceiling and 0 otherwise, so the
    mean of rgb / le is the cosine-weighted solid angle of the ceiling over pi = the form factor - without a factor pi."""
    b = furnace_floor_bridge(RHO, LE, True, emitting=("ceiling",))
    m = gu.model_for(W, b)
    points = _floor_points(256, 0.8, 6)
    out, hits, _ = m.gatherIrradiance(points, 1, 64, gu.SEED)
    assert (hits == 64).all()                                   # a closed box
    ratio = out[:, :3].astype(np.float64) / LE.astype(np.float64)
    assert np.array_equal(ratio[:, 0], ratio[:, 1]) and np.array_equal(ratio[:, 0], ratio[:, 2])
    F = _ceiling_form_factor(points[:, 0].astype(np.float64), points[:, 2].astype(np.float64))
    assert 0.15 < F.min() and F.max() < 0.25
    err = ratio[:, 0] - F
    stderr = err.std(ddof=1) / np.sqrt(err.size)
    print("mean ratio", ratio[:, 0].mean(), "mean F", F.mean(), "stderr", stderr)
    assert abs(ratio[:, 0].mean() - F.mean()) < 5 * stderr, (ratio[:, 0].mean(), F.mean(), stderr)
    assert stderr < 0.01                                       # the bound above means something
