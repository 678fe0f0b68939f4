"""The reference model of the probe gathers (tests/model/probe_model.cpp) on the CPU: its directions are unit and uniform on
the sphere; a probe gather is bit for bit the fixed-tree SH9 projection of the radiance model's queries on the model's
exported directions - on the plain rays at seed = f and on the pad' rays at seed = 0 alike; in a closed emitting box band 0
is the emitted radiance and the higher bands vanish within the estimator's noise; sh9_irradiance gives the analytic
irradiance of a constant and of a linear radiance field.  No GPU needed."""
import numpy as np
import pytest

import parity_util as pu
import probe_util as prb
import radiance_util as ru
import random_scene
from test_radiometric_kat import furnace_floor_bridge

LE = np.array([2.0, 1.0, 0.5], dtype=np.float32)
RHO = np.array([128, 204, 51], dtype=np.float32) / np.float32(255)


def test_directions_are_uniform_on_the_sphere():
    m = prb.ProbeModel()
    N = 1 << 16
    p = prb.make_probes(np.zeros((1, 3)), pad_first=12345)
    d = m.probeDirections(p, N, 3)[0].astype(np.float64)
    assert np.abs((d * d).sum(axis=1) - 1.0).max() <= 1e-6
    sigma = np.sqrt(1.0 / (3.0 * N))                             # a component of a uniform unit vector has variance 1 / 3
    print("component means / sigma", (d.mean(axis=0) / sigma).tolist())
    assert np.abs(d.mean(axis=0)).max() <= 6.0 * sigma, d.mean(axis=0)
    sigma_z2 = np.sqrt(4.0 / (45.0 * N))                         # var(z^2) = 1 / 5 - 1 / 9
    z2 = (d[:, 2] ** 2).mean()
    print("mean z^2", z2, "in sigmas", (z2 - 1.0 / 3.0) / sigma_z2)
    assert abs(z2 - 1.0 / 3.0) <= 6.0 * sigma_z2, z2
    # the samples of one probe differ from each other and from another stream's
    assert np.unique(d, axis=0).shape[0] > N - 64
    q = prb.make_probes(np.zeros((1, 3)), pad_first=12346)
    assert not np.array_equal(m.probeDirections(q, 16, 3)[0], d[:16].astype(np.float32))


def _scene(W, which):
    b = pu.bridge_for(W, "cornell") if which == "cornell" else random_scene.make(2, with_textures=True)
    m = prb.model_for(W, b)
    return m, prb.scene_probes(m, b)


@pytest.mark.parametrize("which", ["cornell", "random_textured"])
def test_a_probe_gather_is_the_projection_of_radiance_queries(W, which):
    """... on the plain rays {position, t_max, d, pad} at seed = f, one query per sample, and through a single query on the
    pad' rays at seed = 0: words, hit counts and ray / hit / node counters."""
    m, probes = _scene(W, which)
    n = probes.shape[0]
    assert n == 96
    for depth, spp, seed in ((4, 3, prb.SEED), (4, 80, 2), (6, 1, 11), (0, 65, 1)):
        out, hits, counts = m.gatherProbes(probes, depth, spp, seed)
        dirs = m.probeDirections(probes, spp, seed)
        tag = (which, depth, spp)
        want, want_hits, each = prb.compose(m.traceRadiance, probes, dirs, depth, spp, seed)
        assert np.array_equal(ru.u32(out), ru.u32(want)), (tag, int((ru.u32(out) != ru.u32(want)).any(axis=1).sum()))
        assert np.array_equal(hits, want_hits), tag
        assert np.array_equal(counts, sum(each)), tag            # the stats of a probe gather are the sums of the composed queries'
        assert np.array_equal(counts[:, 0] >= spp, np.ones(n, bool))   # every first segment is an extension ray
        # the pad' identity: init_rng(pad + f * 719393, 0) == init_rng(pad, f)
        want2, hits2, per_ray = prb.compose_pad_prime(m.traceRadiance, probes, dirs, depth, spp, seed)
        assert np.array_equal(ru.u32(out), ru.u32(want2)), (tag, "pad'")
        assert np.array_equal(hits, hits2), (tag, "pad'")
        assert np.array_equal(counts, per_ray.reshape(n, spp, 5).sum(axis=1)), (tag, "pad'")
        if depth == 4:   # the check must not pass on darkness
            some_hit, lit = int((hits > 0).sum()), int((np.abs(out[:, :3]).max(axis=1) > 0).sum())
            print(tag, "probes with a hit sample", some_hit, "lit", lit, "of", n)
            assert (some_hit >= n // 2 and lit >= n // 4) if which == "cornell" else (some_hit >= 8 and lit >= 2), tag
        if depth == 0:
            assert not ru.u32(out[:, :27]).any() and np.array_equal(counts[:, 0], np.full(n, spp, np.uint64)), tag
            assert not counts[:, 1:3].any(), tag


def test_closed_emitting_box(W):
    """Every direction ends on an emitter of radiance le, max_depth = 1: every sample is le, so band 0 sums equal values -
    le * 4 pi * Y0 within spp roundings of 2^-24 - and every higher coefficient is pure Monte-Carlo noise of variance
    (4 pi)^2 le^2 (1 / 4 pi) / spp."""
    b = furnace_floor_bridge(RHO, LE, emitting=("floor", "ceiling", "x-", "x+", "z-", "z+"))
    m = prb.model_for(W, b)
    spp = 4096
    probes = prb.make_probes([[0.1, -0.2, 0.3], [0.0, 0.0, 0.0], [-0.7, 0.6, 0.2]])
    out, hits, counts = m.gatherProbes(probes, 1, spp, prb.SEED)
    assert (hits == spp).all() and np.array_equal(ru.u32(out[:, 27]), ru.u32(np.ones(3, np.float32)))
    sh = out[:, :27].reshape(3, 9, 3).astype(np.float64)
    le = LE.astype(np.float64)
    want0 = le * 12.566370614 * 0.282094792
    rel = np.abs(sh[:, 0, :] - want0) / want0
    print("band 0 relative error", rel.max(), "bound", spp * 2.0 ** -24)
    assert rel.max() <= spp * 2.0 ** -24
    bound = 6.0 * le * np.sqrt(4.0 * np.pi / spp)
    print("largest |sh[k > 0]| / bound", (np.abs(sh[:, 1:, :]) / bound).max())
    assert (np.abs(sh[:, 1:, :]) <= bound).all()


def test_sh9_irradiance_of_constant_and_linear_radiance():
    """L = 1 has the single coefficient sqrt(4 pi) and irradiance pi at every normal; L = 1 + w . a adds the band-1
    coefficients sqrt(4 pi / 3) (a_y, a_z, a_x) and the irradiance (2 pi / 3)(n . a)."""
    from webgpu_raytracer_amd.renderer import sh9_irradiance
    rng = np.random.default_rng(4)
    normals = rng.normal(size=(64, 3))
    normals /= np.linalg.norm(normals, axis=1)[:, None]
    sh = np.zeros((9, 3))
    sh[0, :] = np.sqrt(4.0 * np.pi)
    E = sh9_irradiance(sh, normals)
    assert E.shape == (64, 3) and np.abs(E - np.pi).max() <= 1e-5
    a = np.array([0.3, -0.5, 0.2])
    sh[1, :], sh[2, :], sh[3, :] = np.sqrt(4.0 * np.pi / 3.0) * a[1], np.sqrt(4.0 * np.pi / 3.0) * a[2], np.sqrt(4.0 * np.pi / 3.0) * a[0]
    E = sh9_irradiance(sh, normals)
    want = np.pi + (2.0 * np.pi / 3.0) * (normals @ a)
    assert np.abs(E - want[:, None]).max() <= 1e-5
    # a batch of probes: (n, 9, 3) -> (n, m, 3)
    assert sh9_irradiance(np.stack([sh, sh]), normals).shape == (2, 64, 3)
