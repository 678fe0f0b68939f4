"""The reflection sampler on the GPU (rt_sample_reflection, k_reflection_sample<PARALLAX>) against the reference model
(tests/model/reflection_sample_model.cpp), bit for bit - where the model has a NaN, a NaN of any payload: chains with NaN,
infinities, denormals and -0 under the hostile query set of reflection_sample_util, in both kernel forms, through the host
entry and the device entry, at query counts that straddle a wave and a workgroup; a Cornell bake sampled at its own texel
centres; and a sample call between frames, which changes nothing of the render or of the reflection stats."""
import numpy as np
import pytest

import parity_util as pu
import probe_util as prb
import reflection_sample_util as rs
import reflection_util as rf
from test_gpu_irradiance_gather import _render

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 257)


@pytest.mark.parametrize("parallax", [False, True])
@pytest.mark.parametrize("n_probes", [1, 3])
@pytest.mark.parametrize("size,levels", [(8, 2), (16, 3)])
def test_bit_parity_with_the_model(W, gpu_renderer, size, levels, n_probes, parallax):
    import torch
    from webgpu_raytracer_amd import renderer as R
    r = gpu_renderer                                                 # nothing uploaded: the sampler needs no scene
    d = R.reflection_sample_desc(size, levels, parallax)
    chains = rs.hostile_chains(size, levels, n_probes)
    probes, boxes = rs.hostile_boxes(n_probes)
    queries = rs.hostile_queries(size, levels, n_probes)
    want = rs.model_sample(d, chains, queries, probes, boxes)
    # parity must not pass on blandness: NaN and infinite results, results of a skipped probe, finite ones
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).all(axis=1).sum() > len(want) // 4
    assert 0 < (~want.view(np.uint32).any(axis=1)).sum() < len(want) // 2
    if parallax:
        plain = rs.model_sample(R.reflection_sample_desc(size, levels), chains, queries)
        assert (plain.view(np.uint32) != want.view(np.uint32)).any(axis=1).mean() > 0.1
    tag = (size, levels, n_probes, parallax)
    args = (probes, boxes) if parallax else ()
    d_chains = torch.from_numpy(chains.copy()).cuda()
    d_queries = torch.from_numpy(rs._words(queries, R.REFLECTION_QUERY_DTYPE).copy()).cuda()
    d_probes = torch.from_numpy(rs._words(probes, R.PROBE_DTYPE).copy()).cuda()
    d_boxes = torch.from_numpy(rs._words(boxes, R.REFLECTION_BOX_DTYPE).copy()).cuda()
    dev = dict(probes_ptr=d_probes.data_ptr(), boxes_ptr=d_boxes.data_ptr()) if parallax else {}
    for n in COUNTS + (len(queries),):
        got = r.sampleReflection(d, chains, queries[:n], *args)
        assert got.shape == (n, 4)
        rs.check_words(got, want[:n], tag + ("host", n))
        d_out = torch.full((n + 1, 4), -7.0, dtype=torch.float32, device="cuda")
        r.sampleReflectionDevice(d, d_chains.data_ptr(), n_probes, d_queries.data_ptr(), n, d_out.data_ptr(), **dev)
        r.sync()
        out = d_out.cpu().numpy()
        assert np.array_equal(out[:n].view(np.uint32), got.view(np.uint32)), tag + ("device", n)
        assert (out[n] == -7.0).all(), tag + ("wrote past n", n)
    # the queries in another order and another cut give the same words: a result depends on its own query alone
    perm = np.random.default_rng(1).permutation(len(queries))[:300]
    rs.check_words(r.sampleReflection(d, chains, queries[perm], *args), want[perm], tag + ("permuted",))
    assert r.sampleReflection(d, chains, queries[:0], *args).shape == (0, 4)


def test_every_refusal_on_a_live_context(W, gpu_renderer):
    """the refusals of test_reflection_sample_abi.py on a context of this device, with nothing uploaded"""
    from webgpu_raytracer_amd import renderer as R
    from test_reflection_sample_abi import check_refusals
    check_refusals(R, R.load_library(), gpu_renderer.ctx)
    d = R.reflection_sample_desc(16, 3, parallax=True)
    assert R.load_library().rt_sample_reflection(gpu_renderer.ctx, d.ctypes.data, None, 0, None, None, None, 0, None) == 0


def test_a_cornell_bake_sampled_at_its_texel_centres(W, gpu_renderer):
    """End to end: bake two probes at size 16, 3 levels, then sample the GPU's own chains at octa_directions(16), roughness 0:
    the sampler's words equal the model's on those chains, and - the centres having nearly all their weight on their own
    texel - lie close to level 0 itself."""
    from webgpu_raytracer_amd import renderer as R
    r = gpu_renderer
    b = pu.bridge_for(W, "cornell")
    W.upload_scene(r, b, 16, 16)
    lo, hi = prb.scene_bounds(b)
    probes = prb.make_probes(np.stack([0.5 * (lo + hi), lo + 0.25 * (hi - lo)]), pad_first=17)
    chains = r.bakeReflection(R.reflection_desc(16, 3, 2, 64), probes, 4, 5)
    assert (chains[..., :3] > 0).mean() > 0.25 and (chains[..., 3] > 0).mean() > 0.5
    dirs = R.octa_directions(16).reshape(-1, 3)
    q = np.concatenate([R.reflection_queries(np.zeros(3), p, dirs, 0.0) for p in (0, 1)])
    d = R.reflection_sample_desc(16, 3)
    got = r.sampleReflection(d, chains, q)
    rs.check_words(got, rs.model_sample(d, chains, q), "cornell bake, roughness 0")
    level0 = chains[:, :256].reshape(512, 4)
    assert np.abs(got - level0).max() <= 1e-4 * max(1.0, float(np.abs(level0).max()))
    # and in between the levels, with the box of the room
    boxes = rs.make_boxes(np.stack([lo, lo]), np.stack([hi, hi]))
    q["roughness"] = 0.6
    q["position"] = lo + 0.4 * (hi - lo)
    dp = R.reflection_sample_desc(16, 3, parallax=True)
    got = r.sampleReflection(dp, chains, q, probes, boxes)
    rs.check_words(got, rs.model_sample(dp, chains, q, probes, boxes), "cornell bake, roughness 0.6, parallax")
    assert (got[:, :3] > 0).mean() > 0.25


def test_a_sample_call_leaves_the_render_and_the_reflection_stats_alone(W):
    """Frames 1-4, a bake, sample calls of both forms, frames 5-8 against the same frames with the bake alone: accumulation,
    presented image, counters, G-buffer and uniforms are equal, and reflectionStats() reads the same before and after."""
    from webgpu_raytracer_amd import renderer as R
    b = pu.bridge_for(W, "cornell")
    W._build.build_rt()
    lo, hi = prb.scene_bounds(b)
    probes = prb.make_probes(np.stack([0.5 * (lo + hi)]), pad_first=3)
    bake_desc = R.reflection_desc(8, 2, 2, 64)
    q = rs.hostile_queries(8, 2, 1)[:200]
    boxes = rs.make_boxes([lo], [hi])

    def run(sample):
        def between(r):
            chains, st = r.bakeReflection(bake_desc, probes, 4, 5, stats=True)
            if sample:
                for parallax in (False, True):
                    d = R.reflection_sample_desc(8, 2, parallax)
                    got = r.sampleReflection(d, chains, q, probes, boxes)
                    rs.check_words(got, rs.model_sample(d, chains, q, probes, boxes), ("between frames", parallax))
                assert r.reflectionStats() == st
        return _render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), between)

    got, want = run(True), run(False)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "accumulation"
    assert np.array_equal(got[1], want[1]), "captureFrame"
    assert got[2] == want[2], (got[2], want[2])
    for a, w in zip(got[3], want[3]):
        assert np.array_equal(pu.bits(a), pu.bits(w)), "G-buffer"
    assert np.array_equal(got[4], want[4]), "uniforms"
