"""Directional gathers on the GPU (rt_gather_directional: k_dir_rays -> k_radiance_query -> k_dir_project) against the reference
model (tests/model/directional_model.cpp, tied to the radiance model by tests/test_directional_model.py), point by point: the
twelve coefficients and the four hit fractions bit for bit, the ray, hit, node and triangle counters as sums, in the LDS and
the global-memory form, at sample counts below, at and above 16 and the 64 lanes of the projection; the composition identity
on the GPU's own radiance queries; a call that is cut into two batches; the device entry; degenerate normals, t_max and
positions; no side effect on a render or on the other path queries' state."""
import numpy as np
import pytest

import directional_util as dru
import gather_util as gu
import parity_util as pu
import probe_util as prb
import radiance_util as ru
from test_gpu_irradiance_gather import _render, _renderer

pytestmark = pytest.mark.gpu

RT_ERR_INVALID = -1
DEPTHS = (0, 1, 4)
SPPS = (1, 3, 16, 17, 64, 65, 80)   # a quarter of the lanes and one more, one sample per lane, lanes with one and with two
_cache = {}


def _scene(W, scene):
    """(bridge, model, points) of a scene, made once: the 1 024 points of the gather tests, pads 7 i + 3"""
    if scene not in _cache:
        b = pu.bridge_for(W, scene)
        m = dru.model_for(W, b)
        points = gu.scene_points(m, b)
        points.setflags(write=False)
        _cache[scene] = (b, m, points, {})
    return _cache[scene][:3]


def _ref(W, scene, depth, spp):
    """the model's (out, hits, counts) for the scene's points, computed once and left unchanged"""
    b, m, points = _scene(W, scene)
    refs = _cache[scene][3]
    if (depth, spp) not in refs:
        res = m.gatherDirectional(points, depth, spp, dru.SEED)
        for a in res:
            a.setflags(write=False)
        refs[depth, spp] = res
    return refs[depth, spp]


def _gather_and_check(r, points, depth, spp, ref, counts, tag, seed=dru.SEED):
    res, st = r.gatherDirectional(points, depth, spp, seed, stats=True)
    print(tag, "lds", st["lds"], "workgroups", st["workgroups"], {k: st[k] for k in dru.COUNT_NAMES})
    dru.check_against_model(res, ref, tag, nan_as_class=True)
    dru.check_counts(st, counts, points.shape[0], spp, tag)
    assert st["workgroups"] >= 1, tag
    plain = r.gatherDirectional(points, depth, spp, seed)
    assert np.array_equal(dru.result_words(plain), dru.result_words(res)), (tag, "counting and product kernel differ")
    st2 = r.directionalGatherStats()
    assert st2["extension_rays"] == st["extension_rays"] and st2["shadow_rays"] == st["shadow_rays"], tag
    assert st2["nodes_visited"] == 0 and st2["tris_tested"] == 0 and st2["shaded_hits"] == 0, tag
    return st


@pytest.mark.parametrize("scene,no_lds,lds", [("cornell", None, 1), ("cornell", "1", 0), ("special", None, 0)])
def test_bit_parity_with_the_model(W, monkeypatch, scene, no_lds, lds):
    b, m, points = _scene(W, scene)
    n = points.shape[0]
    assert n == 1024 and np.array_equal(points.view(np.uint32)[:, 7], 7 * np.arange(n, dtype=np.uint32) + 3)
    ref, hits, _ = _ref(W, scene, 4, 80)
    rows = ref.reshape(n, 4, 4)
    lit = int((np.abs(rows[:, :, :3]).max(axis=(1, 2)) > 0).sum())
    band1 = int((np.abs(rows[:, 1:, :3]).max(axis=(1, 2)) > 0).sum())
    print(scene, "model: points with a hit sample", int((hits > 0).sum()), "lit", lit, "with a band-1 word", band1, "of", n)
    assert 2 * lit >= n and 2 * band1 >= n, (scene, lit, band1)            # parity must not pass on darkness
    r = _renderer(W, monkeypatch, b, no_lds)
    try:
        for depth in DEPTHS:
            for spp in SPPS:
                ref, _, counts = _ref(W, scene, depth, spp)
                st = _gather_and_check(r, points, depth, spp, ref, counts, "%s no_lds=%s depth %d spp %d" % (scene, no_lds, depth, spp))
                assert st["lds"] == lds, (scene, no_lds, st)
                if depth == 0:
                    assert st["extension_rays"] == spp * n and st["shadow_rays"] == 0 and st["shaded_hits"] == 0
                    assert not ru.u32(ref.reshape(n, 4, 4)[:, :, :3]).any()                    # twelve words of +0
    finally:
        r.destroy()


def test_a_directional_gather_is_the_projection_of_the_gpus_radiance_queries(W, monkeypatch):
    """gatherDirectional equals, word for word, the numpy projection of the GPU's OWN radiance queries on the model's exported
    directions (spp = 1, seed = f per sample), and its counters are the sums of theirs."""
    b, m, points = _scene(W, "cornell")
    points = points[:256]
    r = _renderer(W, monkeypatch, b)
    try:
        for depth, spp in ((4, 17), (0, 3)):
            dirs = m.directions(points, spp, dru.SEED)

            def trace(rays, max_depth, one, seed):
                res, st = r.traceRadiance(rays, max_depth, one, seed, stats=True)
                return np.ascontiguousarray(res).view(np.float32).reshape(-1, 4), st

            want, want_hits, each = dru.compose(trace, points, dirs, depth, spp, dru.SEED)
            got, st = r.gatherDirectional(points, depth, spp, dru.SEED, stats=True)
            dru.check_against_model(got, want, "composed on the GPU, depth %d" % depth)
            for name in dru.COUNT_NAMES:
                assert st[name] == sum(e[name] for e in each), (depth, name)
            assert np.array_equal(ru.u32(got["layer"][:, 0, 3]), ru.u32(want_hits.astype(np.float32) / np.float32(spp)))
    finally:
        r.destroy()


def test_a_call_cut_into_two_batches(W, monkeypatch):
    """65 points at spp = 65536 are two batches, of 64 points and of 1: the result equals, word for word, the calls on the
    points [0, 64) and [64, 65) and the call on the reversed array; the stats are the sums over both radiance launches."""
    b, m, points = _scene(W, "cornell")
    pts = np.array(points[:65])
    spp = 65536
    r = _renderer(W, monkeypatch, b)
    try:
        r.setKernelTiming(True)
        full, st = r.gatherDirectional(pts, 1, spp, dru.SEED, stats=True)
        words = dru.result_words(full)
        head, st_a = r.gatherDirectional(pts[:64], 1, spp, dru.SEED, stats=True)
        tail, st_b = r.gatherDirectional(pts[64:], 1, spp, dru.SEED, stats=True)
        print("full", st, "head", st_a, "tail", st_b)
        assert np.array_equal(dru.result_words(head), words[:64]) and np.array_equal(dru.result_words(tail), words[64:])
        back = r.gatherDirectional(pts[::-1], 1, spp, dru.SEED)
        assert np.array_equal(dru.result_words(back)[::-1], words)
        assert st["rays"] == 65 and st["samples"] == 65 * spp and st_a["samples"] == 64 * spp and st_b["samples"] == spp
        for name in dru.COUNT_NAMES + ("workgroups",):
            assert st[name] == st_a[name] + st_b[name], (name, st[name], st_a[name], st_b[name])
        assert st["extension_rays"] >= 65 * spp and min(st["kernel_ms"], st_a["kernel_ms"], st_b["kernel_ms"]) > 0.0
        assert (full["layer"][:, 0, 3] > 0).any() and (full["layer"][:, 1:, :3] != 0).any()
        # with timing off no batch records its events: the same call reports the same stats and no time
        r.setKernelTiming(False)
        again, st_off = r.gatherDirectional(pts, 1, spp, dru.SEED, stats=True)
        assert np.array_equal(dru.result_words(again), words)
        assert st_off["kernel_ms"] == 0.0 and st_off == dict(st, kernel_ms=0.0)
    finally:
        r.destroy()


def test_device_entry_equals_the_host_entry(W, monkeypatch):
    import torch
    from webgpu_raytracer_amd import renderer as R
    b, m, points = _scene(W, "cornell")
    n = points.shape[0]
    ref, hits, counts = _ref(W, "cornell", 4, 17)
    r = _renderer(W, monkeypatch, b)
    try:
        host = r.gatherDirectional(points, 4, 17, dru.SEED)
        side = torch.cuda.Stream()
        r.setStream(side.cuda_stream)
        with torch.cuda.stream(side):
            d_points = torch.from_numpy(np.array(points)).cuda(non_blocking=False)
            d_out = torch.empty((n, 16), dtype=torch.float32, device="cuda")
            r.gatherDirectionalDevice(d_points.data_ptr(), n, d_out.data_ptr(), 4, 17, dru.SEED)
            n_hit = (d_out[:, 3] > 0).sum()            # a torch op on the same stream, behind the gather
        side.synchronize()
        got = d_out.cpu().numpy().view(R.DIRECTIONAL_DTYPE).reshape(-1)
        assert np.array_equal(dru.result_words(got), dru.result_words(host))
        dru.check_against_model(got, ref, "device entry")
        assert int(n_hit) == int((hits > 0).sum())
        st = r.directionalGatherStats()
        assert st["rays"] == n and st["samples"] == 17 * n and st["nodes_visited"] == 0   # counting is off on the device entry ...
        assert st["extension_rays"] == int(counts[:, 0].sum()) and st["shadow_rays"] == int(counts[:, 1].sum())
        r.setCounting(True)
        with torch.cuda.stream(side):
            r.gatherDirectionalDevice(d_points.data_ptr(), n, d_out.data_ptr(), 4, 17, dru.SEED)
        dru.check_counts(r.directionalGatherStats(), counts, n, 17, "device entry, counting")   # ... until asked for
        assert r.L.rt_gather_directional_device(r.ctx, d_points.data_ptr() + 8, 4, 4, 2, 0, d_out.data_ptr()) == RT_ERR_INVALID   # misaligned
        r.setStream(None)
    finally:
        r.destroy()


def _edge_points(points):
    """Eight ordinary points, untouched, followed by each of them with its normal replaced by a zero, a NaN, an infinite and a
    1e30 one, with t_max 0 and NaN, and with a NaN in each component of the position"""
    base = points[8:16]
    out = [p.copy() for p in base]
    normals = [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (np.nan, 0.0, 1.0), (np.nan, np.nan, np.nan), (np.inf, 0.0, 0.0),
               (-np.inf, np.inf, 1.0), (1e30, -1e30, 1e30), (0.0, -1e30, 0.0)]
    for p0 in base:
        for nrm in normals:
            p = p0.copy()
            p[4:7] = nrm
            out.append(p)
        for t_max in (0.0, np.nan):
            p = p0.copy()
            p[3] = t_max
            out.append(p)
        for comp in (0, 1, 2):
            p = p0.copy()
            p[comp] = np.nan
            out.append(p)
    return np.ascontiguousarray(np.stack(out), np.float32)


@pytest.mark.parametrize("no_lds", [None, "1"])
def test_edge_input(W, monkeypatch, no_lds):
    """Degenerate normals, t_max and positions: the call returns with the model's results (NaNs as a class only in rows where
    the model has one), the untouched points of the same call are bit-exact; n == 0 is RT_OK."""
    b, m, points = _scene(W, "cornell")
    pts = _edge_points(points)
    assert pts.shape[0] == 8 + 8 * 13
    r = _renderer(W, monkeypatch, b, no_lds)
    try:
        for depth, spp in ((4, 65), (1, 3)):
            ref, _, _ = m.gatherDirectional(pts, depth, spp, dru.SEED)
            res = r.gatherDirectional(pts, depth, spp, dru.SEED)
            tag = "edge no_lds=%s depth %d" % (no_lds, depth)
            dru.check_against_model(res, ref, tag, nan_as_class=True)
            assert not np.isnan(ref[:8]).any(), tag
            assert np.array_equal(dru.result_words(res)[:8], ru.u32(ref[:8])), tag
        none, st = r.gatherDirectional(pts[:0], 4, 8, dru.SEED, stats=True)
        assert none.shape == (0,) and st["rays"] == 0 and st["samples"] == 0 and st["workgroups"] == 0
        assert r.L.rt_gather_directional(r.ctx, None, 0, 4, 8, dru.SEED, None, None) == 0
        assert r.directionalGatherStats()["rays"] == 0
    finally:
        r.destroy()


def test_directional_gathers_leave_the_render_and_the_other_queries_alone(W, monkeypatch):
    """Frames 1-4, directional gathers, frames 5-8 with lookahead 8 against the same frames without: accumulation, presented
    image, counters, G-buffer and uniforms are equal.  The stats of the last radiance query, irradiance gather and probe
    gather read the same before and after a directional gather, and each of them run again gives the same words."""
    b, m, points = _scene(W, "cornell")
    W._build.build_rt()
    ref, _, counts = _ref(W, "cornell", 4, 17)

    def gathers(r):
        _gather_and_check(r, points, 4, 17, ref, counts, "between frames")

    got = _render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), gathers)
    want = _render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), lambda r: None)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "accumulation"
    assert np.array_equal(got[1], want[1]), "captureFrame"
    assert got[2] == want[2], (got[2], want[2])
    for a, w in zip(got[3], want[3]):
        assert np.array_equal(pu.bits(a), pu.bits(w)), "G-buffer"
    assert np.array_equal(got[4], want[4]), "uniforms"

    r = _renderer(W, monkeypatch, b)
    try:
        some = np.array(points[:40])
        probes = np.array(points[:24])
        probes[:, 4:7] = 0.0
        rays = np.array(points[:96])
        res_r, st_r = r.traceRadiance(rays, 4, 2, dru.SEED, stats=True)
        res_g, st_g = r.gatherIrradiance(some, 4, 2, dru.SEED, stats=True)
        res_p, st_p = r.gatherProbes(probes, 4, 5, dru.SEED, stats=True)
        _gather_and_check(r, points, 4, 17, ref, counts, "after the other queries")
        after_r, after_g, after_p = r.radianceQueryStats(), r.irradianceGatherStats(), r.probeGatherStats()
        after_d = r.directionalGatherStats()
        assert after_r == st_r and after_g == st_g and after_p == st_p, (st_r, after_r, st_g, after_g, st_p, after_p)
        assert after_d["rays"] == 1024 and after_d["samples"] == 1024 * 17
        assert len({st_r["extension_rays"], st_g["extension_rays"], st_p["extension_rays"], after_d["extension_rays"]}) == 4
        again = r.traceRadiance(rays, 4, 2, dru.SEED)
        assert np.array_equal(ru.result_words(again), ru.result_words(res_r))
        again_g = r.gatherIrradiance(some, 4, 2, dru.SEED)
        assert np.array_equal(gu.result_words(again_g), gu.result_words(res_g))
        again_p = r.gatherProbes(probes, 4, 5, dru.SEED)
        assert np.array_equal(prb.result_words(again_p), prb.result_words(res_p))
        # ... and the other way round: a probe gather, which shares the scratch of a batch, leaves the directional stats alone
        assert r.directionalGatherStats() == after_d
    finally:
        r.destroy()


def test_errors(W, monkeypatch):
    """The argument rules on a context without a scene (the body of tests/test_directional_abi.py, here with a device for
    certain), then with one: the light count, the largest spp, kernel timing."""
    from webgpu_raytracer_amd import renderer as R
    from test_directional_abi import test_argument_rules_on_a_context_without_a_scene as argument_rules
    assert R.load_library().rt_device_count() > 0
    argument_rules(W)
    b, m, points = _scene(W, "cornell")
    points = np.array(points[:96])
    r = _renderer(W, monkeypatch, b)
    try:
        out = np.zeros(points.shape[0], R.DIRECTIONAL_DTYPE)
        call = r.L.rt_gather_directional
        assert call(r.ctx, points.ctypes.data, 16, 4, 1, 0, out.ctypes.data, None) == 0
        assert call(r.ctx, points.ctypes.data, 1, 1, 65536, 0, out.ctypes.data, None) == 0      # spp = 65536 is accepted
        b.updateCamera(16, 16)
        r.updateSceneUniforms(b.cameraData, 0, len(np.asarray(b.lights)) // 2 + 1)              # a light count above the lights buffer
        assert call(r.ctx, points.ctypes.data, 16, 4, 1, 0, out.ctypes.data, None) == RT_ERR_INVALID
        assert b"light_count" in r.L.rt_last_error(r.ctx)
        r.updateSceneUniforms(b.cameraData, 0, b.lightCount)
        res, s = r.gatherDirectional(points, 4, 3, dru.SEED, stats=True)
        assert s["kernel_ms"] == 0.0
        r.setKernelTiming(True)
        res, s = r.gatherDirectional(points, 4, 3, dru.SEED, stats=True)
        assert s["kernel_ms"] > 0.0
    finally:
        r.destroy()
