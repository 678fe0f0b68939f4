"""Irradiance volumes on the GPU (rt_bake_volume: k_volume_probes -> the probe gather's device path -> k_volume_finish;
rt_sample_volume: k_volume_sample; rt_encode_volume: k_volume_layers) against the reference model (tests/model/volume_model.cpp
and, for the path work, tests/model/probe_model.cpp): the sampler bit for bit at the wave boundary and a ragged tail, over
invalid, NaN and infinite probes and points outside, on the last node and at non-finite positions; a bake as the numpy finish of
the GPU's own probe gather on numpy-made grid probes, in the LDS and the global-memory form, and cut into batches; the layer
export; the whole route against irradiance gathers; no side effect on a render or on the other queries' state."""
import numpy as np
import pytest

import encode_util as eu
import gather_util as gu
import parity_util as pu
import probe_util as prb
import radiance_util as ru
import volume_util as vu
from test_gpu_irradiance_gather import _render, _renderer

pytestmark = pytest.mark.gpu

RT_ERR_INVALID = -1
GRIDS = ((1, 1, 1), (2, 1, 3), (3, 4, 5), (5, 2, 2))
COUNTS = (1, 63, 64, 65, 1000)
_cache = {}


def _R():
    from webgpu_raytracer_amd import renderer
    return renderer


def _sampler_case(dims, n):
    """(desc, volume, points, the model's results), made once and left unchanged"""
    key = ("sampler", dims, n)
    if key not in _cache:
        g = GRIDS.index(dims)
        d = _R().volume_desc((-1.25, 0.5, 2.0), (0.75, 1.5, 0.3), dims, max_hit_fraction=0.5)
        v = vu.random_volume(d, 300 + g)
        pts = vu.parity_points(d, n, 400 + 16 * g + COUNTS.index(n))
        ref = vu.model_sample(d, v, pts)
        for a in (v, pts, ref):
            a.setflags(write=False)
        _cache[key] = (d, v, pts, ref)
    return _cache[key]


def test_the_sampler_cases_are_not_empty():
    """so the parity does not pass on nothing: over each grid's cases at least half of the points have W > 0 and a non-zero
    rgb in the model; except on the one-probe grid, whose single probe is valid, some point has W == 0; NaNs and infinities
    are among the coefficients, and the special points are there."""
    for dims in GRIDS:
        W_all, rgb_all = [], []
        for n in COUNTS:
            d, v, pts, ref = _sampler_case(dims, n)
            W_all.append(ref[:, 3])
            rgb_all.append(np.nan_to_num(ref[:, :3], nan=1.0).max(axis=1))
        Wc, rgb = np.concatenate(W_all), np.concatenate(rgb_all)
        lit = int(((Wc > 0) & (rgb > 0)).sum())
        print(dims, "points", Wc.size, "W > 0 and lit", lit, "W == 0", int((Wc == 0).sum()))
        assert 2 * lit >= Wc.size, (dims, lit)
        if dims != (1, 1, 1):
            assert (Wc == 0).any(), dims
            assert not np.isfinite(v[:, :27]).all()
        d, v, pts, ref = _sampler_case(dims, 1000)
        assert np.isnan(pts[:, 0:3]).any() and np.isinf(pts[:, 0:3]).any() and (pts[:, 4:7] == 0).all(axis=1).any()
        assert ((ref[:, 3] > 0) & (ref[:, 3] < 1)).any() or dims == (1, 1, 1)      # partly valid cells


@pytest.mark.parametrize("dims", GRIDS)
def test_sampler_bit_parity_with_the_model(W, dims):
    import torch
    r = W.WebGPURenderer(0)                                    # nothing uploaded: a sample needs no scene
    try:
        for n in COUNTS:
            d, v, pts, ref = _sampler_case(dims, n)
            got = r.sampleVolume(d, v, pts)
            vu.check_samples(got, ref, "%s n %d" % (dims, n))
            # the device entry on the same arrays, inside a larger allocation whose tail must stay untouched
            d_vol, d_pts = torch.from_numpy(np.array(v)).cuda(), torch.from_numpy(np.array(pts)).cuda()
            d_out = torch.full((n + 64, 4), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            r.sampleVolumeDevice(d, d_vol.data_ptr(), d_pts.data_ptr(), n, d_out.data_ptr())
            r.sync()
            out = d_out.cpu().numpy()
            assert np.array_equal(vu.words(out[:n]), vu.words(got)), (dims, n)
            assert (out[n:] == -7.0).all(), (dims, n)
        # a result does not depend on n or on the point's place in the array
        d, v, pts, ref = _sampler_case(dims, 1000)
        back = r.sampleVolume(d, v, pts[::-1])
        vu.check_samples(back[::-1], ref, "%s reversed" % (dims,))
        vu.check_samples(r.sampleVolume(d, v, pts[437:438]), ref[437:438], "%s alone" % (dims,))
        assert r.sampleVolume(d, v, pts[:0]).shape == (0,)
        assert r.L.rt_sample_volume_device(r.ctx, d.ctypes.data, d_vol.data_ptr() + 8, d_pts.data_ptr(), 4,
                                           d_out.data_ptr()) == RT_ERR_INVALID           # misaligned
    finally:
        r.destroy()


def _bake_scene(W, scene):
    """(bridge, probe model, desc of a 3 x 2 x 4 grid inside the bounds) of a scene, made once"""
    key = ("scene", scene)
    if key not in _cache:
        b = pu.bridge_for(W, scene)
        m = prb.model_for(W, b)
        lo, hi = prb.scene_bounds(b)
        dims = np.array([3, 2, 4])
        step = (hi - lo) / (dims + 1.0)
        _cache[key] = (b, m, lo, step)
    return _cache[key]


def _bake_desc(W, scene, window=(1.0, 1.0, 1.0), dims=(3, 2, 4)):
    b, m, lo, step = _bake_scene(W, scene)
    return _R().volume_desc(lo + step, step, dims, window=window, pad_first=41, t_max=1e30)


def _model_volume(W, scene, desc, depth, spp):
    key = ("volume", scene, desc.tobytes(), depth, spp)
    if key not in _cache:
        m = _bake_scene(W, scene)[1]
        sh9, hits, counts = m.gatherProbes(vu.model_probes(desc), depth, spp, prb.SEED)
        vol = vu.model_finish(desc, sh9)
        vol.setflags(write=False)
        _cache[key] = (vol, sh9, counts)
    return _cache[key]


@pytest.mark.parametrize("scene,no_lds,lds", [("cornell", None, 1), ("cornell", "1", 0), ("special", None, 0)])
def test_a_bake_is_the_finish_of_the_gpus_probe_gather(W, monkeypatch, scene, no_lds, lds):
    import torch
    b = _bake_scene(W, scene)[0]
    r = _renderer(W, monkeypatch, b, no_lds)
    try:
        for depth, spp, window in ((4, 65, (1.0, 0.5, 0.0)), (4, 3, (1.0, 1.0, 1.0)), (0, 65, tuple(_R().sh_hanning_window(3))),
                                  (0, 3, (1.0, 1.0, 1.0))):
            tag = "%s no_lds=%s depth %d spp %d" % (scene, no_lds, depth, spp)
            d = _bake_desc(W, scene, window)
            probes = vu.numpy_probes(d)
            sh9, st_g = r.gatherProbes(probes, depth, spp, prb.SEED, stats=True)
            want = vu.numpy_finish(d, prb.result_words(sh9).view(np.float32))
            vol, st = r.bakeVolume(d, depth, spp, prb.SEED, stats=True)
            assert vol.shape == (4, 2, 3)
            assert np.array_equal(vu.words(vol), vu.words(want)), (tag, "bake against the finished gather")
            model_vol, model_sh9, counts = _model_volume(W, scene, d, depth, spp)
            if depth == 4:
                lit = int((np.abs(model_sh9[:, :27]).max(axis=1) > 0).sum())
                assert 2 * lit >= len(probes), (tag, lit)
            prb.check_against_model(vol.reshape(-1), model_vol, tag, nan_as_class=True)
            for name in ("rays", "samples", "lds", "workgroups") + prb.COUNT_NAMES:
                assert st[name] == st_g[name], (tag, name, st[name], st_g[name])
            assert st["lds"] == lds and st["rays"] == 24 and st["samples"] == 24 * spp, (tag, st)
            prb.check_counts(st, counts, 24, spp, tag)
            assert r.probeGatherStats()["samples"] == 24 * spp                     # the state is the probe gather's
            plain = r.bakeVolume(d, depth, spp, prb.SEED)
            assert np.array_equal(vu.words(plain), vu.words(vol)), (tag, "counting and product kernel differ")
            # the device entry, into a torch tensor on a side stream
            side = torch.cuda.Stream()
            r.setStream(side.cuda_stream)
            with torch.cuda.stream(side):
                d_out = torch.full((24 + 2, 28), -7.0, dtype=torch.float32, device="cuda")
                r.bakeVolumeDevice(d, d_out.data_ptr(), depth, spp, prb.SEED)
                n_hit = (d_out[:24, 27] > 0).sum()         # a torch op on the same stream, behind the bake
            side.synchronize()
            r.setStream(None)
            out = d_out.cpu().numpy()
            assert np.array_equal(vu.words(out[:24]), vu.words(vol)), (tag, "device entry")
            assert (out[24:] == -7.0).all() and int(n_hit) == int((out[:24, 27] > 0).sum())
        if scene == "cornell":
            assert (vol["hit_fraction"] > 0).all()
    finally:
        r.destroy()


@pytest.mark.timeout(300)
def test_a_bake_cut_into_batches(W, monkeypatch):
    """A 5 x 1 x 1 grid and a 65 x 1 x 1 grid at spp = 65536, depth 1: the second is two batches of the probe gather, 64 probes
    and 1.  Both equal the gatherProbes results on the numpy-made probes, finished in numpy; the grids share their first five
    probes, whose records are therefore the same in both."""
    b, m, lo, step = _bake_scene(W, "cornell")
    spp = 65536
    r = _renderer(W, monkeypatch, b)
    try:
        lo64, hi64 = prb.scene_bounds(b)
        vols = {}
        for nx in (5, 65):
            origin = lo64 + 0.25 * (hi64 - lo64)
            step_x = np.array([0.5 * (hi64[0] - lo64[0]) / 64.0, 1.0, 1.0])
            d = _R().volume_desc(origin, step_x, (nx, 1, 1), window=(1.0, 0.5, 0.25), pad_first=9)
            probes = vu.numpy_probes(d)
            sh9, st_g = r.gatherProbes(probes, 1, spp, prb.SEED, stats=True)
            vol, st = r.bakeVolume(d, 1, spp, prb.SEED, stats=True)
            assert np.array_equal(vu.words(vol), vu.words(vu.numpy_finish(d, prb.result_words(sh9).view(np.float32)))), nx
            for name in ("rays", "samples", "workgroups") + prb.COUNT_NAMES:
                assert st[name] == st_g[name], (nx, name)
            assert st["samples"] == nx * spp and (vol["hit_fraction"] > 0).all()
            assert st["kernel_ms"] == 0.0                        # timing is off: no batch recorded its events
            if nx == 65:
                # the stats of the cut bake are the sums over its two batches, its time that of both radiance launches
                st_a = r.gatherProbes(probes[:64], 1, spp, prb.SEED, stats=True)[1]
                st_b = r.gatherProbes(probes[64:], 1, spp, prb.SEED, stats=True)[1]
                for name in ("rays", "samples", "workgroups") + prb.COUNT_NAMES:
                    assert st[name] == st_a[name] + st_b[name], (name, st[name], st_a[name], st_b[name])
                r.setKernelTiming(True)
                st_t = r.bakeVolume(d, 1, spp, prb.SEED, stats=True)[1]
                r.setKernelTiming(False)
                assert st_t["kernel_ms"] > 0.0 and st_t == dict(st, kernel_ms=st_t["kernel_ms"])
            vols[nx] = vu.words(vol).reshape(-1, 28)
        assert np.array_equal(vols[65][:5], vols[5])
    finally:
        r.destroy()


def test_export(W):
    R = _R()
    d = R.volume_desc((0, 0, 0), (1, 1, 1), (5, 3, 7))
    n = 105
    v = np.ascontiguousarray(eu.special_atlas(7 * n, 1, 31).reshape(n, 28))     # every special of the encode tests, as coefficients
    assert np.isnan(v).any() and np.isinf(v).any()
    r = W.WebGPURenderer(0)
    try:
        f32 = r.encodeVolume(d, v, "f32")
        assert f32.shape == (7, 7, 3, 5, 4) and f32.dtype == np.float32
        assert np.array_equal(vu.words(f32), vu.words(v.reshape(n, 7, 4).transpose(1, 0, 2)))
        assert np.array_equal(vu.words(f32), vu.words(vu.model_layers(d, v, False)))
        f16 = r.encodeVolume(d, v, "f16")
        assert f16.shape == (7, 7, 3, 5, 4) and f16.dtype == np.float16
        assert eu.same_f16(f16.view(np.uint16), vu.model_layers(d, v, True))
        assert eu.same_f16(f16.view(np.uint16), eu.host_f16(f32))
        with pytest.raises(W.RendererError, match="volume: RT_LIGHTMAP_RGBE8"):
            r.encodeVolume(d, v, "rgbe")
        # a volume as a PROBE_SH9_DTYPE array goes in the same way
        rec = v.view(R.PROBE_SH9_DTYPE).reshape(7, 3, 5)
        assert np.array_equal(vu.words(r.encodeVolume(d, rec, "f32")), vu.words(f32))
    finally:
        r.destroy()


def test_end_to_end_against_irradiance_gathers(W, monkeypatch):
    """Statistical.  In cornell a 4^3 volume baked at spp 4096 and depth 4 without a window, sampled at 16 grid nodes with the
    six axis normals, against pi * gatherIrradiance at the same position, normal and spp.  The two are different estimators of
    the same integral only as far as bands 0 .. 2 capture it, so the bound comes from the reference route - the same comparison
    made from sh9_irradiance(gatherProbes(...)) in numpy: the device sampler must agree with that route to the float tolerance
    of tests/test_volume_model.py, and is then exactly as close to the gathers as the numpy route is."""
    R = _R()
    b = _bake_scene(W, "cornell")[0]
    lo, hi = prb.scene_bounds(b)
    step = (hi - lo) / 5.0
    d = R.volume_desc(lo + step, step, (4, 4, 4), pad_first=100)
    spp = 4096
    r = _renderer(W, monkeypatch, b)
    try:
        probes = vu.numpy_probes(d)
        vol = r.bakeVolume(d, 4, spp, prb.SEED)
        nodes = np.random.default_rng(5).permutation(64)[:16]
        normals = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
        pts = vu.make_points(np.repeat(probes[nodes, 0:3], 6, axis=0), np.tile(normals, (16, 1)))
        got = r.sampleVolume(d, vol, pts)
        assert np.array_equal(got["hit_fraction"], np.ones(96, np.float32))
        sh9 = r.gatherProbes(probes, 4, spp, prb.SEED)
        route = np.maximum(R.sh9_irradiance(sh9["sh"][nodes], normals), 0.0).reshape(96, 3)        # the existing host route
        err = np.abs(got["rgb"].astype(np.float64) - route) / np.maximum(1.0, np.abs(route))
        print("sampler against the numpy route: largest relative difference", err.max())
        assert err.max() <= vu.FLOAT_TOLERANCE, err.max()
        gather_pts = pts.copy()
        gather_pts[:, 3] = 1e30
        gather_pts.view(np.uint32)[:, 7] = 7 * np.arange(96, dtype=np.uint32) + 3
        E = np.pi * r.gatherIrradiance(gather_pts, 4, spp, prb.SEED)["rgb"].astype(np.float64)
        scale = E.mean()
        dev, ref = np.abs(got["rgb"] - E).mean() / scale, np.abs(route - E).mean() / scale
        print("mean |sampled - pi gather| / mean E", dev, "the numpy route's", ref, "mean E", scale)
        # mean | |a - E| - |b - E| | <= mean |a - b|: the two routes are equally far from the gathers, to the float tolerance
        assert scale > 0 and abs(dev - ref) * scale <= vu.FLOAT_TOLERANCE * max(1.0, np.abs(route).max())
    finally:
        r.destroy()


def test_volumes_leave_the_render_and_the_other_queries_alone(W, monkeypatch):
    """Frames 1-4, a bake, a sample and an encode, frames 5-8 with lookahead 8 against the same frames without: accumulation,
    presented image, counters, G-buffer and uniforms are equal.  The stats of the last radiance query, irradiance gather and
    directional gather read the same before and after, and a radiance query run again gives the same words."""
    b = _bake_scene(W, "cornell")[0]
    W._build.build_rt()
    d = _bake_desc(W, "cornell", (1.0, 0.5, 0.0))
    model_vol = _model_volume(W, "cornell", d, 4, 65)[0]
    pts = vu.parity_points(d, 100, 77)

    def volume_work(r):
        vol = r.bakeVolume(d, 4, 65, prb.SEED)
        prb.check_against_model(vol.reshape(-1), model_vol, "between frames")
        vu.check_samples(r.sampleVolume(d, vol, pts), vu.model_sample(d, model_vol, pts), "between frames")
        assert eu.same_f16(r.encodeVolume(d, vol, "f16").view(np.uint16), vu.model_layers(d, model_vol, True))

    got = _render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), volume_work)
    want = _render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), lambda r: None)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "accumulation"
    assert np.array_equal(got[1], want[1]), "captureFrame"
    assert got[2] == want[2], (got[2], want[2])
    for a, w in zip(got[3], want[3]):
        assert np.array_equal(pu.bits(a), pu.bits(w)), "G-buffer"
    assert np.array_equal(got[4], want[4]), "uniforms"

    r = _renderer(W, monkeypatch, b)
    try:
        probes = vu.numpy_probes(d)
        points = np.array(probes)
        points[:, 5] = 1.0                                        # gather points: the probes with a normal
        rays = np.array(probes)
        rays[:, 4] = 1.0
        res_r, st_r = r.traceRadiance(rays, 4, 2, prb.SEED, stats=True)
        res_g, st_g = r.gatherIrradiance(points, 4, 2, prb.SEED, stats=True)
        res_d, st_d = r.gatherDirectional(points, 4, 3, prb.SEED, stats=True)
        volume_work(r)
        assert r.radianceQueryStats() == st_r and r.irradianceGatherStats() == st_g and r.directionalGatherStats() == st_d
        after_p = r.probeGatherStats()
        assert after_p["rays"] == 24 and after_p["samples"] == 24 * 65
        assert np.array_equal(ru.result_words(r.traceRadiance(rays, 4, 2, prb.SEED)), ru.result_words(res_r))
        assert np.array_equal(gu.result_words(r.gatherIrradiance(points, 4, 2, prb.SEED)), gu.result_words(res_g))
    finally:
        r.destroy()
