"""Probe visibility maps on the GPU (rt_bake_volume_visibility: k_visibility_rays -> k_ray_query -> k_visibility_texels;
rt_sample_volume_visible: k_volume_sample_visible; rt_encode_volume_visibility: k_visibility_tiles) against the reference model
(tests/model/volume_visibility_model.cpp): the sampler bit for bit at the wave boundary and a ragged tail, over invalid, NaN and
infinite probes, NaN, infinite and zero-variance texels, points on a probe and outside, zero and NaN normals, with every option
of the descriptor; the identity against sampleVolume; a bake as the model's reduction of the GPU's own traceRays on the rule's
rays, in the LDS and the global-memory form, and cut into batches; the export; no side effect on a render or on the other
queries' state."""
import numpy as np
import pytest

import encode_util as eu
import parity_util as pu
import probe_util as prb
import radiance_util as ru
import volume_util as vu
import volume_visibility_util as vv
from test_gpu_irradiance_gather import _render, _renderer

pytestmark = pytest.mark.gpu

RT_ERR_INVALID = -1
GRIDS = ((1, 1, 1), (2, 1, 3), (3, 4, 5))
COUNTS = (1, 63, 64, 65, 1000)
SIZES = (4, 8)
_cache = {}


def _R():
    from webgpu_raytracer_amd import renderer
    return renderer


def _vis(size, backface, crush):
    return _R().volume_visibility_desc(size, 3.0, normal_bias=0.05, min_visibility=0.02, crush_threshold=0.3 if crush else 0.0,
                                       backface=backface)


def _sampler_inputs(dims, size):
    """(desc, volume, maps, {n: points}) of a grid and a map size, made once and left unchanged"""
    key = ("inputs", dims, size)
    if key not in _cache:
        g = GRIDS.index(dims)
        d = _R().volume_desc((-1.25, 0.5, 2.0), (0.75, 1.5, 0.3), dims, max_hit_fraction=0.5)
        vol = vu.random_volume(d, 300 + g)
        maps = vv.random_maps(d, _vis(size, False, False), 350 + 8 * g + size)
        pts = {n: vv.parity_points(d, n, 400 + 16 * g + COUNTS.index(n)) for n in COUNTS}
        for a in [vol, maps] + list(pts.values()):
            a.setflags(write=False)
        _cache[key] = (d, vol, maps, pts)
    return _cache[key]


def _sampler_ref(dims, size, backface, crush, n):
    key = ("ref", dims, size, backface, crush, n)
    if key not in _cache:
        d, vol, maps, pts = _sampler_inputs(dims, size)
        ref = vv.model_sample(d, _vis(size, backface, crush), vol, maps, pts[n])
        ref.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def test_the_sampler_cases_are_not_empty():
    """so the parity does not pass on nothing: per grid, at least a third of the points have W > 0 and a lit rgb in the model;
    the weights the model gives the corners take 0 .. 1 and values between; hostile texels and probes are among the inputs,
    and so are points on a probe, outside, at non-finite positions and with zero and non-finite normals."""
    for dims in GRIDS:
        d, vol, maps, pts = _sampler_inputs(dims, 8)
        ref = _sampler_ref(dims, 8, False, False, 1000)
        lit = int(((ref[:, 3] > 0) & (np.nan_to_num(ref[:, :3], nan=1.0).max(axis=1) > 0)).sum())
        print(dims, "lit", lit, "W == 0", int((ref[:, 3] == 0).sum()))
        assert 3 * lit >= 1000, (dims, lit)
        w = vv.model_weights(d, _vis(8, False, False), maps, pts[1000])
        finite = w[np.isfinite(w)]
        assert (finite == 1.0).any() and ((finite > 0.02) & (finite < 1.0)).any() and (finite == np.float32(0.02)).any()
        assert np.isnan(maps).any() and np.isinf(maps).any() and (maps[..., 1] == maps[..., 0] * maps[..., 0]).any()
        if dims != (1, 1, 1):
            assert not np.isfinite(vol[:, :27]).all() and (~(vol[:, 27] <= 0.5)).any()       # a hostile and an invalid probe
        if dims == (3, 4, 5):
            assert np.isnan(vol[:, 27]).any()
        p = pts[1000]
        nodes = vu.numpy_probes(d)[:, 0:3]
        assert (p[:, None, 0:3] == nodes[None, :, :]).all(axis=2).any(), "a point exactly on a probe"
        assert np.isnan(p[:, 0:3]).any() and np.isinf(p[:, 0:3]).any()
        assert (p[:, 4:7] == 0).all(axis=1).any() and np.isnan(p[:, 4:7]).any() and np.isinf(p[:, 4:7]).any()


@pytest.mark.parametrize("dims", GRIDS)
def test_sampler_bit_parity_with_the_model(W, dims):
    import torch
    r = W.WebGPURenderer(0)                                    # nothing uploaded: a sample needs no scene
    try:
        for size in SIZES:
            d, vol, maps, pts = _sampler_inputs(dims, size)
            d_vol, d_maps = torch.from_numpy(np.array(vol)).cuda(), torch.from_numpy(np.array(maps)).cuda()
            for backface in (False, True):
                for crush in (False, True):
                    v = _vis(size, backface, crush)
                    for n in COUNTS:
                        tag = "%s size %d backface %s crush %s n %d" % (dims, size, backface, crush, n)
                        ref = _sampler_ref(dims, size, backface, crush, n)
                        got = r.sampleVolumeVisible(d, v, vol, maps, pts[n])
                        vu.check_samples(got, ref, tag)
                        # the device entry on the same arrays, inside a larger allocation whose tail must stay untouched
                        d_pts = torch.from_numpy(np.array(pts[n])).cuda()
                        d_out = torch.full((n + 64, 4), -7.0, dtype=torch.float32, device="cuda")
                        torch.cuda.synchronize()
                        r.sampleVolumeVisibleDevice(d, v, d_vol.data_ptr(), d_maps.data_ptr(), d_pts.data_ptr(), n,
                                                    d_out.data_ptr())
                        r.sync()
                        out = d_out.cpu().numpy()
                        assert np.array_equal(vu.words(out[:n]), vu.words(got)), tag
                        assert (out[n:] == -7.0).all(), tag
        # a result does not depend on n or on the point's place in the array
        v = _vis(8, True, True)
        d, vol, maps, pts = _sampler_inputs(dims, 8)
        ref = _sampler_ref(dims, 8, True, True, 1000)
        back = r.sampleVolumeVisible(d, v, vol, maps, pts[1000][::-1])
        vu.check_samples(back[::-1], ref, "%s reversed" % (dims,))
        vu.check_samples(r.sampleVolumeVisible(d, v, vol, maps, pts[1000][437:438]), ref[437:438], "%s alone" % (dims,))
        assert r.sampleVolumeVisible(d, v, vol, maps, pts[1000][:0]).shape == (0,)
        assert r.L.rt_sample_volume_visible_device(r.ctx, d.ctypes.data, v.ctypes.data, d_vol.data_ptr(), d_maps.data_ptr() + 8,
                                                   d_pts.data_ptr(), 4, d_out.data_ptr()) == RT_ERR_INVALID     # misaligned
    finally:
        r.destroy()


@pytest.mark.parametrize("dims", GRIDS)
def test_identity_against_the_plain_sampler(W, dims):
    """(a) of tests/test_volume_visibility_model.py on the device: maps of {D, D * D} beyond every distance and flags = 0 give
    sampleVolume's words, whatever min_visibility and crush_threshold."""
    R = _R()
    g = GRIDS.index(dims)
    d = R.volume_desc((-1.25, 0.5, 2.0), (0.75, 1.5, 0.3), dims, max_hit_fraction=0.5)
    vol = vu.random_volume(d, 500 + g)
    pts = vu.parity_points(d, 1000, 600 + g)
    pts = pts[~np.isinf(pts[:, 0:3]).any(axis=1)]
    nodes = vu.numpy_probes(d)[:, 0:3].astype(np.float64)
    finite = pts[np.isfinite(pts[:, 0:3]).all(axis=1), 0:3].astype(np.float64)
    D = 2.0 * (np.sqrt(((finite[:, None, :] - nodes[None, :, :]) ** 2).sum(axis=2)).max() + 0.25) + 1.0
    r = W.WebGPURenderer(0)
    try:
        plain = r.sampleVolume(d, vol, pts)
        for size, min_vis, crush in ((4, 0.0, 0.0), (8, 0.3, 0.7), (32, 1.0, 1.0)):
            v = R.volume_visibility_desc(size, 4.0 * D, normal_bias=0.25, min_visibility=min_vis, crush_threshold=crush)
            got = r.sampleVolumeVisible(d, v, vol, vv.constant_maps(d, v, D), pts)
            assert np.array_equal(vu.words(got), vu.words(plain)), (dims, size)
        assert (plain["hit_fraction"] > 0).any()
    finally:
        r.destroy()


def _bake_case(W, scene, dims=(2, 1, 2), size=4, spt=3, pad_first=41):
    """(bridge, desc of a grid inside the scene's bounds, visibility desc with rays half the scene's diagonal long)"""
    b = pu.bridge_for(W, scene)
    lo, hi = prb.scene_bounds(b)
    n = np.array(dims)
    step = (hi - lo) / (n + 1.0)
    d = _R().volume_desc(lo + step, step, dims, pad_first=pad_first)
    v = _R().volume_visibility_desc(size, 0.5 * float(np.linalg.norm(hi - lo)), spt=spt)
    return b, d, v


@pytest.mark.parametrize("scene,no_lds,lds", [("cornell", None, 1), ("cornell", "1", 0), ("special", None, 0)])
def test_a_bake_is_the_reduction_of_the_gpus_own_ray_query(W, monkeypatch, scene, no_lds, lds):
    import torch
    b, d, v = _bake_case(W, scene)
    r = _renderer(W, monkeypatch, b, no_lds)
    try:
        for seed in (prb.SEED, 0):
            tag = "%s no_lds=%s seed %d" % (scene, no_lds, seed)
            rays = vv.model_rays(d, v, seed)
            assert rays.shape == (4 * 16 * 3, 8)
            hits, st_q = r.traceRays(rays, stats=True)
            want = vv.model_texels(v, hits)
            maps, st = r.bakeVolumeVisibility(d, v, seed, stats=True)
            assert maps.shape == (2, 1, 2, 4, 4, 2)
            assert np.array_equal(vu.words(maps), vu.words(want)), (tag, "bake against the reduced ray query")
            far = np.float32(v["max_distance"])
            assert (maps[..., 0] < far).any() and (maps[..., 0] <= far * np.float32(1.000001)).all() and (maps[..., 0] > 0).all(), tag
            assert (maps[..., 1] >= maps[..., 0] * maps[..., 0] * np.float32(0.999)).all(), tag      # a variance is not negative
            for name in ("rays", "nodes_visited", "tris_tested", "walk", "lds", "rayreg", "workgroups"):
                assert st[name] == st_q[name], (tag, name, st[name], st_q[name])
            assert st["rays"] == 192 and st["lds"] == lds and st["nodes_visited"] > 0, (tag, st)
            assert r.volumeVisibilityStats()["rays"] == 192
            assert r.rayQueryStats() == st_q, "the ray query's own stats are untouched"
            plain = r.bakeVolumeVisibility(d, v, seed)
            assert np.array_equal(vu.words(plain), vu.words(maps)), (tag, "counting and product kernel differ")
            # the device entry, into a torch tensor on a side stream
            side = torch.cuda.Stream()
            r.setStream(side.cuda_stream)
            with torch.cuda.stream(side):
                d_out = torch.full((64 + 2, 2), -7.0, dtype=torch.float32, device="cuda")
                r.bakeVolumeVisibilityDevice(d, v, d_out.data_ptr(), seed)
                total = d_out[:64, 0].sum()                # a torch op on the same stream, behind the bake
            side.synchronize()
            r.setStream(None)
            out = d_out.cpu().numpy()
            assert np.array_equal(vu.words(out[:64]), vu.words(maps)), (tag, "device entry")
            assert (out[64:] == -7.0).all() and float(total) > 0
        other = r.bakeVolumeVisibility(d, v, prb.SEED)
        assert not np.array_equal(vu.words(other), vu.words(maps)), "the seed moves the jitter"
    finally:
        r.destroy()


@pytest.mark.timeout(300)
def test_a_bake_cut_into_batches(W, monkeypatch):
    """A (1, 1, 2) grid at size 8 and spt 65536: 128 texels of 2^16 samples are two batches of RT_PROBE_BATCH_SAMPLES.  The call
    equals, word for word, two one-probe bakes with pad_first advanced by size * size; its stats are their sums."""
    R = _R()
    b, d, v = _bake_case(W, "cornell", dims=(1, 1, 2), size=8, spt=65536, pad_first=9)
    r = _renderer(W, monkeypatch, b)
    try:
        both, st = r.bakeVolumeVisibility(d, v, prb.SEED, stats=True)
        assert both.shape == (2, 1, 1, 8, 8, 2) and st["rays"] == 128 * 65536
        probes = vu.numpy_probes(d)
        each = []
        for p in (0, 1):
            one = R.volume_desc(probes[p, 0:3], d["step"], (1, 1, 1), pad_first=9 + 64 * p)
            assert np.array_equal(vu.numpy_probes(one)[0, 0:3], probes[p, 0:3])
            alone = r.bakeVolumeVisibility(one, v, prb.SEED)
            assert np.array_equal(vu.words(alone), vu.words(both[p])), p
            each.append(r.bakeVolumeVisibility(one, v, prb.SEED, stats=True)[1])
        # a batch is one probe here: the stats of the cut bake are the sums over the two ray launches, the form theirs
        print("both", st, "each", each)
        for name in ("rays", "nodes_visited", "tris_tested", "workgroups"):
            assert st[name] == each[0][name] + each[1][name], (name, st[name], each[0][name], each[1][name])
        for name in ("walk", "lds", "rayreg"):
            assert st[name] == each[0][name] == each[1][name], name
        assert st["nodes_visited"] > 0 and st["kernel_ms"] == 0.0 # timing is off: no batch recorded its events
        r.setKernelTiming(True)
        timed, st_t = r.bakeVolumeVisibility(d, v, prb.SEED, stats=True)
        r.setKernelTiming(False)
        assert np.array_equal(vu.words(timed), vu.words(both))
        assert st_t["kernel_ms"] > 0.0 and st_t == dict(st, kernel_ms=st_t["kernel_ms"])
        far = np.float32(v["max_distance"])
        # (the f32 sum of 65536 samples in sample order carries its rounding: a mean may lie a few 1e-4 above the clamp)
        assert (both[..., 0] < far * np.float32(1.001)).all() and (both[..., 1] > both[..., 0] * both[..., 0]).any()
    finally:
        r.destroy()


def test_export(W):
    R = _R()
    d = R.volume_desc((0, 0, 0), (1, 1, 1), (5, 3, 2))
    r = W.WebGPURenderer(0)
    try:
        for size in (4, 32):
            v = R.volume_visibility_desc(size, 1.0)
            n = 30 * size * size
            maps = np.ascontiguousarray(eu.special_atlas(n // 2, 1, 31).reshape(-1)[:2 * n].reshape(30, size, size, 2))
            assert np.isnan(maps).any() and np.isinf(maps).any()
            f32 = r.encodeVolumeVisibility(d, v, maps, "f32")
            assert f32.shape == (6 * (size + 2), 5 * (size + 2), 2) and f32.dtype == np.float32
            assert np.array_equal(vu.words(f32), vu.words(vv.model_tiles(d, v, maps, False))), size
            f16 = r.encodeVolumeVisibility(d, v, maps, "f16")
            assert f16.shape == f32.shape and f16.dtype == np.float16
            assert eu.same_f16(f16.view(np.uint16), vv.model_tiles(d, v, maps, True)), size
            with pytest.raises(W.RendererError, match="volume visibility: RT_LIGHTMAP_RGBE8"):
                r.encodeVolumeVisibility(d, v, maps, "rgbe")
    finally:
        r.destroy()


def test_visibility_leaves_the_render_and_the_other_queries_alone(W, monkeypatch):
    """Frames 1-4, a bake, a sample and an export, frames 5-8 with lookahead 8 against the same frames without: accumulation,
    presented image, counters, G-buffer and uniforms are equal.  The stats of the last ray query, radiance query, irradiance
    gather, probe gather, directional gather and reflection capture read the same before and after, and a ray query run again
    gives the same words."""
    R = _R()
    b, d, v = _bake_case(W, "cornell")
    W._build.build_rt()
    pts = vu.parity_points(d, 100, 77)
    vol = vu.random_volume(d, 9, invalid=False)
    rays = vv.model_rays(d, v, prb.SEED)

    def visibility_work(r):
        maps = r.bakeVolumeVisibility(d, v, prb.SEED)
        assert np.array_equal(vu.words(maps), vu.words(vv.model_texels(v, r.traceRays(rays)))), "between frames"
        vu.check_samples(r.sampleVolumeVisible(d, v, vol, maps, pts), vv.model_sample(d, v, vol, maps, pts), "between frames")
        assert eu.same_f16(r.encodeVolumeVisibility(d, v, maps, "f16").view(np.uint16), vv.model_tiles(d, v, maps, True))

    got = _render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), visibility_work)
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
        prays = np.array(probes)
        prays[:, 4] = 1.0
        res_q, st_q = r.traceRays(prays, stats=True)
        res_r, st_r = r.traceRadiance(prays, 4, 2, prb.SEED, stats=True)
        res_g, st_g = r.gatherIrradiance(points, 4, 2, prb.SEED, stats=True)
        res_p, st_p = r.gatherProbes(probes, 4, 5, prb.SEED, stats=True)
        res_d, st_d = r.gatherDirectional(points, 4, 3, prb.SEED, stats=True)
        rd = R.reflection_desc(8, 2, spt=2, filter_samples=64)
        res_f, st_f = r.captureReflection(rd, probes, 2, prb.SEED, stats=True)
        maps = r.bakeVolumeVisibility(d, v, prb.SEED)
        r.sampleVolumeVisible(d, v, vol, maps, pts)
        r.encodeVolumeVisibility(d, v, maps, "f32")
        assert r.rayQueryStats() == st_q and r.radianceQueryStats() == st_r and r.irradianceGatherStats() == st_g
        assert r.probeGatherStats() == st_p and r.directionalGatherStats() == st_d and r.reflectionStats() == st_f
        assert r.volumeVisibilityStats()["rays"] == 192
        assert np.array_equal(vu.words(r.traceRays(prays)), vu.words(res_q))
        assert np.array_equal(ru.result_words(r.traceRadiance(prays, 4, 2, prb.SEED)), ru.result_words(res_r))
    finally:
        r.destroy()
