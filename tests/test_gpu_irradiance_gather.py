"""Irradiance gathers on the GPU (rt_gather_irradiance, k_irradiance_gather) against the reference model (tests/model/
gather_model.cpp, tied to the radiance model by tests/test_gather_model.py), point by point: rgb and hit_fraction bit for bit,
the ray, hit, node and triangle counters as sums, in the LDS and the global-memory form; textures and transforms; the
composition identity on the GPU's own radiance queries; independence of the point's place in the array; t_max, max_depth = 0;
degenerate points; no side effect on a render; the device entry on a torch side stream; the device-resident animated world;
the error returns; a radiance query and a gather on one context, each with its own state and last stats."""
import ctypes

import numpy as np
import pytest

import gather_util as gu
import parity_util as pu
import radiance_util as ru
import random_scene
import ray_query_util as rq
from test_bvh_independent import _random_rays

pytestmark = pytest.mark.gpu

RT_ERR_INVALID, RT_ERR_NOT_READY = -1, -3
SETTINGS = ((4, 8), (1, 3), (8, 1), (0, 4))      # (max_depth, spp)
_cache = {}


def _scene(W, scene):
    """(bridge, model, points) of a scene, made once: 1 024 points, pads 7 i + 3"""
    if scene not in _cache:
        b = pu.bridge_for(W, scene)
        m = gu.model_for(W, b)
        points = gu.scene_points(m, b)
        points.setflags(write=False)
        _cache[scene] = (b, m, points, {})
    return _cache[scene][:3]


def _ref(W, scene, depth, spp):
    """the model's (out, hits, counts) for the scene's points, computed once and left unchanged"""
    b, m, points = _scene(W, scene)
    refs = _cache[scene][3]
    if (depth, spp) not in refs:
        res = m.gatherIrradiance(points, depth, spp, gu.SEED)
        for a in res:
            a.setflags(write=False)
        refs[depth, spp] = res
    return refs[depth, spp]


def _renderer(W, monkeypatch, bridge, no_lds=None):
    """a context created AFTER the env knob is set, with the scene uploaded as a render would (light count included)"""
    if no_lds is None:
        monkeypatch.delenv("MI355RT_NO_LDS_STAGING", raising=False)
    else:
        monkeypatch.setenv("MI355RT_NO_LDS_STAGING", no_lds)
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    W.upload_scene(r, bridge, 16, 16)
    return r


def _gather_and_check(r, points, depth, spp, ref, counts, tag, seed=gu.SEED):
    res, st = r.gatherIrradiance(points, depth, spp, seed, stats=True)
    print(tag, "lds", st["lds"], "workgroups", st["workgroups"], {k: st[k] for k in gu.COUNT_NAMES})
    gu.check_against_model(res, ref, tag)
    gu.check_counts(st, counts, points.shape[0], spp, tag)
    assert 1 <= st["workgroups"] <= (points.shape[0] + 255) // 256, tag
    plain = r.gatherIrradiance(points, depth, spp, seed)
    assert np.array_equal(gu.result_words(plain), gu.result_words(res)), (tag, "counting and product kernel differ")
    st2 = r.irradianceGatherStats()
    assert st2["extension_rays"] == st["extension_rays"] and st2["shadow_rays"] == st["shadow_rays"], tag
    assert st2["nodes_visited"] == 0 and st2["tris_tested"] == 0 and st2["shaded_hits"] == 0, tag
    return st


@pytest.mark.parametrize("scene,no_lds,lds", [("cornell", None, 1), ("cornell", "1", 0), ("special", None, 0),
                                              ("instanced1000", None, 0), ("glass_blob", None, 0)])
def test_bit_parity_with_the_model(W, monkeypatch, scene, no_lds, lds):
    b, m, points = _scene(W, scene)
    n = points.shape[0]
    assert n == 1024
    ref, hits, _ = _ref(W, scene, 4, 8)
    some_hit, lit = int((ref[:, 3] > 0).sum()), int((ref[:, :3].max(axis=1) > 0).sum())
    print(scene, "model: points with a hit sample", some_hit, "lit", lit, "of", n)
    assert 4 * some_hit >= 3 * n and 5 * lit >= 2 * n, (scene, some_hit, lit)      # parity must not pass on darkness
    r = _renderer(W, monkeypatch, b, no_lds)
    try:
        for depth, spp in SETTINGS:
            ref, _, counts = _ref(W, scene, depth, spp)
            st = _gather_and_check(r, points, depth, spp, ref, counts, "%s no_lds=%s depth %d spp %d" % (scene, no_lds, depth, spp))
            assert st["lds"] == lds, (scene, no_lds, st)
    finally:
        r.destroy()


@pytest.mark.parametrize("seed", [1, 2])
def test_textures_and_transforms(W, monkeypatch, seed):
    b = random_scene.make(seed, with_textures=True)
    m = gu.model_for(W, b)
    points = gu.points_from_rays(m, ru.with_pads(rq.to_rt_rays(_random_rays(b, 1024, 40 + seed))))
    r = _renderer(W, monkeypatch, b)
    try:
        ref, hits, counts = m.gatherIrradiance(points, 6, 2, gu.SEED)
        print("random scene", seed, "points with a hit sample", int((hits > 0).sum()), "lit", int((ref[:, :3].max(axis=1) > 0).sum()))
        assert (hits > 0).sum() >= 32 and (ref[:, :3].max(axis=1) > 0).sum() >= 8, seed   # sparse scenes: objects in open space
        _gather_and_check(r, points, 6, 2, ref, counts, "random scene %d depth 6 spp 2" % seed)
    finally:
        r.destroy()


@pytest.mark.parametrize("scene", ["cornell", "instanced1000"])
def test_a_gather_is_the_composition_of_radiance_queries(W, monkeypatch, scene):
    """gatherIrradiance equals the in-order float32 sum and division of the GPU's OWN radiance queries on the model's exported
    directions, and its ray counters are the sums of theirs."""
    b, m, points = _scene(W, scene)
    r = _renderer(W, monkeypatch, b)
    try:
        for depth, spp in ((4, 8), (0, 4)):
            dirs = m.gatherDirections(points, spp, gu.SEED)

            def trace(rays, max_depth, one, seed):
                res, st = r.traceRadiance(rays, max_depth, one, seed, stats=True)
                return np.ascontiguousarray(res).view(np.float32).reshape(-1, 4), st

            want, want_hits, each = gu.compose(trace, points, dirs, depth, spp, gu.SEED)
            got, st = r.gatherIrradiance(points, depth, spp, gu.SEED, stats=True)
            gu.check_against_model(got, want, "%s composed on the GPU, depth %d" % (scene, depth))
            for name in ("extension_rays", "shadow_rays", "shaded_hits", "nodes_visited", "tris_tested"):
                assert st[name] == sum(e[name] for e in each), (scene, depth, name)
            assert np.array_equal(ru.u32(got["hit_fraction"]), ru.u32(want_hits.astype(np.float32) / np.float32(spp)))
    finally:
        r.destroy()


@pytest.mark.parametrize("no_lds", [None, "1"])
def test_results_do_not_depend_on_scheduling(W, monkeypatch, no_lds):
    b, m, points = _scene(W, "cornell")
    n = points.shape[0]
    ref, _, _ = _ref(W, "cornell", 4, 8)
    r = _renderer(W, monkeypatch, b, no_lds)
    try:
        full = r.gatherIrradiance(points, 4, 8, gu.SEED)
        gu.check_against_model(full, ref, "full")
        words = gu.result_words(full)
        # chunk and workgroup edges: the first k points alone give a prefix of the full result
        for k in (1, 63, 64, 65, 257):
            part, st = r.gatherIrradiance(points[:k], 4, 8, gu.SEED, stats=True)
            assert np.array_equal(gu.result_words(part), words[:k]), k
            assert st["rays"] == k and st["samples"] == 8 * k
        # reversed, shuffled, and as the two halves of one call
        assert np.array_equal(gu.result_words(r.gatherIrradiance(points[::-1], 4, 8, gu.SEED)), words[::-1])
        perm = np.random.default_rng(9).permutation(n)
        assert np.array_equal(gu.result_words(r.gatherIrradiance(points[perm], 4, 8, gu.SEED)), words[perm])
        assert np.array_equal(gu.result_words(r.gatherIrradiance(points[: n // 2], 4, 8, gu.SEED)), words[: n // 2])
        assert np.array_equal(gu.result_words(r.gatherIrradiance(points[n // 2:], 4, 8, gu.SEED)), words[n // 2:])
        # n == 0
        none, st = r.gatherIrradiance(points[:0], 4, 8, gu.SEED, stats=True)
        assert none.shape == (0,) and st["rays"] == 0 and st["workgroups"] == 0
        assert r.L.rt_gather_irradiance(r.ctx, None, 0, 4, 8, gu.SEED, None, None) == 0
        # two copies of a point with the same pad agree, wherever they stand
        twice = np.concatenate([points[:300], points[100:101], points[300:700], points[100:101]])
        res = gu.result_words(r.gatherIrradiance(twice, 4, 8, gu.SEED))
        assert np.array_equal(res[300], res[100]) and np.array_equal(res[701], res[100])
    finally:
        r.destroy()


@pytest.mark.parametrize("no_lds,lds", [(None, 1), ("1", 0)])
def test_the_two_kinds_of_path_query_keep_their_own_state(W, monkeypatch, no_lds, lds):
    """One context, 130 items (two full chunks of 64 and a partial one), max_depth 4, spp 2: a radiance query and a gather
    through the one host launch path, both counting.  Each equals its model; the radiance query's stats read AFTER the gather
    are still the radiance query's and the gather's are the gather's (the kinds share neither a QueryState nor a last-stats
    record); the radiance query run again, without counting, gives the same words."""
    b, m, points = _scene(W, "cornell")
    pts = points[:130]
    rays = gu.sample_rays(pts, m.gatherDirections(pts, 1, gu.SEED), 0)      # a ray per point: its first gather direction
    ref_r, counts_r = m.traceRadiance(rays, 4, 2, gu.SEED)
    ref_g, _, counts_g = m.gatherIrradiance(pts, 4, 2, gu.SEED)
    sums_r, sums_g = counts_r.sum(axis=0).tolist(), counts_g.sum(axis=0).tolist()
    print("model counts", dict(zip(gu.COUNT_NAMES, sums_r)), dict(zip(gu.COUNT_NAMES, sums_g)))
    assert all(a != c for a, c in zip(sums_r, sums_g)), "the two queries must not count alike: mixed-up stats would pass"
    r = _renderer(W, monkeypatch, b, no_lds)
    try:
        res_r, st_r = r.traceRadiance(rays, 4, 2, gu.SEED, stats=True)
        res_g, st_g = r.gatherIrradiance(pts, 4, 2, gu.SEED, stats=True)
        after_r, after_g = r.radianceQueryStats(), r.irradianceGatherStats()
        print("radiance", st_r, after_r)
        print("gather", st_g, after_g)
        ru.check_against_model(res_r, ref_r, "radiance query, no_lds=%s" % no_lds)
        gu.check_against_model(res_g, ref_g, "gather, no_lds=%s" % no_lds)
        for tag, st, counts in (("radiance query", st_r, counts_r), ("radiance query, read after the gather", after_r, counts_r),
                                ("gather", st_g, counts_g), ("gather, read again", after_g, counts_g)):
            gu.check_counts(st, counts, 130, 2, tag)
            assert st["lds"] == lds and st["workgroups"] == 1, (tag, st)
        again = r.traceRadiance(rays, 4, 2, gu.SEED)
        assert np.array_equal(ru.result_words(again), ru.result_words(res_r)), "the second radiance query differs from the first"
    finally:
        r.destroy()


@pytest.mark.parametrize("no_lds", [None, "1"])
def test_t_max_and_depth(W, monkeypatch, no_lds):
    b, m, points = _scene(W, "cornell")
    n = points.shape[0]
    r = _renderer(W, monkeypatch, b, no_lds)
    try:
        # a finite t_max shorter than the nearest surface: half the smallest first-hit distance of the point's own eight
        # sample directions (the model's), 0.25 where all eight miss
        dist = np.full(n, np.float32(1e30))
        dirs = m.gatherDirections(points, 8, gu.SEED)
        for s in range(8):
            t, _ = m.traceRadiance(gu.sample_rays(points, dirs, s), 0, 1, 0)
            dist = np.minimum(dist, t[:, 3])
        short = points.copy()
        short[:, 3] = np.where(dist < 1e30, np.float32(0.5) * dist, np.float32(0.25))
        ref_s, hits_s, counts_s = m.gatherIrradiance(short, 4, 8, gu.SEED)
        assert not hits_s.any() and (dist < 1e30).sum() >= 3 * n // 4
        res = r.gatherIrradiance(short, 4, 8, gu.SEED)
        gu.check_against_model(res, ref_s, "t_max below the nearest surface")
        assert not gu.result_words(res).any()                   # rgb = +0, hit_fraction = +0
        # a finite t_max that cuts some first segments and not others
        mixed = points.copy()
        mixed[:, 3] = np.float32(0.6)
        ref_m, hits_m, counts_m = m.gatherIrradiance(mixed, 4, 8, gu.SEED)
        full, hits_f, _ = _ref(W, "cornell", 4, 8)
        assert 100 <= (hits_m < hits_f).sum() and 100 <= (hits_m > 0).sum()
        _gather_and_check(r, mixed, 4, 8, ref_m, counts_m, "finite t_max")
        # max_depth = 0: every first segment is traced, nothing is shaded
        ref_0, hits_0, counts_0 = _ref(W, "cornell", 0, 4)
        st = _gather_and_check(r, points, 0, 4, ref_0, counts_0, "max_depth 0")
        res = r.gatherIrradiance(points, 0, 4, gu.SEED)
        assert not ru.u32(res["rgb"]).any()
        assert np.array_equal(ru.u32(res["hit_fraction"]), ru.u32(ref_0[:, 3])) and hits_0.any()
        assert st["extension_rays"] == 4 * n and st["shadow_rays"] == 0 and st["shaded_hits"] == 0
    finally:
        r.destroy()


def _degenerate_points(points):
    """Eight ordinary points, untouched, followed by each of them with ONE component of position, t_max or normal replaced
    by each of SPECIALS, and once with an all-zero normal"""
    base = points[40:48]
    out = [b.copy() for b in base]
    for b in base:
        for comp in (0, 1, 2, 3, 4, 5, 6):
            for v in rq.SPECIALS:
                p = b.copy()
                p[comp] = v
                out.append(p)
        p = b.copy()
        p[4:7] = 0.0
        out.append(p)
    return np.ascontiguousarray(np.stack(out), np.float32)


@pytest.mark.parametrize("scene", ["cornell", "instanced1000"])
@pytest.mark.parametrize("no_lds", [None, "1"])
def test_degenerate_points(W, monkeypatch, scene, no_lds):
    """One component NaN / +-inf / +-0 / denormal / +-3e38, or a zero normal: the call returns (the walks terminate for any
    bit pattern and the depth is bounded) with the model's results; NaNs compare as a class only in rows where the model has
    one, and the untouched points of the same call are bit-exact."""
    b, m, points = _scene(W, scene)
    pts = _degenerate_points(points)
    assert pts.shape[0] == 8 + 8 * (7 * 8 + 1)
    r = _renderer(W, monkeypatch, b, no_lds)
    try:
        for depth, spp in ((4, 8), (8, 1)):
            ref, _, _ = m.gatherIrradiance(pts, depth, spp, gu.SEED)
            res = r.gatherIrradiance(pts, depth, spp, gu.SEED)
            tag = "degenerate %s no_lds=%s depth %d" % (scene, no_lds, depth)
            gu.check_against_model(res, ref, tag, nan_as_class=True)
            assert not np.isnan(ref[:8]).any(), tag
            assert np.array_equal(gu.result_words(res)[:8], ru.u32(ref[:8])), tag
            alone = r.gatherIrradiance(pts[:8], depth, spp, gu.SEED)
            assert np.array_equal(gu.result_words(alone), gu.result_words(res)[:8]), tag
    finally:
        r.destroy()


def _render(W, b, frames_a, frames_b, between):
    r = W.WebGPURenderer(0)
    r.buildPipeline(6, 1)
    W.upload_scene(r, b, 96, 64)
    r.setLookahead(8)
    r.resetCounters()
    for f in frames_a:
        r.compute(f)
        r.present()
    between(r)
    for f in frames_b:
        r.compute(f)
        r.present()
    r.sync()
    out = (r.readAccum().copy(), r.captureFrame()["data"].copy(), r.getCounters(), [a.copy() for a in r.readGBuffer()], r.readUniforms().copy())
    r.destroy()
    return out


@pytest.mark.parametrize("scene", ["cornell", "instanced1000"])
def test_gathers_leave_the_render_alone(W, scene):
    """Frames 1-4, irradiance gathers, frames 5-8 with lookahead 8 against the same frames without a gather: accumulation,
    presented image, counters, G-buffer and uniforms are equal; the gathers themselves equal the model."""
    b, m, points = _scene(W, scene)
    W._build.build_rt()

    def gathers(r):
        for depth, spp in ((4, 8), (8, 1)):
            ref, _, counts = _ref(W, scene, depth, spp)
            _gather_and_check(r, points, depth, spp, ref, counts, "%s between frames, depth %d" % (scene, depth))

    got = _render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), gathers)
    want = _render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), lambda r: None)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "accumulation"
    assert np.array_equal(got[1], want[1]), "captureFrame"
    assert got[2] == want[2], (got[2], want[2])
    for a, w in zip(got[3], want[3]):
        assert np.array_equal(pu.bits(a), pu.bits(w)), "G-buffer"
    assert np.array_equal(got[4], want[4]), "uniforms"


def test_device_entry_on_a_torch_side_stream(W, monkeypatch):
    import torch
    from webgpu_raytracer_amd import renderer as R
    b, m, points = _scene(W, "instanced1000")
    n = points.shape[0]
    ref, hits, counts = _ref(W, "instanced1000", 4, 8)
    r = _renderer(W, monkeypatch, b)
    try:
        r.buildPipeline(4, 1)
        host = r.gatherIrradiance(points, 4, 8, gu.SEED)
        side = torch.cuda.Stream()
        r.setStream(side.cuda_stream)
        with torch.cuda.stream(side):
            d_points = torch.from_numpy(np.array(points)).cuda(non_blocking=False)
            d_out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            # a gather and a frame queued back to back: nothing here waits for the GPU
            r.gatherIrradianceDevice(d_points.data_ptr(), n, d_out.data_ptr(), 4, 8, gu.SEED)
            r.compute(1)
            n_hit = (d_out[:, 3] > 0).sum()            # a torch op on the same stream, behind the gather
        side.synchronize()
        got = d_out.cpu().numpy().view(R.IRRADIANCE_DTYPE).reshape(-1)
        assert np.array_equal(gu.result_words(got), gu.result_words(host))
        gu.check_against_model(got, ref, "device entry")
        assert int(n_hit) == int((hits > 0).sum())
        st = r.irradianceGatherStats()
        assert st["rays"] == n and st["samples"] == 8 * n and st["nodes_visited"] == 0   # counting is off on the device entry ...
        assert st["extension_rays"] == int(counts[:, 0].sum()) and st["shadow_rays"] == int(counts[:, 1].sum())
        r.setCounting(True)
        with torch.cuda.stream(side):
            r.gatherIrradianceDevice(d_points.data_ptr(), n, d_out.data_ptr(), 4, 8, gu.SEED)
        gu.check_counts(r.irradianceGatherStats(), counts, n, 8, "device entry, counting")   # ... until asked for
        assert r.L.rt_gather_irradiance_device(r.ctx, d_points.data_ptr() + 8, 4, 4, 2, 0, d_out.data_ptr()) == RT_ERR_INVALID   # misaligned
        r.setStream(None)
    finally:
        r.destroy()


class _Arrays:
    """the arrays of a device-resident world, read back (rt_world_read), with the bridge's textures and camera"""

    def __init__(self, r, bridge):
        for name in ("vertices", "normals", "uvs", "mesh_topology", "tlas", "blas", "instances", "lights", "draw_commands"):
            setattr(self, name, r.worldRead(name))
        self.bridge = bridge


def test_device_resident_animated_scene(W):
    """rt_world_update at two times: the gather follows the new frame.  The arrays never reach the host on their way to the
    kernels; the model gets them from rt_world_read."""
    import test_gltf
    glb = test_gltf.big_skinned_glb(W, 48, 24)[0]
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    try:
        dev_b = W.WorldBridge()
        dev_b.setDeviceUpdater(r)
        dev_b.loadScene("viewer", glbData=glb)
        seen = []
        for t in (0.4, 1.7):
            dev_b.update(t)
            assert dev_b.deviceResident, dev_b.deviceWarning
            a = _Arrays(r, dev_b)
            n_lights = len(a.lights) // 2
            dev_b.updateCamera(16, 16)
            r.updateSceneUniforms(dev_b.cameraData, 0, n_lights)
            m = gu.GatherModel()
            m.buildPipeline(4, 1)
            m.loadTexturesFromWorld(dev_b)
            m.updateCombinedGeometry(a.vertices, a.normals, a.uvs)
            m.updateCombinedBVH(a.tlas, a.blas)
            m.updateBuffer("topology", a.mesh_topology)
            m.updateBuffer("instance", a.instances)
            m.updateBuffer("lights", a.lights)
            m.updateScreenSize(16, 16)
            m.updateSceneUniforms(dev_b.cameraData, 0, n_lights)
            if not seen:   # the points of the first frame, kept for the second
                points = gu.scene_points(m, a)
            for depth, spp in ((4, 8), (0, 4)):
                ref, hits, counts = m.gatherIrradiance(points, depth, spp, gu.SEED)
                assert (hits > 0).sum() >= 50
                _gather_and_check(r, points, depth, spp, ref, counts, "device world t=%g depth %d" % (t, depth))
                if depth == 4:
                    seen.append(ref.copy())
        assert not np.array_equal(ru.u32(seen[0]), ru.u32(seen[1])), "the two frames gather the same: nothing moved"
    finally:
        r.destroy()


def test_errors(W, monkeypatch):
    from webgpu_raytracer_amd import renderer as R
    b, m, points = _scene(W, "cornell")
    points = np.array(points)
    monkeypatch.delenv("MI355RT_NO_LDS_STAGING", raising=False)
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    try:
        out = np.zeros(points.shape[0], R.IRRADIANCE_DTYPE)
        st = R.RtRadianceStats()
        call = r.L.rt_gather_irradiance
        assert call(r.ctx, points.ctypes.data, 16, 4, 1, 0, out.ctypes.data, None) == RT_ERR_NOT_READY and r.L.rt_last_error(r.ctx)
        assert call(r.ctx, points.ctypes.data, 0, 4, 1, 0, out.ctypes.data, ctypes.addressof(st)) == 0          # n == 0
        W.upload_scene(r, b, 16, 16)
        assert call(r.ctx, points.ctypes.data, 16, 4, 0, 0, out.ctypes.data, None) == RT_ERR_INVALID           # spp = 0
        assert call(r.ctx, points.ctypes.data, 16, 4, 65537, 0, out.ctypes.data, None) == RT_ERR_INVALID
        assert call(r.ctx, None, 16, 4, 1, 0, out.ctypes.data, None) == RT_ERR_INVALID
        assert call(r.ctx, points.ctypes.data, 16, 4, 1, 0, None, None) == RT_ERR_INVALID
        assert call(r.ctx, points.ctypes.data, 1 << 31, 4, 1, 0, out.ctypes.data, None) == RT_ERR_INVALID
        assert r.L.rt_irradiance_gather_stats(r.ctx, None) == RT_ERR_INVALID
        assert call(r.ctx, points.ctypes.data, 16, 4, 1, 0, out.ctypes.data, None) == 0
        # spp = 65536 is accepted (one point, depth 1)
        assert call(r.ctx, points.ctypes.data, 1, 1, 65536, 0, out.ctypes.data, None) == 0
        # a light count above the lights buffer
        b.updateCamera(16, 16)
        r.updateSceneUniforms(b.cameraData, 0, len(np.asarray(b.lights)) // 2 + 1)
        assert call(r.ctx, points.ctypes.data, 16, 4, 1, 0, out.ctypes.data, None) == RT_ERR_INVALID
        assert b"light_count" in r.L.rt_last_error(r.ctx)
        r.updateSceneUniforms(b.cameraData, 0, b.lightCount)
        # timing
        res, s = r.gatherIrradiance(points, 4, 1, gu.SEED, stats=True)
        assert s["kernel_ms"] == 0.0
        r.setKernelTiming(True)
        res, s = r.gatherIrradiance(points, 4, 1, gu.SEED, stats=True)
        assert s["kernel_ms"] > 0.0
    finally:
        r.destroy()
