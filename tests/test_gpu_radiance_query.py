"""Radiance queries on the GPU (rt_trace_radiance, k_radiance_query) against the reference model (tests/model/
radiance_model.cpp, tied to the oracle by tests/test_radiance_model.py), ray by ray: rgb and t bit for bit, the ray, hit,
node and triangle counters as sums, in the LDS and the global-memory form; textures and transforms; independence of the
ray's place in the array; t_max, max_depth = 0; degenerate rays; no side effect on a render; the device entry on a torch
side stream; the device-resident animated world; the error returns."""
import ctypes

import numpy as np
import pytest

import parity_util as pu
import radiance_util as ru
import random_scene
import ray_query_util as rq
from test_bvh_independent import _random_rays

pytestmark = pytest.mark.gpu

RT_ERR_INVALID, RT_ERR_NOT_READY = -1, -3
SETTINGS = ((4, 2), (8, 1), (1, 1))      # (max_depth, spp)
_cache = {}


def _rays(b, finite_t_max=False):
    """4 000 rays of the scene in the rt_ray layout, pad = 7 i + 3"""
    return ru.with_pads(rq.to_rt_rays(rq.scene_rays(b, finite_t_max, 2500, 1500)))


def _scene(W, scene):
    """(bridge, model, rays) of a scene, made once"""
    if scene not in _cache:
        b = pu.bridge_for(W, scene)
        _cache[scene] = (b, ru.model_for(W, b), _rays(b), {})
    return _cache[scene][:3]


def _ref(W, scene, depth, spp):
    """the model's (out, counts) for the scene's rays, computed once and left unchanged"""
    b, m, rays = _scene(W, scene)
    refs = _cache[scene][3]
    if (depth, spp) not in refs:
        out, counts = m.traceRadiance(rays, depth, spp, ru.SEED)
        out.setflags(write=False)
        counts.setflags(write=False)
        refs[depth, spp] = (out, counts)
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


def _query_and_check(r, rays, depth, spp, ref, counts, tag, seed=ru.SEED):
    res, st = r.traceRadiance(rays, depth, spp, seed, stats=True)
    print(tag, "lds", st["lds"], "workgroups", st["workgroups"], {k: st[k] for k in ru.COUNT_NAMES})
    ru.check_against_model(res, ref, tag)
    ru.check_counts(st, counts, rays.shape[0], spp, tag)
    assert 1 <= st["workgroups"] <= (rays.shape[0] + 255) // 256, tag
    plain = r.traceRadiance(rays, depth, spp, seed)
    assert np.array_equal(ru.result_words(plain), ru.result_words(res)), (tag, "counting and product kernel differ")
    st2 = r.radianceQueryStats()
    assert st2["extension_rays"] == st["extension_rays"] and st2["shadow_rays"] == st["shadow_rays"], tag
    assert st2["nodes_visited"] == 0 and st2["tris_tested"] == 0 and st2["shaded_hits"] == 0, tag
    return st


@pytest.mark.parametrize("scene,no_lds,lds", [("cornell", None, 1), ("cornell", "1", 0), ("special", None, 0),
                                              ("instanced1000", None, 0), ("glass_blob", None, 0)])
def test_bit_parity_with_the_model(W, monkeypatch, scene, no_lds, lds):
    b, m, rays = _scene(W, scene)
    n = rays.shape[0]
    assert n == 4000
    ref, _ = _ref(W, scene, 4, 2)
    hits, lit = int((ref[:, 3] < 1e30).sum()), int((ref[:, :3].max(axis=1) > 0).sum())
    print(scene, "model: hits", hits, "lit", lit, "of", n)
    assert 5 * hits >= 3 * n and 5 * lit >= n, (scene, hits, lit)      # parity must not pass on darkness
    r = _renderer(W, monkeypatch, b, no_lds)
    try:
        for depth, spp in SETTINGS:
            ref, counts = _ref(W, scene, depth, spp)
            st = _query_and_check(r, rays, depth, spp, ref, counts, "%s no_lds=%s depth %d spp %d" % (scene, no_lds, depth, spp))
            assert st["lds"] == lds, (scene, no_lds, st)
    finally:
        r.destroy()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_textures_and_transforms(W, monkeypatch, seed):
    b = random_scene.make(seed, with_textures=True)
    m = ru.model_for(W, b)
    rays = ru.with_pads(rq.to_rt_rays(_random_rays(b, 3000, 40 + seed)))
    r = _renderer(W, monkeypatch, b)
    try:
        for depth, spp in ((6, 2), (3, 1)):
            ref, counts = m.traceRadiance(rays, depth, spp, ru.SEED)
            if depth == 6:
                assert (ref[:, 3] < 1e30).sum() >= 100 and (ref[:, :3].max(axis=1) > 0).sum() >= 50, seed
            _query_and_check(r, rays, depth, spp, ref, counts, "random scene %d depth %d spp %d" % (seed, depth, spp))
    finally:
        r.destroy()


@pytest.mark.parametrize("no_lds", [None, "1"])
def test_results_do_not_depend_on_scheduling(W, monkeypatch, no_lds):
    b, m, rays = _scene(W, "cornell")
    n = rays.shape[0]
    ref, _ = _ref(W, "cornell", 4, 2)
    r = _renderer(W, monkeypatch, b, no_lds)
    try:
        full = r.traceRadiance(rays, 4, 2, ru.SEED)
        ru.check_against_model(full, ref, "full")
        # the same rays shuffled give the same results shuffled
        perm = np.random.default_rng(9).permutation(n)
        shuffled = r.traceRadiance(rays[perm], 4, 2, ru.SEED)
        assert np.array_equal(ru.result_words(shuffled), ru.result_words(full)[perm])
        # the first k rays alone give a prefix of the full result
        for k in (1, 63, 64, 65, 129, 4000):
            part, st = r.traceRadiance(rays[:k], 4, 2, ru.SEED, stats=True)
            assert np.array_equal(ru.result_words(part), ru.result_words(full)[:k]), k
            assert st["rays"] == k and st["samples"] == 2 * k
        # n == 0
        none, st = r.traceRadiance(rays[:0], 4, 2, ru.SEED, stats=True)
        assert none.shape == (0,) and st["rays"] == 0 and st["workgroups"] == 0
        assert r.L.rt_trace_radiance(r.ctx, None, 0, 4, 2, ru.SEED, None, None) == 0
        # two copies of a ray with the same pad agree, wherever they stand
        twice = np.concatenate([rays[:300], rays[100:101], rays[300:700], rays[100:101]])
        res = ru.result_words(r.traceRadiance(twice, 4, 2, ru.SEED))
        assert np.array_equal(res[300], res[100]) and np.array_equal(res[701], res[100])
        # spp = 2 is the sum / 2 of the two spp = 1 calls with seeds 2 seed and 2 seed + 1
        a = r.traceRadiance(rays, 4, 1, 2 * ru.SEED)
        c = r.traceRadiance(rays, 4, 1, 2 * ru.SEED + 1)
        want = ((np.float32(0) + a["rgb"]) + c["rgb"]) / np.float32(2)
        assert want.dtype == np.float32
        assert np.array_equal(ru.u32(want), ru.u32(full["rgb"]))
        assert np.array_equal(ru.u32(a["t"]), ru.u32(full["t"]))
    finally:
        r.destroy()


@pytest.mark.parametrize("no_lds", [None, "1"])
def test_t_max_and_depth(W, monkeypatch, no_lds):
    b, m, _ = _scene(W, "cornell")
    rays = _rays(b, finite_t_max=True)
    r = _renderer(W, monkeypatch, b, no_lds)
    try:
        ref, counts = m.traceRadiance(rays, 4, 2, ru.SEED)
        hit = ref[:, 3] != rays[:, 3]
        assert 200 <= hit.sum() <= rays.shape[0] - 200          # the finite bounds cut some first segments and not others
        _query_and_check(r, rays, 4, 2, ref, counts, "finite t_max")
        # a t_max below the first hit: a miss with the t_max bits
        open_rays = _scene(W, "cornell")[2]
        full, _ = _ref(W, "cornell", 4, 2)
        was_hit = full[:, 3] < 1e30
        short = open_rays.copy()
        short[:, 3] = np.where(was_hit, np.nextafter(full[:, 3], np.float32(0)), np.float32(0.25))
        res = r.traceRadiance(short, 4, 2, ru.SEED)
        ref_s, counts_s = m.traceRadiance(short, 4, 2, ru.SEED)
        ru.check_against_model(res, ref_s, "t_max just below the first hit")
        assert np.array_equal(ru.u32(res["t"])[was_hit], ru.u32(short[:, 3])[was_hit]) and not res["rgb"][was_hit].any()
        assert not np.signbit(res["rgb"][was_hit]).any()
        # max_depth = 0: the first segment is traced and t reported, nothing is shaded
        ref_0, counts_0 = m.traceRadiance(open_rays, 0, 2, ru.SEED)
        st = _query_and_check(r, open_rays, 0, 2, ref_0, counts_0, "max_depth 0")
        res = r.traceRadiance(open_rays, 0, 2, ru.SEED)
        assert np.array_equal(ru.u32(res["t"]), ru.u32(full[:, 3])) and not ru.u32(res["rgb"]).any()
        assert st["extension_rays"] == open_rays.shape[0] and st["shadow_rays"] == 0 and st["shaded_hits"] == 0
    finally:
        r.destroy()


@pytest.mark.parametrize("scene", ["cornell", "instanced1000"])
@pytest.mark.parametrize("no_lds", [None, "1"])
def test_degenerate_rays(W, monkeypatch, scene, no_lds):
    """One component NaN / +-inf / +-0 / denormal / +-3e38, or a zero direction: the call returns (the walks terminate for any
    bit pattern and the depth is bounded) with the model's results, NaNs compared as a class."""
    b, m, _ = _scene(W, scene)
    r = _renderer(W, monkeypatch, b, no_lds)
    try:
        for finite in (False, True):
            rays = ru.with_pads(rq.to_rt_rays(rq.degenerate_rays(b, finite)))
            for depth, spp in ((4, 2), (8, 1)):
                ref, _ = m.traceRadiance(rays, depth, spp, ru.SEED)
                assert np.isfinite(ref[:, :3]).all(), "the model gives no NaN and no infinity on these rays"
                res = r.traceRadiance(rays, depth, spp, ru.SEED)
                ru.check_against_model(res, ref, "degenerate %s no_lds=%s finite=%s depth %d" % (scene, no_lds, finite, depth),
                                       nan_as_class=True)
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
def test_queries_leave_the_render_alone(W, scene):
    """Frames 1-4, radiance queries, frames 5-8 with lookahead 8 against the same frames without a query: accumulation,
    presented image, counters, G-buffer and uniforms are equal; the queries themselves equal the model."""
    b, m, rays = _scene(W, scene)
    W._build.build_rt()

    def queries(r):
        for depth, spp in ((4, 2), (8, 1)):
            ref, counts = _ref(W, scene, depth, spp)
            _query_and_check(r, rays, depth, spp, ref, counts, "%s between frames, depth %d" % (scene, depth))

    got = _render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), queries)
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
    b, m, rays = _scene(W, "instanced1000")
    ref, counts = _ref(W, "instanced1000", 4, 2)
    r = _renderer(W, monkeypatch, b)
    try:
        r.buildPipeline(4, 1)
        host = r.traceRadiance(rays, 4, 2, ru.SEED)
        side = torch.cuda.Stream()
        r.setStream(side.cuda_stream)
        with torch.cuda.stream(side):
            d_rays = torch.from_numpy(rays).cuda(non_blocking=False)
            d_out = torch.empty((rays.shape[0], 4), dtype=torch.float32, device="cuda")
            # a query and a frame queued back to back: nothing here waits for the GPU
            r.traceRadianceDevice(d_rays.data_ptr(), rays.shape[0], d_out.data_ptr(), 4, 2, ru.SEED)
            r.compute(1)
            n_hit = (d_out[:, 3] < 1e30).sum()            # a torch op on the same stream, behind the query
        side.synchronize()
        got = d_out.cpu().numpy().view(R.RADIANCE_DTYPE).reshape(-1)
        assert np.array_equal(ru.result_words(got), ru.result_words(host))
        ru.check_against_model(got, ref, "device entry")
        assert int(n_hit) == int((ref[:, 3] < 1e30).sum())
        st = r.radianceQueryStats()
        assert st["rays"] == rays.shape[0] and st["nodes_visited"] == 0        # counting is off on the device entry ...
        assert st["extension_rays"] == int(counts[:, 0].sum()) and st["shadow_rays"] == int(counts[:, 1].sum())
        r.setCounting(True)
        with torch.cuda.stream(side):
            r.traceRadianceDevice(d_rays.data_ptr(), rays.shape[0], d_out.data_ptr(), 4, 2, ru.SEED)
        ru.check_counts(r.radianceQueryStats(), counts, rays.shape[0], 2, "device entry, counting")   # ... until asked for
        assert r.L.rt_trace_radiance_device(r.ctx, d_rays.data_ptr() + 8, 4, 4, 2, 0, d_out.data_ptr()) == RT_ERR_INVALID   # misaligned
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
    """rt_world_update at two times: the arrays never reach the host on their way to the kernels; the model gets them from
    rt_world_read."""
    import test_gltf
    glb = test_gltf.big_skinned_glb(W, 48, 24)[0]
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    try:
        dev_b = W.WorldBridge()
        dev_b.setDeviceUpdater(r)
        dev_b.loadScene("viewer", glbData=glb)
        for t in (0.4, 1.7):
            dev_b.update(t)
            assert dev_b.deviceResident, dev_b.deviceWarning
            a = _Arrays(r, dev_b)
            n_lights = len(a.lights) // 2
            dev_b.updateCamera(16, 16)
            r.updateSceneUniforms(dev_b.cameraData, 0, n_lights)
            m = ru.ModelRenderer()
            m.buildPipeline(4, 1)
            m.loadTexturesFromWorld(dev_b)
            m.updateCombinedGeometry(a.vertices, a.normals, a.uvs)
            m.updateCombinedBVH(a.tlas, a.blas)
            m.updateBuffer("topology", a.mesh_topology)
            m.updateBuffer("instance", a.instances)
            m.updateBuffer("lights", a.lights)
            m.updateScreenSize(16, 16)
            m.updateSceneUniforms(dev_b.cameraData, 0, n_lights)
            rays = ru.with_pads(rq.to_rt_rays(rq.scene_rays(a, False, 2500, 1500)))
            for depth, spp in ((4, 2), (8, 1)):
                ref, counts = m.traceRadiance(rays, depth, spp, ru.SEED)
                assert (ref[:, 3] < 1e30).sum() >= 50
                _query_and_check(r, rays, depth, spp, ref, counts, "device world t=%g depth %d" % (t, depth))
    finally:
        r.destroy()


def test_errors(W, monkeypatch):
    from webgpu_raytracer_amd import renderer as R
    b, m, rays = _scene(W, "cornell")
    monkeypatch.delenv("MI355RT_NO_LDS_STAGING", raising=False)
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    try:
        out = np.zeros(rays.shape[0], R.RADIANCE_DTYPE)
        st = R.RtRadianceStats()
        call = r.L.rt_trace_radiance
        assert call(r.ctx, rays.ctypes.data, 16, 4, 1, 0, out.ctypes.data, None) == RT_ERR_NOT_READY and r.L.rt_last_error(r.ctx)
        assert call(r.ctx, rays.ctypes.data, 0, 4, 1, 0, out.ctypes.data, ctypes.addressof(st)) == 0          # n == 0
        W.upload_scene(r, b, 16, 16)
        assert call(r.ctx, rays.ctypes.data, 16, 4, 0, 0, out.ctypes.data, None) == RT_ERR_INVALID           # spp = 0
        assert call(r.ctx, rays.ctypes.data, 16, 4, 65537, 0, out.ctypes.data, None) == RT_ERR_INVALID
        assert call(r.ctx, None, 16, 4, 1, 0, out.ctypes.data, None) == RT_ERR_INVALID
        assert call(r.ctx, rays.ctypes.data, 16, 4, 1, 0, None, None) == RT_ERR_INVALID
        assert call(r.ctx, rays.ctypes.data, 1 << 31, 4, 1, 0, out.ctypes.data, None) == RT_ERR_INVALID
        assert r.L.rt_radiance_query_stats(r.ctx, None) == RT_ERR_INVALID
        assert call(r.ctx, rays.ctypes.data, 16, 4, 1, 0, out.ctypes.data, None) == 0
        # spp = 65536 is accepted (one ray)
        assert call(r.ctx, rays.ctypes.data, 1, 1, 65536, 0, out.ctypes.data, None) == 0
        # a light count above the lights buffer
        b.updateCamera(16, 16)
        r.updateSceneUniforms(b.cameraData, 0, len(np.asarray(b.lights)) // 2 + 1)
        assert call(r.ctx, rays.ctypes.data, 16, 4, 1, 0, out.ctypes.data, None) == RT_ERR_INVALID
        assert b"light_count" in r.L.rt_last_error(r.ctx)
        r.updateSceneUniforms(b.cameraData, 0, b.lightCount)
        # timing
        res, s = r.traceRadiance(rays, 4, 1, ru.SEED, stats=True)
        assert s["kernel_ms"] == 0.0
        r.setKernelTiming(True)
        res, s = r.traceRadiance(rays, 4, 1, ru.SEED, stats=True)
        assert s["kernel_ms"] > 0.0
    finally:
        r.destroy()
