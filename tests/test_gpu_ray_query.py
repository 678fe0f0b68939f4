"""Ray queries on the GPU (rt_trace_rays, k_ray_query) against the CPU oracle's literal traversal loop, ray by ray: every
kernel form (node / pair walk, LDS / mixed / RAYREG / global), closest and any hit, results bit for bit and the node /
triangle counters as sums; degenerate rays; t_min / t_max; no side effect on a render; the device-resident animated world;
the device entry on a torch side stream.  The reference of every comparison is OracleRenderer.traceRays."""
import ctypes

import numpy as np
import pytest

import parity_util as pu
import ray_query_util as rq

pytestmark = pytest.mark.gpu

_forms_seen = {}      # scene -> set of forms its parity test ran


def _query_and_check(r, rays_o, ref, ref_counts, shadow, tag, counters=True):
    rt = rq.to_rt_rays(rays_o)
    hits, st = r.traceRays(rt, any_hit=shadow, t_min=rq.T_MIN, stats=True)
    print(tag, rq.form_of(st), "rays", st["rays"], "nodes", st["nodes_visited"], "tris", st["tris_tested"],
          "oracle nodes", int(ref_counts[:, 0].sum()), "tris", int(ref_counts[:, 1].sum()))
    if shadow:
        rq.check_any(hits, ref, tag)
    else:
        rq.check_closest(hits, rays_o, ref, tag)
    assert st["rays"] == rays_o.shape[0], tag
    if counters:
        assert st["nodes_visited"] == int(ref_counts[:, 0].sum()), tag
        assert st["tris_tested"] == int(ref_counts[:, 1].sum()), tag
    # the product kernel (no counting) gives the same results
    plain = r.traceRays(rt, any_hit=shadow, t_min=rq.T_MIN)
    assert np.array_equal(plain.view(np.uint32), hits.view(np.uint32)), (tag, "counting and product kernel differ")
    return st


@pytest.mark.parametrize("scene", rq.SCENES)
def test_bit_parity_per_form(W, oracle_lib, monkeypatch, scene):
    b = pu.bridge_for(W, scene)
    cpu = rq.oracle_for(W, oracle_lib, b)
    sets = []
    for shadow in (False, True):
        rays = rq.scene_rays(b, shadow)
        n = rays.shape[0]
        assert n >= 20000
        ref, counts = cpu.traceRays(rays, any_hit=shadow)
        n_hit = int((ref[:, 3] != 0).sum()) if shadow else int((ref[:, 1] >= 0).sum())
        print(scene, "shadow" if shadow else "closest", "oracle hits", n_hit, "of", n)
        assert n_hit >= max(50, n // 100), (scene, shadow, n_hit)      # the oracle's own hit count on these rays
        sets.append((shadow, rays, ref, counts))
    seen = _forms_seen.setdefault(scene, set())
    for walk, no_lds, rayreg in rq.CONFIGS:
        r = rq.make_renderer(W, monkeypatch, b, walk, no_lds, rayreg)
        try:
            for shadow, rays, ref, counts in sets:
                tag = "%s walk=%d no_lds=%s rayreg=%s %s" % (scene, walk, no_lds, rayreg, "any" if shadow else "closest")
                st = _query_and_check(r, rays, ref, counts, shadow, tag)
                seen.add(rq.form_of(st))
                if walk != 2:
                    assert st["walk"] == walk, tag
                if no_lds == "1":
                    assert st["lds"] == 0, tag
                if st["walk"] == 0 and st["lds"] == 0:
                    assert st["rayreg"] == int(rayreg), tag
                assert 1 <= st["workgroups"] <= (rays.shape[0] + 255) // 256, tag
        finally:
            r.destroy()


def test_every_form_ran_on_two_scenes(W, monkeypatch):
    """rt_ray_stats.walk / lds / rayreg of the parity runs: each of the five forms on at least two scenes.  A scene whose
    parity test did not run in this session is probed here (which form each configuration picks, 256 rays)."""
    for scene in rq.SCENES:
        if scene in _forms_seen:
            continue
        b = pu.bridge_for(W, scene)
        seen = _forms_seen.setdefault(scene, set())
        rays = rq.to_rt_rays(rq.scene_rays(b, False, 128, 128))
        for walk, no_lds, rayreg in rq.CONFIGS:
            r = rq.make_renderer(W, monkeypatch, b, walk, no_lds, rayreg)
            seen.add(rq.form_of(r.traceRays(rays, stats=True)[1]))
            r.destroy()
    for form in rq.FORMS:
        scenes = sorted(s for s, f in _forms_seen.items() if form in f)
        print(form, scenes)
        assert len(scenes) >= 2, (form, scenes)


@pytest.mark.parametrize("scene", ["cornell", "mixed", "instanced1000", "special"])
def test_degenerate_rays(W, oracle_lib, monkeypatch, scene):
    """One component NaN / +-inf / +-0 / denormal / +-3e38, or a zero direction, in a call of their own: every form comes
    back with the oracle's results.  Node / triangle totals are not compared on this set (they differ on a NaN t_max)."""
    b = pu.bridge_for(W, scene)
    cpu = rq.oracle_for(W, oracle_lib, b)
    sets = []
    for shadow in (False, True):
        rays = rq.degenerate_rays(b, shadow)
        ref, counts = cpu.traceRays(rays, any_hit=shadow)
        sets.append((shadow, rays, ref, counts))
    for walk, no_lds, rayreg in rq.CONFIGS:
        r = rq.make_renderer(W, monkeypatch, b, walk, no_lds, rayreg)
        try:
            for shadow, rays, ref, counts in sets:
                tag = "degenerate %s walk=%d no_lds=%s rayreg=%s %s" % (scene, walk, no_lds, rayreg, "any" if shadow else "closest")
                _query_and_check(r, rays, ref, counts, shadow, tag, counters=False)
        finally:
            r.destroy()


@pytest.mark.parametrize("walk,no_lds", [(0, None), (1, None), (0, "1"), (1, "1")])
def test_t_min_and_t_max_are_honoured(W, oracle_lib, monkeypatch, walk, no_lds):
    b = pu.bridge_for(W, "cornell")
    cpu = rq.oracle_for(W, oracle_lib, b)
    root = np.asarray(b.tlas, np.float32).reshape(-1, 8)[0]
    centre = ((root[0:3] + root[4:7]) * np.float32(0.5)).astype(np.float32)
    base = np.zeros((6, 8), np.float32)
    for k, d in enumerate(([1, 0.03, 0.02], [-1, 0.02, 0.03], [0.02, 1, 0.03], [0.03, -1, 0.02], [0.02, 0.03, 1], [0.03, 0.02, -1])):
        base[k, 0:3], base[k, 3], base[k, 4:7], base[k, 7] = centre, rq.T_MIN, np.array(d, np.float32), 1e30
    ref, _ = cpu.traceRays(base)
    assert (ref[:, 1] >= 0).sum() >= 5, ref          # the walls of the box around the centre
    t_hit = ref[:, 0].copy()
    t_hit[ref[:, 1] < 0] = 1.0
    below, above = np.nextafter(t_hit, np.float32(0)), np.nextafter(t_hit, np.float32(np.inf))
    r = rq.make_renderer(W, monkeypatch, b, walk, no_lds, "0")
    try:
        for shadow in (False, True):
            for name, t_min, t_max in (("t_max below", rq.T_MIN, below), ("t_max at", rq.T_MIN, t_hit), ("t_max above", rq.T_MIN, above),
                                       ("t_min at", t_hit, None), ("t_min above", above, None), ("t_min below", below, None)):
                for k in range(base.shape[0]):      # t_min is per call: one call per ray
                    ray = base[k:k + 1].copy()
                    tm = float(t_min[k]) if isinstance(t_min, np.ndarray) else t_min
                    ray[0, 3] = tm
                    if t_max is not None:
                        ray[0, 7] = t_max[k]
                    want, _ = cpu.traceRays(ray, any_hit=shadow)
                    got = r.traceRays(rq.to_rt_rays(ray), any_hit=shadow, t_min=tm)
                    tag = "%s ray %d %s" % (name, k, "any" if shadow else "closest")
                    if shadow:
                        rq.check_any(got, want, tag)
                    else:
                        rq.check_closest(got, ray, want, tag)
            # and the bounds do what their names say on the wall itself
            k = int(np.argmax(ref[:, 1] >= 0))
            ray = rq.to_rt_rays(base[k:k + 1])
            assert r.traceRays(ray, t_min=rq.T_MIN)["tri"][0] == int(ref[k, 1])
            ray[0, 3] = below[k]
            assert r.traceRays(ray, t_min=rq.T_MIN)["tri"][0] != int(ref[k, 1]) or r.traceRays(ray, t_min=rq.T_MIN)["t"][0] < t_hit[k]
            ray[0, 3] = 1e30
            far = r.traceRays(ray, t_min=float(above[k]))
            assert far["hit"][0] == 0 or far["t"][0] > t_hit[k]
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
def test_queries_leave_the_render_alone(W, oracle_lib, scene):
    """Frames 1-4, queries, frames 5-8 with lookahead 8 against the same frames without a query: accumulation, presented
    image, counters, G-buffer and uniforms are equal; the queries themselves equal the oracle."""
    b = pu.bridge_for(W, scene)
    cpu = rq.oracle_for(W, oracle_lib, b)
    rays = rq.scene_rays(b, False, 1500, 500)
    ref, counts = cpu.traceRays(rays)

    def queries(r):
        _query_and_check(r, rays, ref, counts, False, scene + " between frames")
        sref, scounts = cpu.traceRays(rays, any_hit=True)
        _query_and_check(r, rays, sref, scounts, True, scene + " between frames (any)")

    got = _render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), queries)
    want = _render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), lambda r: None)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "accumulation"
    assert np.array_equal(got[1], want[1]), "captureFrame"
    assert got[2] == want[2], (got[2], want[2])
    for a, w in zip(got[3], want[3]):
        assert np.array_equal(pu.bits(a), pu.bits(w)), "G-buffer"
    assert np.array_equal(got[4], want[4]), "uniforms"


def test_query_without_a_scene_and_after_a_resize(W, oracle_lib):
    from webgpu_raytracer_amd import renderer as R
    b = pu.bridge_for(W, "cornell")
    rays = rq.scene_rays(b, False, 600, 200)
    rt = rq.to_rt_rays(rays)
    r = W.WebGPURenderer(0)
    try:
        hits = np.zeros(rt.shape[0], R.RAY_HIT_DTYPE)
        RT_ERR_INVALID, RT_ERR_NOT_READY = -1, -3
        rc = r.L.rt_trace_rays(r.ctx, rt.ctypes.data, rt.shape[0], 0, 0.001, hits.ctypes.data, None)
        assert rc == RT_ERR_NOT_READY and r.L.rt_last_error(r.ctx)
        assert r.L.rt_trace_rays(r.ctx, rt.ctypes.data, 0, 0, 0.001, hits.ctypes.data, None) == 0          # n == 0
        assert r.L.rt_trace_rays(r.ctx, None, 4, 0, 0.001, hits.ctypes.data, None) == RT_ERR_INVALID
        assert r.L.rt_trace_rays(r.ctx, rt.ctypes.data, 4, 0, 0.001, None, None) == RT_ERR_INVALID
        assert r.L.rt_trace_rays(r.ctx, rt.ctypes.data, 4, 2, 0.001, hits.ctypes.data, None) == RT_ERR_INVALID   # unknown mode
        assert r.L.rt_trace_rays(r.ctx, rt.ctypes.data, 1 << 31, 0, 0.001, hits.ctypes.data, None) == RT_ERR_INVALID
        assert r.L.rt_trace_rays_device(r.ctx, 8, 4, 0, 0.001, 16) == RT_ERR_INVALID                      # misaligned
        assert r.L.rt_ray_query_stats(r.ctx, None) == RT_ERR_INVALID
        cpu = rq.oracle_for(W, oracle_lib, b)
        ref, counts = cpu.traceRays(rays)
        r.buildPipeline(4, 1)
        W.upload_scene(r, b, 64, 48)
        r.compute(1)
        _query_and_check(r, rays, ref, counts, False, "before the resize")
        r.updateScreenSize(40, 24)
        _query_and_check(r, rays, ref, counts, False, "after the resize")
        st = r.rayQueryStats()
        assert st["rays"] == rays.shape[0] and st["kernel_ms"] == 0.0
        r.setKernelTiming(True)
        _, st = r.traceRays(rt, stats=True)
        assert st["kernel_ms"] > 0.0
    finally:
        r.destroy()


def test_device_resident_animated_scene(W, oracle_lib):
    """rt_world_update at two times: the arrays never reach the host, and the GPU's answers are the oracle's on the
    host-built arrays of the same t."""
    import test_gltf
    glb = test_gltf.big_skinned_glb(W, 48, 24)[0]
    r = W.WebGPURenderer(0)
    try:
        cpu_b, dev_b = W.WorldBridge(), W.WorldBridge()
        dev_b.setDeviceUpdater(r)
        cpu_b.loadScene("viewer", glbData=glb)
        dev_b.loadScene("viewer", glbData=glb)
        for t in (0.4, 1.7):
            cpu_b.update(t)
            dev_b.update(t)
            assert dev_b.deviceResident, dev_b.deviceWarning
            cpu = oracle_lib.OracleRenderer()
            cpu.buildPipeline(4, 1)
            cpu.loadTexturesFromWorld(cpu_b)
            W.upload_scene(cpu, cpu_b, 16, 16)
            for shadow in (False, True):
                rays = rq.scene_rays(cpu_b, shadow, 3000, 1000)
                ref, counts = cpu.traceRays(rays, any_hit=shadow)
                n_hit = int((ref[:, 3] != 0).sum()) if shadow else int((ref[:, 1] >= 0).sum())
                assert n_hit >= 50, n_hit
                for walk in (0, 1):
                    r.setWalk(walk)
                    _query_and_check(r, rays, ref, counts, shadow, "device world t=%g walk=%d %s" % (t, walk, "any" if shadow else "closest"))
    finally:
        r.destroy()


def test_device_entry_on_a_torch_side_stream(W, oracle_lib):
    import torch
    b = pu.bridge_for(W, "instanced1000")
    cpu = rq.oracle_for(W, oracle_lib, b)
    rays = rq.scene_rays(b, False, 6000, 2000)
    srays = rq.scene_rays(b, True, 6000, 2000)
    ref, counts = cpu.traceRays(rays)
    sref, _ = cpu.traceRays(srays, any_hit=True)
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    try:
        r.buildPipeline(4, 1)
        W.upload_scene(r, b, 64, 48)
        host_closest = r.traceRays(rq.to_rt_rays(rays), t_min=rq.T_MIN)
        host_any = r.traceRays(rq.to_rt_rays(srays), any_hit=True, t_min=rq.T_MIN)
        side = torch.cuda.Stream()
        r.setStream(side.cuda_stream)
        with torch.cuda.stream(side):
            d_rays = torch.from_numpy(rq.to_rt_rays(rays)).cuda(non_blocking=False)
            d_srays = torch.from_numpy(rq.to_rt_rays(srays)).cuda(non_blocking=False)
            d_hits = torch.empty((rays.shape[0], 4), dtype=torch.int32, device="cuda")
            d_shits = torch.empty((srays.shape[0], 4), dtype=torch.int32, device="cuda")
            # two queries and a frame queued back to back: nothing here waits for the GPU
            r.traceRaysDevice(d_rays.data_ptr(), rays.shape[0], d_hits.data_ptr(), t_min=rq.T_MIN)
            r.traceRaysDevice(d_srays.data_ptr(), srays.shape[0], d_shits.data_ptr(), any_hit=True, t_min=rq.T_MIN)
            r.compute(1)
            n_hit = (d_hits[:, 3] != 0).sum()            # a torch op on the same stream, behind the queries
        side.synchronize()
        from webgpu_raytracer_amd import renderer as R
        got = d_hits.cpu().numpy().view(R.RAY_HIT_DTYPE).reshape(-1)
        sgot = d_shits.cpu().numpy().view(R.RAY_HIT_DTYPE).reshape(-1)
        assert np.array_equal(got.view(np.uint32), host_closest.view(np.uint32))
        assert np.array_equal(sgot.view(np.uint32), host_any.view(np.uint32))
        rq.check_closest(got, rays, ref, "device entry")
        rq.check_any(sgot, sref, "device entry (any)")
        assert int(n_hit) == int((ref[:, 1] >= 0).sum())
        st = r.rayQueryStats()
        assert st["rays"] == srays.shape[0] and st["nodes_visited"] == 0        # counting is off on the device entry ...
        r.setCounting(True)
        with torch.cuda.stream(side):
            r.traceRaysDevice(d_rays.data_ptr(), rays.shape[0], d_hits.data_ptr(), t_min=rq.T_MIN)
        st = r.rayQueryStats()
        assert st["nodes_visited"] == int(counts[:, 0].sum()) and st["tris_tested"] == int(counts[:, 1].sum())   # ... until asked for
        r.setStream(None)
    finally:
        r.destroy()
