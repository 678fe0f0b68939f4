"""Lightmap bakes on the GPU (rt_bake_points / rt_bake_points_device / rt_bake_irradiance, csrc/k_bake.hip.h) against the
reference model (tests/model/bake_model.cpp, tied to a float64 brute force by tests/test_bake_model.py): points, texel
indices, count and owner map word for word; the hand-worked cases; the bake as the composition of the GPU's own points and
gather; independence of scheduling and of cap; the device entry on a torch side stream, and its owner map without points; scratch shared with atlas bakes; the
device-resident animated world;
no side effect on a render; the error returns.

The atlas sizes are the smallest that cross the kernels' edges: 1 x 1, one row of 130 (three waves of the count pass, one
partial), 7 x 5 (one partial 8 x 8 tile), 64 x 64 (full tiles, 16 count workgroups), 65 x 63 (a 65th column, a partial last
tile row) and 257 x 3 (four count workgroups, the last with three texels); 1024 x 1024 crosses the split of a big box into
bands of tile rows and gives the scan 4096 workgroup totals (four per scan thread).

Parity must not pass on emptiness: the model's covered share is asserted > 10 % for every (scene, layout, size) - except
1 x 1 and 7 x 5 under the GRID layout, where it cannot be demanded: a chart of that layout is a third of one of at least 36
cells, smaller than a texel of an atlas of 35 texels or fewer, so most centres miss every chart (the deliberate n = 0 end of
the range).  The scene-uv layout carries those two sizes, and there the share is asserted too."""
import ctypes

import numpy as np
import pytest

import bake_util as bu
import gather_util as gu
import parity_util as pu
import random_scene

pytestmark = pytest.mark.gpu

RT_ERR_INVALID, RT_ERR_NOT_READY = -1, -3
SIZES = ((1, 1), (1, 130), (7, 5), (64, 64), (65, 63), (257, 3))
_cache = {}


def _scene(W, name):
    """(bridge, model) of a scene, made once"""
    if name not in _cache:
        b = random_scene.make(int(name[6:])) if name.startswith("random") else pu.bridge_for(W, name)
        _cache[name] = (b, bu.model_for(W, b))
    return _cache[name]


def _renderer(W, bridge):
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    W.upload_scene(r, bridge, 16, 16)
    return r


def check_points(got, want, tag):
    """(points, texels, owner) of the GPU against the model's, word for word; in rows where the MODEL has a NaN, NaNs
    compare as a class and everything else of the row stays bit-exact"""
    gp, gt, go = got
    wp, wt, wo = want
    assert np.array_equal(go, wo), (tag, "owner maps differ at", np.argwhere(go != wo)[:8].tolist())
    assert len(gt) == len(wt) and np.array_equal(gt, wt), (tag, "texel indices", len(gt), len(wt))
    g, w = gp.view(np.uint32), wp.view(np.uint32)
    bad = g != w
    model_nan_row = np.isnan(wp).any(axis=1)
    bad &= ~(np.isnan(gp) & np.isnan(wp) & model_nan_row[:, None])
    rows = np.nonzero(bad.any(axis=1))[0]
    assert rows.size == 0, (tag, "points that differ", int(rows.size), rows[:8].tolist(), gp[rows[:4]].tolist(), wp[rows[:4]].tolist())


CASES = [("cornell", 0, "scene"), ("cornell", 0, "grid"), ("special", 0, "scene"), ("special", 0, "grid"),
         ("instanced1000", 0, "scene"), ("instanced1000", 1, "grid"), ("instanced1000", 3, "grid"),
         ("random1", 0, "scene"), ("random1", 2, "grid"), ("random2", 1, "scene"), ("random2", 0, "grid")]


@pytest.mark.parametrize("scene,inst,layout", CASES)
def test_bit_parity_with_the_model(W, scene, inst, layout):
    b, m = _scene(W, scene)
    uv = bu.grid_uv(b, inst) if layout == "grid" else None
    r = _renderer(W, b)
    try:
        for width, height in SIZES:
            want = m.bakePoints(inst, width, height, t_max=5.0, pad_base=1000, atlas_uv=uv)
            share = len(want[1]) / (width * height)
            print(scene, inst, layout, (width, height), "covered share %.3f" % share, "owners", len(np.unique(want[2])) - 1)
            if layout == "scene" or width * height > 35:
                assert share > 0.1, (scene, inst, layout, width, height, share)
            got = r.bakePoints(inst, width, height, t_max=5.0, pad_base=1000, atlas_uv=uv, owner=True)
            check_points(got, want, "%s inst %d %s %dx%d" % (scene, inst, layout, width, height))
    finally:
        r.destroy()


def test_two_instances_of_one_geometry(W):
    """instanced1000: instances 1 and 3 share their triangles - the same owner map, other points"""
    b, m = _scene(W, "instanced1000")
    assert bu.instance_triangles(b, 1) == bu.instance_triangles(b, 3)
    r = _renderer(W, b)
    try:
        uv = bu.grid_uv(b, 1)
        p1, t1, o1 = r.bakePoints(1, 64, 64, atlas_uv=uv, owner=True)
        p3, t3, o3 = r.bakePoints(3, 64, 64, atlas_uv=uv, owner=True)
        assert np.array_equal(o1, o3) and np.array_equal(t1, t3) and len(t1) > 400
        assert not np.array_equal(p1[:, 0:3], p3[:, 0:3])
    finally:
        r.destroy()


def test_the_big_box_split_at_1024(W):
    b, m = _scene(W, "cornell")
    r = _renderer(W, b)
    try:
        want = m.bakePoints(0, 1024, 1024)
        assert len(want[1]) > 0.1 * 1024 * 1024
        check_points(r.bakePoints(0, 1024, 1024, owner=True), want, "cornell 1024x1024")
    finally:
        r.destroy()


def test_hand_worked_cases(W):
    """the written answers of bake_util.hand_cases, laid over the first triangles of instance 0 of a random scene"""
    b, m = _scene(W, "random1")
    first, _ = bu.instance_triangles(b, 0)
    r = _renderer(W, b)
    try:
        for name, (tri_uvs, width, height, want) in sorted(bu.hand_cases().items()):
            want = np.asarray(want)
            want = np.where(want >= 0, want + first, -1)
            uv = bu.hand_uv(b, 0, tri_uvs)
            points, texels, owner = r.bakePoints(0, width, height, t_max=2.0, pad_base=5, atlas_uv=uv, owner=True)
            assert owner.tolist() == want.tolist(), name
            assert np.array_equal(texels, np.flatnonzero(want.ravel() >= 0)), name
            assert np.array_equal(points.view(np.uint32)[:, 7], 5 + texels), name
            check_points((points, texels, owner), m.bakePoints(0, width, height, t_max=2.0, pad_base=5, atlas_uv=uv), name)
    finally:
        r.destroy()


def test_special_values_in_the_scene(W):
    """zero, non-finite and denormal vertex normals: rows where the model has a NaN compare as a class, every other row of
    the same call bit for bit"""
    b = random_scene.make(1)
    first, count = bu.instance_triangles(b, 0)
    topo = np.asarray(b.mesh_topology, np.uint32).reshape(-1, 20)
    nrm = np.asarray(b.normals, np.float32).reshape(-1, 4).copy()
    nrm[topo[first, 0:3], 0:3] = 0.0                      # a triangle whose normals are all zero: NaN normals
    nrm[topo[first + 3, 0], 0] = np.inf
    nrm[topo[first + 4, 1], 1] = np.nan
    nrm[topo[first + 5, 2], 2] = np.float32(1e-42)        # denormal
    b.normals = nrm.reshape(-1)
    uv = bu.grid_uv(b, 0)
    m = bu.model_for(W, b)
    r = _renderer(W, b)
    try:
        want = m.bakePoints(0, 64, 64, atlas_uv=uv)
        assert np.isnan(want[0]).any(axis=1).sum() >= 10 and (~np.isnan(want[0]).any(axis=1)).sum() >= 400
        check_points(r.bakePoints(0, 64, 64, atlas_uv=uv, owner=True), want, "special values")
    finally:
        r.destroy()


@pytest.mark.parametrize("depth,spp", [(4, 8), (0, 4)])
def test_a_bake_is_points_then_gather_then_scatter(W, depth, spp):
    from webgpu_raytracer_amd import renderer as R
    b, m = _scene(W, "cornell")
    uv = bu.grid_uv(b, 0)
    r = _renderer(W, b)
    try:
        points, texels = r.bakePoints(0, 64, 64, atlas_uv=uv)
        res, gst = r.gatherIrradiance(points, depth, spp, bu.SEED, stats=True)
        atlas, n, st = r.bakeIrradiance(0, 64, 64, depth, spp, bu.SEED, atlas_uv=uv, stats=True)
        assert atlas.shape == (64, 64) and atlas.dtype == R.IRRADIANCE_DTYPE
        words = atlas.view(np.uint32).reshape(-1, 4)
        assert n == len(texels) and 400 < n < 0.8 * 4096
        assert np.array_equal(words[texels], gu.result_words(res))
        none = np.ones(4096, bool)
        none[texels] = False
        assert np.array_equal(words[none], np.tile(np.array([0, 0, 0, -1], np.float32).view(np.uint32), (none.sum(), 1)))
        for k in gst:
            if k != "kernel_ms":
                assert st[k] == gst[k], (k, st[k], gst[k])
        want, wpoints, wtexels, counts = m.bakeIrradiance(0, 64, 64, depth, spp, bu.SEED, atlas_uv=uv)
        assert np.array_equal(words, want.reshape(-1, 4).view(np.uint32))
        gu.check_counts(st, counts, n, spp, "bake stats")
        plain = r.bakeIrradiance(0, 64, 64, depth, spp, bu.SEED, atlas_uv=uv)
        assert np.array_equal(plain.view(np.uint32), atlas.view(np.uint32))
    finally:
        r.destroy()


def test_a_bake_that_covers_nothing(W):
    """all override uvs (0, 0): n = 0 - no emit, no gather launch, a scatter that only fills; then an ordinary bake on the
    same context"""
    b, m = _scene(W, "cornell")
    r = _renderer(W, b)
    try:
        uv = np.zeros((np.asarray(b.uvs).size // 2, 2), np.float32)
        for width, height in ((7, 5), (64, 64)):
            atlas, n, st = r.bakeIrradiance(0, width, height, 4, 8, bu.SEED, atlas_uv=uv, stats=True)
            assert n == 0 and atlas.shape == (height, width)
            assert np.array_equal(atlas.view(np.uint32).reshape(-1, 4),
                                  np.tile(np.array([0, 0, 0, -1], np.float32).view(np.uint32), (width * height, 1)))
            assert all(st[k] == 0 for k in st), st
            assert r.irradianceGatherStats()["rays"] == 0
        plain = r.bakeIrradiance(0, 7, 5, 4, 8, bu.SEED, atlas_uv=uv)
        assert (plain["hit_fraction"] == -1).all()
        want = m.bakeIrradiance(0, 32, 32, 4, 8, bu.SEED)[0]
        assert np.array_equal(r.bakeIrradiance(0, 32, 32, 4, 8, bu.SEED).view(np.uint32).reshape(-1, 4),
                              want.reshape(-1, 4).view(np.uint32))
    finally:
        r.destroy()


def test_scheduling_independence_and_cap(W):
    b, m = _scene(W, "random2")
    r = _renderer(W, b)
    try:
        full = r.bakePoints(1, 65, 63, owner=True)
        again = r.bakePoints(1, 65, 63, owner=True)
        for a, c in zip(full, again):
            assert np.array_equal(pu.bits(a), pu.bits(c))
        n = len(full[1])
        assert n > 600
        for cap in (n - 1, 257, 1):
            p, t, count = r.bakePoints(1, 65, 63, cap=cap)
            assert count == n and len(t) == cap
            assert np.array_equal(t, full[1][:cap]) and np.array_equal(pu.bits(p), pu.bits(full[0][:cap]))
        p, t, count = r.bakePoints(1, 65, 63, cap=0)
        assert count == n and len(t) == 0
        p, t, count = r.bakePoints(1, 65, 63, cap=n + 100)
        assert count == n and np.array_equal(pu.bits(p), pu.bits(full[0]))
    finally:
        r.destroy()


def test_device_entry_on_a_torch_side_stream(W):
    import torch
    b, m = _scene(W, "instanced1000")
    width, height = 65, 63
    want = m.bakePoints(0, width, height, pad_base=9)
    n = len(want[1])
    r = _renderer(W, b)
    try:
        r.buildPipeline(4, 1)
        side = torch.cuda.Stream()
        r.setStream(side.cuda_stream)
        with torch.cuda.stream(side):
            d_points = torch.zeros((width * height, 8), dtype=torch.float32, device="cuda")
            d_texels = torch.zeros(width * height, dtype=torch.int32, device="cuda")
            d_count = torch.zeros(4, dtype=torch.int32, device="cuda")
            d_owner = torch.zeros(width * height, dtype=torch.int32, device="cuda")
            # a bake and a frame queued back to back: nothing here waits for the GPU
            r.bakePointsDevice(0, width, height, d_points.data_ptr(), d_texels.data_ptr(), width * height, d_count.data_ptr(),
                               pad_base=9, owner_ptr=d_owner.data_ptr())
            r.compute(1)
            covered = (d_owner >= 0).sum()            # a torch op on the same stream, behind the bake
        side.synchronize()
        assert int(d_count[0]) == n == int(covered)
        got = (d_points.cpu().numpy()[:n], d_texels.cpu().numpy()[:n].view(np.uint32), d_owner.cpu().numpy().reshape(height, width))
        check_points(got, want, "device entry")
        d = bu.BakeDesc(0, width, height, 9, 1e30)
        call = r.L.rt_bake_points_device
        assert call(r.ctx, ctypes.addressof(d), None, d_points.data_ptr() + 8, d_texels.data_ptr(), 16, d_count.data_ptr(),
                    None) == RT_ERR_INVALID   # misaligned
        assert call(r.ctx, ctypes.addressof(d), None, d_points.data_ptr(), d_texels.data_ptr(), 16, None, None) == RT_ERR_INVALID
        # count only: no arrays, no owner map
        with torch.cuda.stream(side):
            d_count.zero_()
            r.bakePointsDevice(0, width, height, None, None, 0, d_count.data_ptr(), pad_base=9)
        side.synchronize()
        assert int(d_count[0]) == n
        r.setStream(None)
    finally:
        r.destroy()


@pytest.mark.parametrize("size", ((65, 63), (1, 1)))
def test_device_entry_owner_map_without_points(W, size):
    """cap = 0 and no point arrays, but an owner_ptr: the count and the u32 owner map of the model, all ones where nothing
    covers.  65 x 63 is no multiple of 256 texels, so the last workgroup of every per-texel launch is partial."""
    import torch
    b, m = _scene(W, "instanced1000")
    width, height = size
    want = m.bakePoints(0, width, height)
    assert len(want[1]) > 0.1 * width * height
    r = _renderer(W, b)
    try:
        side = torch.cuda.Stream()
        r.setStream(side.cuda_stream)
        with torch.cuda.stream(side):
            d_count = torch.zeros(4, dtype=torch.int32, device="cuda")
            d_owner = torch.zeros(width * height, dtype=torch.int32, device="cuda")
            r.bakePointsDevice(0, width, height, None, None, 0, d_count.data_ptr(), owner_ptr=d_owner.data_ptr())
        side.synchronize()
        owner = d_owner.cpu().numpy().reshape(height, width)
        assert int(d_count[0]) == len(want[1])
        assert np.array_equal(owner, want[2]), np.argwhere(owner != want[2])[:8].tolist()
        assert np.array_equal(np.flatnonzero(owner.ravel() >= 0), want[1])
        assert (owner.view(np.uint32)[want[2] < 0] == 0xffffffff).all()
        r.setStream(None)
    finally:
        r.destroy()


def test_scratch_shared_with_atlas_bakes_does_not_leak(W):
    """an atlas bake of five entries with override uvs, a 7 x 5 single bake with the scene's, the atlas bake again, on one
    context: the single bake is the model's bit for bit and the second atlas bake is the first (the two kinds of bake share
    the context's staging arrays, block counts and count word)"""
    import atlas_bake_util as au
    b, m = _scene(W, "instanced1000")
    entries = au.small_entries(au.instance_count(b))
    uv = au.merged_grid_uv(b, [e[0] for e in entries])
    want = m.bakePoints(0, 7, 5, t_max=5.0, pad_base=1000)
    assert len(want[1]) > 0.1 * 35
    r = _renderer(W, b)
    try:
        first = r.bakeAtlasPoints(entries, au.SMALL_W, au.SMALL_H, t_max=5.0, pad_base=1000, atlas_uv=uv, owner=True)
        assert len(first[1]) > 0.1 * au.SMALL_W * au.SMALL_H and first[2][:, :, 0].max() >= 3
        check_points(r.bakePoints(0, 7, 5, t_max=5.0, pad_base=1000, owner=True), want, "between two atlas bakes")
        again = r.bakeAtlasPoints(entries, au.SMALL_W, au.SMALL_H, t_max=5.0, pad_base=1000, atlas_uv=uv, owner=True)
        for a, c in zip(first, again):
            assert np.array_equal(pu.bits(a), pu.bits(c))
    finally:
        r.destroy()


class _Arrays:
    """the arrays of a device-resident world, read back (rt_world_read)"""

    def __init__(self, r):
        for name in ("vertices", "normals", "uvs", "mesh_topology", "tlas", "blas", "instances", "lights", "draw_commands"):
            setattr(self, name, r.worldRead(name))


def test_device_resident_animated_scene(W):
    """rt_world_update at two times: the points follow the skinned vertices, the coverage (uv space) does not move.  The
    arrays never reach the host on their way to the kernels; the model gets them from rt_world_read.
    The atlas layout is made once, per vertex, from the first frame and used for both: vertex ids are stable.  Triangle
    INDICES are not - every update rebuilds the skinned mesh's BLAS and packs the topology rows in its leaf order - so the
    owner map, which holds triangle indices, is compared as what does not depend on that order: which texels are owned."""
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
            a = _Arrays(r)
            m = bu.BakeModel()
            m.buildPipeline(4, 1)
            m.loadTexturesFromWorld(dev_b)
            m.updateCombinedGeometry(a.vertices, a.normals, a.uvs)
            m.updateCombinedBVH(a.tlas, a.blas)
            m.updateBuffer("topology", a.mesh_topology)
            m.updateBuffer("instance", a.instances)
            m.updateBuffer("lights", a.lights)
            m.updateBuffer("draw_commands", a.draw_commands)
            n_inst = len(a.draw_commands) // 4
            inst = int(np.argmax(np.asarray(a.draw_commands, np.uint32).reshape(-1, 4)[:, 0]))   # the skinned mesh
            if not seen:
                uv = bu.grid_uv(a, inst)
            want = m.bakePoints(inst, 64, 64, atlas_uv=uv)
            assert len(want[1]) > 0.1 * 4096 and n_inst >= 1
            got = r.bakePoints(inst, 64, 64, atlas_uv=uv, owner=True)
            check_points(got, want, "device world t=%g" % t)
            seen.append(got)
        assert np.array_equal(seen[0][2] >= 0, seen[1][2] >= 0) and np.array_equal(seen[0][1], seen[1][1])
        assert not np.array_equal(pu.bits(seen[0][0]), pu.bits(seen[1][0])), "the two frames give the same points: nothing moved"
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


def test_bakes_leave_the_render_alone(W):
    """Frames 1-4, bakes, frames 5-8 with lookahead 8 against the same frames without a bake: accumulation, presented image,
    counters, G-buffer and uniforms are equal; the radiance query's last stats are what they were before the bakes."""
    b, m = _scene(W, "cornell")
    W._build.build_rt()
    rays = np.zeros((64, 8), np.float32)
    rays[:, 0:3] = np.asarray(b.cameraData, np.float32)[0:3]
    rays[:, 3] = 1e30
    rays[:, 4:7] = (0.01 * np.arange(64)[:, None] - 0.3) * np.array([1, 0.5, 0], np.float32) + np.array([0, 0, 1], np.float32)

    def bakes(r):
        r.traceRadiance(rays, 4, 2, 3, stats=True)
        before = r.radianceQueryStats()
        check_points(r.bakePoints(0, 65, 63, owner=True), m.bakePoints(0, 65, 63), "between frames")
        atlas = r.bakeIrradiance(0, 32, 32, 4, 4, bu.SEED)
        assert np.array_equal(atlas.view(np.uint32).reshape(-1, 4),
                              m.bakeIrradiance(0, 32, 32, 4, 4, bu.SEED)[0].reshape(-1, 4).view(np.uint32))
        after = r.radianceQueryStats()
        assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in before.items() if k != "kernel_ms"}

    got = _render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), bakes)
    want = _render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), lambda r: None)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "accumulation"
    assert np.array_equal(got[1], want[1]), "captureFrame"
    assert got[2] == want[2], (got[2], want[2])
    for a, w in zip(got[3], want[3]):
        assert np.array_equal(pu.bits(a), pu.bits(w)), "G-buffer"
    assert np.array_equal(got[4], want[4]), "uniforms"


def test_errors(W):
    from webgpu_raytracer_amd import renderer as R
    b, m = _scene(W, "cornell")
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    try:
        points = np.zeros((64, 8), np.float32)
        texels = np.zeros(64, np.uint32)
        atlas = np.zeros(64, R.IRRADIANCE_DTYPE)
        n = ctypes.c_uint32(0)
        n_verts = np.asarray(b.uvs).size // 2
        uv = np.zeros((n_verts, 2), np.float32)

        def desc(inst=0, width=8, height=8, pad_base=0, reserved=0):
            d = R.RtBakeDesc(inst, width, height, pad_base, 1e30)
            d.reserved[1] = reserved
            return d

        def bake(d, uv_ptr=None, n_uv=0, p=points.ctypes.data, t=texels.ctypes.data, cap=64, count=ctypes.addressof(n)):
            return r.L.rt_bake_points(r.ctx, ctypes.addressof(d) if d is not None else None, uv_ptr, n_uv, p, t, cap, count, None)

        def irr(d, out=atlas.ctypes.data, spp=1):
            return r.L.rt_bake_irradiance(r.ctx, ctypes.addressof(d) if d is not None else None, None, 0, 4, spp, 0, out, None, None)

        assert bake(desc()) == RT_ERR_NOT_READY and r.L.rt_last_error(r.ctx)          # no scene
        assert irr(desc()) == RT_ERR_NOT_READY
        # a scene without draw commands, as a caller of rt_upload_bvh alone leaves it
        r.loadTexturesFromWorld(b)
        r.updateCombinedGeometry(b.vertices, b.normals, b.uvs)
        r.updateCombinedBVH(b.tlas, b.blas)
        r.updateBuffer("topology", b.mesh_topology)
        r.updateBuffer("instance", b.instances)
        r.updateBuffer("lights", b.lights)
        b.updateCamera(16, 16)
        r.updateSceneUniforms(b.cameraData, 0, b.lightCount)
        assert bake(desc()) == RT_ERR_NOT_READY and b"draw command" in r.L.rt_last_error(r.ctx)
        assert irr(desc()) == RT_ERR_NOT_READY
        r.updateBuffer("draw_commands", b.draw_commands)
        assert bake(desc()) == 0 and n.value == 64
        assert irr(desc()) == 0
        for bad in (None, desc(width=0), desc(height=0), desc(width=4097, height=4096), desc(width=1 << 24, height=2),
                    desc(pad_base=(1 << 31) - 63), desc(inst=1), desc(reserved=1)):
            assert bake(bad) == RT_ERR_INVALID, bad
            assert irr(bad) == RT_ERR_INVALID, bad
        assert bake(desc(pad_base=(1 << 31) - 64)) == 0                                 # pad_base + W * H == 2^31 is allowed
        assert bake(desc(width=4096, height=4096), cap=0, p=None, t=None) == 0 and n.value == 4096 * 4096   # 2^24 texels
        assert bake(desc(), p=None) == RT_ERR_INVALID
        assert bake(desc(), t=None) == RT_ERR_INVALID
        assert bake(desc(), count=None) == RT_ERR_INVALID
        assert bake(desc(), cap=0, p=None, t=None) == 0 and n.value == 64               # counts only
        assert bake(desc(), uv.ctypes.data, n_verts) == 0 and n.value == 0              # all uvs (0, 0): nothing covered
        assert bake(desc(), uv.ctypes.data, n_verts - 1) == RT_ERR_INVALID
        assert irr(desc(), out=None) == RT_ERR_INVALID
        assert irr(desc(), spp=0) == RT_ERR_INVALID and irr(desc(), spp=65537) == RT_ERR_INVALID
        r.updateSceneUniforms(b.cameraData, 0, len(np.asarray(b.lights)) // 2 + 1)       # a light count above the lights buffer
        assert irr(desc()) == RT_ERR_INVALID and b"light_count" in r.L.rt_last_error(r.ctx)
    finally:
        r.destroy()
