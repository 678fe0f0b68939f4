"""Atlas bakes on the GPU (rt_bake_atlas_points / rt_bake_atlas_points_device / rt_bake_atlas_irradiance, the k_atlas_* kernels
of csrc/k_bake.hip.h) against the two identities of include/mi355rt.h: (A) one whole-atlas entry is rt_bake_points, on the
GPU's own; (B) any atlas bake is the composition of its entries' single-instance bakes (atlas_bake_util.compose on the
reference model of tests/model/bake_model.cpp, held to paper by tests/test_atlas_bake_model.py) - points, texel indices, count
and the two-channel owner map word for word.  Then the work list (many entries; chunks and bands), an entry that covers
nothing, independence of scheduling and of cap, the whole bake as the GPU's own points + gather + scatter, the device entry on
a torch side stream, the device-resident animated world, no side effect on a render, and the error returns.

Parity must not pass on emptiness: the covered share, the contested texels and the owning entries are asserted on the MODEL
before the GPU is asked."""
import ctypes

import numpy as np
import pytest

import atlas_bake_util as au
import bake_util as bu
import gather_util as gu
import parity_util as pu
import test_gpu_bake as tb

pytestmark = pytest.mark.gpu

RT_ERR_INVALID, RT_ERR_NOT_READY = -1, -3
NONE4 = np.array([0, 0, 0, -1], np.float32).view(np.uint32)
_small = {}


def small_case(W, scene, layout):
    """(bridge, entries, override layout, composition of the model) of the small composition case, made once"""
    key = (scene, layout)
    if key not in _small:
        b, m = tb._scene(W, scene)
        entries = au.small_entries(au.instance_count(b))
        uv = au.merged_grid_uv(b, [e[0] for e in entries], bleed=(layout == "bleed"))
        want = au.compose(m, entries, au.SMALL_W, au.SMALL_H, t_max=5.0, pad_base=1000, atlas_uv=uv)
        _small[key] = (b, entries, uv, want)
    return _small[key]


def owners_of(want):
    """texels owned per entry, from a composed owner map"""
    e = want[2][:, :, 0]
    return np.bincount(e[e >= 0], minlength=1)


@pytest.mark.parametrize("size", ((1, 1), (7, 5), (65, 63)))
def test_one_whole_atlas_entry_is_bake_points(W, size):
    """identity (A), on the GPU's own bakePoints: instanced1000, instance 0, the scene's uvs"""
    b, m = tb._scene(W, "instanced1000")
    width, height = size
    r = tb._renderer(W, b)
    try:
        points, texels, owner = r.bakePoints(0, width, height, t_max=5.0, pad_base=1000, owner=True)
        assert len(texels) > 0.1 * width * height
        ap, at, ao = r.bakeAtlasPoints([(0, 0, 0, width, height)], width, height, t_max=5.0, pad_base=1000, owner=True)
        assert np.array_equal(at, texels) and np.array_equal(pu.bits(ap), pu.bits(points))
        assert ao.shape == (height, width, 2)
        assert np.array_equal(ao[:, :, 1], owner)
        assert np.array_equal(ao[:, :, 0], np.where(owner >= 0, 0, -1))
    finally:
        r.destroy()


@pytest.mark.parametrize("layout", ("grid", "bleed"))
@pytest.mark.parametrize("scene", ("instanced1000", "random1", "random2", "special", "cornell"))
def test_composition_small(W, scene, layout):
    b, entries, uv, want = small_case(W, scene, layout)
    share = len(want[1]) / (au.SMALL_W * au.SMALL_H)
    per_entry = owners_of(want)
    print(scene, layout, "covered share %.2f" % share, "contested", want[3], "texels per entry", per_entry.tolist())
    assert share > 0.1 and want[3] >= 5
    assert len(per_entry) >= 4 and (per_entry[0:4] > 0).all()
    r = tb._renderer(W, b)
    try:
        got = r.bakeAtlasPoints(entries, au.SMALL_W, au.SMALL_H, t_max=5.0, pad_base=1000, atlas_uv=uv, owner=True)
        au.check_atlas_points(got, want, "%s %s" % (scene, layout))
    finally:
        r.destroy()


def test_many_entries_and_the_work_list(W):
    """256 entries of 20 x 12 texels over the four geometries of instanced1000: one entry per thread of the item pass, a
    prefix array of 257, waves that find their entry by binary search"""
    b, m = tb._scene(W, "instanced1000")
    entries = [(e, (e % 16) * 20, (e // 16) * 12, 20, 12) for e in range(256)]
    uv = au.merged_grid_uv(b, (0, 1, 2, 4))
    want = au.compose(m, entries, 320, 192, atlas_uv=uv)
    per_entry = owners_of(want)
    share = len(want[1]) / (320 * 192)
    print("covered share %.3f" % share, "texels per entry %d .. %d" % (per_entry.min(), per_entry.max()))
    assert share > 0.1 and len(per_entry) == 256 and per_entry.min() > 0
    r = tb._renderer(W, b)
    try:
        au.check_atlas_points(r.bakeAtlasPoints(entries, 320, 192, atlas_uv=uv, owner=True), want, "256 entries")
    finally:
        r.destroy()


def test_chunks_and_bands(W):
    """special: one instance of 564 triangles = 9 chunks of 64; rectangles three bands tall that start off the band grid"""
    b, m = tb._scene(W, "special")
    first, count = bu.instance_triangles(b, 0)
    assert count > 8 * 64
    entries = [(0, 3, 5, 40, 70), (0, 43, 0, 21, 75)]
    uv = bu.grid_uv(b, 0)
    want = au.compose(m, entries, 64, 75, atlas_uv=uv)
    tris = want[2][:, :, 1]
    share = len(want[1]) / (64 * 75)
    print("covered share %.2f" % share, "distinct owner triangles", len(np.unique(tris[tris >= 0])), "highest", tris.max())
    assert share > 0.1 and tris.max() >= first + 8 * 64
    r = tb._renderer(W, b)
    try:
        au.check_atlas_points(r.bakeAtlasPoints(entries, 64, 75, atlas_uv=uv, owner=True), want, "special")
    finally:
        r.destroy()


def test_an_entry_that_covers_nothing(W):
    """instance 0 carries the hand-worked quad, every vertex of the other geometries lies at (-1, -1): the middle entry has
    no texel, its neighbours have theirs.  Then a bake in which no entry covers anything."""
    b, m = tb._scene(W, "instanced1000")
    assert bu.instance_triangles(b, 0) != bu.instance_triangles(b, 1)
    uv = bu.hand_uv(b, 0, bu.QUAD)
    entries = [(0, 0, 0, 8, 8), (1, 6, 2, 9, 9), (0, 13, 4, 8, 8)]
    want = au.compose(m, entries, 24, 13, atlas_uv=uv)
    assert owners_of(want).tolist() == [64, 0, 64]
    r = tb._renderer(W, b)
    try:
        au.check_atlas_points(r.bakeAtlasPoints(entries, 24, 13, atlas_uv=uv, owner=True), want, "empty entry")
        none = np.full_like(uv, -1.0)
        points, texels, owner = r.bakeAtlasPoints(entries, 24, 13, atlas_uv=none, owner=True)
        assert len(points) == 0 and len(texels) == 0 and (owner == -1).all()
        atlas, n, st = r.bakeAtlasIrradiance(entries, 24, 13, 4, 8, bu.SEED, atlas_uv=none, stats=True)
        assert n == 0 and atlas.shape == (13, 24)
        assert np.array_equal(atlas.view(np.uint32).reshape(-1, 4), np.tile(NONE4, (24 * 13, 1)))
        assert all(st[k] == 0 for k in st), st
        # ... and an ordinary one on the same context
        au.check_atlas_points(r.bakeAtlasPoints(entries, 24, 13, atlas_uv=uv, owner=True), want, "after the empty bake")
    finally:
        r.destroy()


def test_scheduling_independence_and_cap(W):
    b, entries, uv, want = small_case(W, "random2", "grid")
    r = tb._renderer(W, b)
    try:
        args = dict(t_max=5.0, pad_base=1000, atlas_uv=uv)
        full = r.bakeAtlasPoints(entries, au.SMALL_W, au.SMALL_H, owner=True, **args)
        again = r.bakeAtlasPoints(entries, au.SMALL_W, au.SMALL_H, owner=True, **args)
        for a, c in zip(full, again):
            assert np.array_equal(pu.bits(a), pu.bits(c))
        n = len(full[1])
        assert n == len(want[1]) and n > 258
        for cap in (n - 1, 257, 1, 0, n + 100):
            p, t, count = r.bakeAtlasPoints(entries, au.SMALL_W, au.SMALL_H, cap=cap, **args)
            assert count == n and len(t) == min(cap, n)
            assert np.array_equal(t, full[1][:cap]) and np.array_equal(pu.bits(p), pu.bits(full[0][:cap]))
    finally:
        r.destroy()


@pytest.mark.parametrize("depth,spp", [(4, 8), (0, 4)])
@pytest.mark.parametrize("scene", ("cornell", "random1"))
def test_a_bake_is_points_then_gather_then_scatter(W, scene, depth, spp):
    from webgpu_raytracer_amd import renderer as R
    b, entries, uv, want = small_case(W, scene, "grid")
    width, height = au.SMALL_W, au.SMALL_H
    r = tb._renderer(W, b)
    try:
        points, texels = r.bakeAtlasPoints(entries, width, height, t_max=5.0, pad_base=1000, atlas_uv=uv)
        res, gst = r.gatherIrradiance(points, depth, spp, bu.SEED, stats=True)
        atlas, n, st = r.bakeAtlasIrradiance(entries, width, height, depth, spp, bu.SEED, t_max=5.0, pad_base=1000, atlas_uv=uv,
                                             stats=True)
        assert atlas.shape == (height, width) and atlas.dtype == R.IRRADIANCE_DTYPE
        words = atlas.view(np.uint32).reshape(-1, 4)
        assert n == len(texels) == len(want[1]) and n > 0.1 * width * height
        assert np.array_equal(words[texels], gu.result_words(res))
        none = np.ones(width * height, bool)
        none[texels] = False
        assert none.any() and np.array_equal(words[none], np.tile(NONE4, (none.sum(), 1)))
        for k in gst:
            if k != "kernel_ms":
                assert st[k] == gst[k], (k, st[k], gst[k])
        plain = r.bakeAtlasIrradiance(entries, width, height, depth, spp, bu.SEED, t_max=5.0, pad_base=1000, atlas_uv=uv)
        assert np.array_equal(plain.view(np.uint32), atlas.view(np.uint32))
    finally:
        r.destroy()


def test_device_entry_on_a_torch_side_stream(W):
    import torch
    from webgpu_raytracer_amd import renderer as R
    b, entries, uv, want = small_case(W, "instanced1000", "grid")
    width, height = au.SMALL_W, au.SMALL_H
    n = len(want[1])
    r = tb._renderer(W, b)
    try:
        r.buildPipeline(4, 1)
        side = torch.cuda.Stream()
        r.setStream(side.cuda_stream)
        d = R.RtBakeAtlasDesc(width, height, 1000, 5.0, len(entries))
        rects = np.zeros((len(entries), 8), np.uint32)
        rects[:, 0:5] = entries
        with torch.cuda.stream(side):
            d_uv = torch.from_numpy(uv).to("cuda", non_blocking=False)
            d_points = torch.zeros((width * height, 8), dtype=torch.float32, device="cuda")
            d_texels = torch.zeros(width * height, dtype=torch.int32, device="cuda")
            d_count = torch.zeros(4, dtype=torch.int32, device="cuda")
            d_owner = torch.zeros(width * height, dtype=torch.int64, device="cuda")
            # a bake and a frame queued back to back: nothing here waits for the GPU
            rc = r.L.rt_bake_atlas_points_device(r.ctx, ctypes.addressof(d), rects.ctypes.data, d_uv.data_ptr(), d_points.data_ptr(),
                                                 d_texels.data_ptr(), width * height, d_count.data_ptr(), d_owner.data_ptr())
            rects[:] = 0xffffffff                      # the library has copied the entries: the caller's array is free
            assert rc == 0, r.L.rt_last_error(r.ctx)
            r.compute(1)
            covered = (d_owner >= 0).sum()            # a torch op on the same stream, behind the bake
        side.synchronize()
        assert int(d_count[0]) == n == int(covered)
        o = d_owner.cpu().numpy()                      # (entry << 32) | triangle, -1 for none
        owner = np.stack([(o >> 32).astype(np.int32), (o & 0xffffffff).astype(np.uint32).view(np.int32)], axis=1)
        got = (d_points.cpu().numpy()[:n], d_texels.cpu().numpy()[:n].view(np.uint32), owner.reshape(height, width, 2))
        au.check_atlas_points(got, want, "device entry")
        rects[:, 0:5] = entries
        call = r.L.rt_bake_atlas_points_device
        assert call(r.ctx, ctypes.addressof(d), rects.ctypes.data, None, d_points.data_ptr() + 8, d_texels.data_ptr(), 16,
                    d_count.data_ptr(), None) == RT_ERR_INVALID   # misaligned
        assert call(r.ctx, ctypes.addressof(d), rects.ctypes.data, None, d_points.data_ptr(), d_texels.data_ptr(), 16, None,
                    None) == RT_ERR_INVALID
        # count only, through the binding: no arrays, no owner map
        with torch.cuda.stream(side):
            d_count.zero_()
            r.bakeAtlasPointsDevice(entries, width, height, None, None, 0, d_count.data_ptr(), t_max=5.0, pad_base=1000,
                                    atlas_uv_ptr=d_uv.data_ptr())
        side.synchronize()
        assert int(d_count[0]) == n
        r.setStream(None)
    finally:
        r.destroy()


def test_device_resident_animated_scene(W):
    """rt_world_update: the draw commands and the skinned vertices exist only on the device; the model gets them from
    rt_world_read.  Two overlapping entries of the skinned instance."""
    import test_gltf
    glb = test_gltf.big_skinned_glb(W, 48, 24)[0]
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    try:
        dev_b = W.WorldBridge()
        dev_b.setDeviceUpdater(r)
        dev_b.loadScene("viewer", glbData=glb)
        dev_b.update(0.4)
        assert dev_b.deviceResident, dev_b.deviceWarning
        a = tb._Arrays(r)
        m = bu.BakeModel()
        m.buildPipeline(4, 1)
        m.loadTexturesFromWorld(dev_b)
        m.updateCombinedGeometry(a.vertices, a.normals, a.uvs)
        m.updateCombinedBVH(a.tlas, a.blas)
        m.updateBuffer("topology", a.mesh_topology)
        m.updateBuffer("instance", a.instances)
        m.updateBuffer("lights", a.lights)
        m.updateBuffer("draw_commands", a.draw_commands)
        inst = int(np.argmax(np.asarray(a.draw_commands, np.uint32).reshape(-1, 4)[:, 0]))   # the skinned mesh
        uv = bu.grid_uv(a, inst)
        entries = [(inst, 0, 0, 40, 40), (inst, 29, 5, 35, 33)]
        want = au.compose(m, entries, 64, 40, atlas_uv=uv)
        print("covered share %.2f" % (len(want[1]) / (64 * 40)), "contested", want[3], owners_of(want).tolist())
        assert len(want[1]) > 0.1 * 64 * 40 and (owners_of(want) > 0).all() and want[3] > 0
        au.check_atlas_points(r.bakeAtlasPoints(entries, 64, 40, atlas_uv=uv, owner=True), want, "device world")
    finally:
        r.destroy()


def test_atlas_bakes_leave_the_render_alone(W):
    """Frames 1-4, atlas bakes, frames 5-8 with lookahead 8 against the same frames without a bake: accumulation, presented
    image, counters, G-buffer and uniforms are equal; the radiance query's last stats are what they were before."""
    b, entries, uv, want = small_case(W, "cornell", "grid")
    W._build.build_rt()
    rays = np.zeros((64, 8), np.float32)
    rays[:, 0:3] = np.asarray(b.cameraData, np.float32)[0:3]
    rays[:, 3] = 1e30
    rays[:, 4:7] = (0.01 * np.arange(64)[:, None] - 0.3) * np.array([1, 0.5, 0], np.float32) + np.array([0, 0, 1], np.float32)

    def bakes(r):
        r.traceRadiance(rays, 4, 2, 3, stats=True)
        before = r.radianceQueryStats()
        got = r.bakeAtlasPoints(entries, au.SMALL_W, au.SMALL_H, t_max=5.0, pad_base=1000, atlas_uv=uv, owner=True)
        au.check_atlas_points(got, want, "between frames")
        atlas, n, _ = r.bakeAtlasIrradiance(entries, au.SMALL_W, au.SMALL_H, 4, 4, bu.SEED, atlas_uv=uv, stats=True)
        assert n == len(want[1])
        after = r.radianceQueryStats()
        assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in before.items() if k != "kernel_ms"}

    got = tb._render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), bakes)
    ref = tb._render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), lambda r: None)
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), "accumulation"
    assert np.array_equal(got[1], ref[1]), "captureFrame"
    assert got[2] == ref[2], (got[2], ref[2])
    for a, w in zip(got[3], ref[3]):
        assert np.array_equal(pu.bits(a), pu.bits(w)), "G-buffer"
    assert np.array_equal(got[4], ref[4]), "uniforms"


def test_errors(W):
    from webgpu_raytracer_amd import renderer as R
    b, m = tb._scene(W, "cornell")
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    try:
        points = np.zeros((64, 8), np.float32)
        texels = np.zeros(64, np.uint32)
        atlas = np.zeros(64, R.IRRADIANCE_DTYPE)
        n = ctypes.c_uint32(0)
        n_verts = np.asarray(b.uvs).size // 2
        uv = np.zeros((n_verts, 2), np.float32)
        keep = []

        def desc(width=8, height=8, pad_base=0, n_entries=1, reserved=0):
            d = R.RtBakeAtlasDesc(width, height, pad_base, 1e30, n_entries)
            d.reserved[2] = reserved
            return d

        def rect(inst=0, x=0, y=0, w=8, h=8, reserved=0):
            q = R.RtBakeRect(inst, x, y, w, h)
            q.reserved[0] = reserved
            return q

        def addr(o):
            keep.append(o)
            return ctypes.addressof(o) if o is not None else None

        def bake(d, q, uv_ptr=None, n_uv=0, p=points.ctypes.data, t=texels.ctypes.data, cap=64, count=ctypes.addressof(n)):
            return r.L.rt_bake_atlas_points(r.ctx, addr(d), addr(q), uv_ptr, n_uv, p, t, cap, count, None)

        def irr(d, q, out=atlas.ctypes.data, spp=1):
            return r.L.rt_bake_atlas_irradiance(r.ctx, addr(d), addr(q), None, 0, 4, spp, 0, out, None, None)

        assert bake(desc(), rect()) == RT_ERR_NOT_READY and r.L.rt_last_error(r.ctx).startswith(b"bake atlas:")   # no scene
        assert irr(desc(), rect()) == RT_ERR_NOT_READY
        # a scene without draw commands, as a caller of rt_upload_bvh alone leaves it
        r.loadTexturesFromWorld(b)
        r.updateCombinedGeometry(b.vertices, b.normals, b.uvs)
        r.updateCombinedBVH(b.tlas, b.blas)
        r.updateBuffer("topology", b.mesh_topology)
        r.updateBuffer("instance", b.instances)
        r.updateBuffer("lights", b.lights)
        b.updateCamera(16, 16)
        r.updateSceneUniforms(b.cameraData, 0, b.lightCount)
        assert bake(desc(), rect()) == RT_ERR_NOT_READY and b"draw command" in r.L.rt_last_error(r.ctx)
        assert irr(desc(), rect()) == RT_ERR_NOT_READY
        r.updateBuffer("draw_commands", b.draw_commands)
        assert bake(desc(), rect()) == 0 and n.value == 64
        assert irr(desc(), rect()) == 0
        two = (R.RtBakeRect * 2)(rect(), rect(w=0))
        bad = [(None, rect()), (desc(), None), (desc(reserved=1), rect()), (desc(), rect(reserved=1)),
               (desc(n_entries=0), rect()), (desc(n_entries=65537), rect()),
               (desc(width=0), rect()), (desc(height=0), rect()), (desc(width=4097, height=4096), rect()),
               (desc(width=1 << 24, height=2), rect()), (desc(pad_base=(1 << 31) - 63), rect()),
               (desc(), rect(w=0)), (desc(), rect(h=0)), (desc(n_entries=2), two),
               (desc(), rect(x=1)), (desc(), rect(y=1)), (desc(), rect(w=9)), (desc(), rect(h=9)),
               (desc(), rect(x=0xfffffff0, w=32)), (desc(), rect(y=0xfffffff0, h=32)), (desc(), rect(x=8, w=1)),
               (desc(), rect(inst=1))]
        for d, q in bad:
            assert bake(d, q) == RT_ERR_INVALID, (d, q)
            assert r.L.rt_last_error(r.ctx).startswith(b"bake atlas:")
            assert irr(d, q) == RT_ERR_INVALID, (d, q)
        assert bake(desc(pad_base=(1 << 31) - 64), rect()) == 0                         # pad_base + W * H == 2^31 is allowed
        assert bake(desc(width=9, height=9), rect(x=1, y=1)) == 0 and n.value == 64     # a rectangle that ends at the edge
        assert bake(desc(), rect(), p=None) == RT_ERR_INVALID
        assert bake(desc(), rect(), t=None) == RT_ERR_INVALID
        assert bake(desc(), rect(), count=None) == RT_ERR_INVALID
        assert bake(desc(), rect(), cap=0, p=None, t=None) == 0 and n.value == 64       # counts only
        assert bake(desc(), rect(), uv.ctypes.data, n_verts) == 0 and n.value == 0      # all uvs (0, 0): nothing covered
        assert bake(desc(), rect(), uv.ctypes.data, n_verts - 1) == RT_ERR_INVALID
        assert irr(desc(), rect(), out=None) == RT_ERR_INVALID
        assert irr(desc(), rect(), spp=0) == RT_ERR_INVALID and irr(desc(), rect(), spp=65537) == RT_ERR_INVALID
    finally:
        r.destroy()
