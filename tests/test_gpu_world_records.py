"""Per-triangle world records of one-leaf-TLAS scenes (k_prepare_world_tris, csrc/k_prepare_primary.hip.h).  For a scene
whose TLAS is one leaf the library computes once per upload what the persistent path tracer and the primary pass would
otherwise compute per hit from (instance, triangle) alone: the geometric normal, the area and unit normal light_pdf uses,
the world-space vertex normals; and the one-leaf forms of the path tracer read the picked light's emission, texture index
and texture coordinates from its shading record.  The records are made by the functions the kernels call per hit, so
every image stays bit-identical to the oracle's: product and counting build, batched dispatches (the 512-thread form) and
single frames (256 threads).

The one way this can go wrong silently is a record that outlives its inputs.  The last three tests change the scene of
ONE renderer (another instance transform, other vertices, a device-resident world update) after it has traced, and compare
with an oracle that was given the same sequence: they fail if an upload path does not mark the records dirty."""
import numpy as np
import pytest

import parity_util as pu
import random_scene
from test_gpu_one_leaf_occupancy import dyn_lds
from test_gpu_one_leaf_wide import COL_PARK, LDS_PER_CU, WAVE_QUEUE
from test_gpu_product_build import RAYS, _check as check_product

pytestmark = pytest.mark.gpu

W_, H_, DEPTH, FRAMES = 128, 96, 8, (1, 2, 3)


def _clone(b, **kw):
    d = {k: v for k, v in b.__dict__.items() if k not in ("hasNewData", "hasNewGeometry")}
    d.update(kw)
    return random_scene.Bridge(**d)


def _one_leaf(seed, tris, **kw):
    b = random_scene.make(seed, n_geoms=1, tris_per_geom=tris, n_instances=1, **kw)
    assert len(b.tlas) // 8 == 1 and len(b.instances) // 36 == 1, "not a one-leaf TLAS"
    return b


def _with_transform(b, m):
    """The one-instance scene `b` with the instance's forward matrix replaced by `m` (4x4, float64): instance row and
    the TLAS leaf's box, as random_scene.make lays them out."""
    m32 = m.astype(np.float32)
    inst = np.array(b.instances, np.float32).copy()
    inst[0:16] = m32.T.reshape(-1)
    inst[16:32] = np.linalg.inv(m32.astype(np.float64)).astype(np.float32).T.reshape(-1)
    root = np.asarray(b.blas, np.float32).reshape(-1, 8)[0]
    lo, hi = root[0:3], root[4:7]
    corners = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    wc = (corners @ m32.astype(np.float64).T)[:, :3]
    tlas = np.array(b.tlas, np.float32).copy()
    tlas[0:3] = wc.min(axis=0) - 1e-3
    tlas[4:7] = wc.max(axis=0) + 1e-3
    return _clone(b, instances=inst, tlas=tlas)


def _rotated_scaled(b, seed):
    """A rotation times a strongly non-uniform scale: the transposed inverse that takes normals to world space is then
    far from the forward matrix that takes the light's vertices there."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    m = np.eye(4)
    m[:3, :3] = q @ np.diag([0.7, 2.0, 1.4])
    m[:3, 3] = [rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), -1.2]     # towards the camera: a fifth of the image
    return _with_transform(b, m)


def _zero_area_triangles(b):
    v = np.asarray(b.vertices, np.float32).reshape(-1, 4)[:, :3]
    idx = np.asarray(b.mesh_topology, np.uint32).reshape(-1, 20)[:, :3]
    cr = np.cross(v[idx[:, 1]] - v[idx[:, 0]], v[idx[:, 2]] - v[idx[:, 0]])
    return int((np.abs(cr).sum(axis=1) == 0).sum())


def _textured_lights(seed, tris):
    """Every light triangle carries a base-colour texture (what sample_light multiplies the emission with) and an
    emissive texture; a third of the other triangles keep the random texture indices of random_scene."""
    b = _one_leaf(seed, tris, with_textures=True)
    topo = np.array(b.mesh_topology, np.uint32).reshape(-1, 20).copy()
    f = topo.view(np.float32)
    lights = f[:, 7] == 3.0
    assert lights.any()
    f[lights, 12] = 0.0
    f[lights, 15] = 1.0
    return _clone(b, mesh_topology=topo.reshape(-1))


def _scene(W, name):
    if name == "cornell":
        b = pu.bridge_for(W, "cornell")
        assert len(b.tlas) // 8 == 1
        return b
    if name == "rotated":
        return _rotated_scaled(_one_leaf(1, 30), 7)
    if name == "textured_lights":
        return _rotated_scaled(_textured_lights(3, 30), 8)
    if name == "zero_area":
        b = _rotated_scaled(_one_leaf(2, 40), 9)
        assert _zero_area_triangles(b) >= 1
        return b
    raise KeyError(name)


def _trace(r, frames, batch):
    for i in range(0, len(frames), batch):
        if batch == 1 or not hasattr(r, "computeBatch"):
            for f in frames[i:i + batch]:
                r.compute(f)
        else:
            r.computeBatch(list(frames[i:i + batch]))
    r.sync()


def _same_images(gpu, cpu, what):
    ga, ca = gpu.readAccum(), cpu.readAccum()
    assert np.array_equal(pu.bits(ga), pu.bits(ca)), pu.describe_mismatch("accumulation buffer, " + what, ga, ca)
    for name, g, c in zip(("albedo", "normal_id", "depth"), gpu.readGBuffer(), cpu.readGBuffer()):
        assert np.array_equal(pu.bits(g), pu.bits(c)), pu.describe_mismatch("G-buffer %s, %s" % (name, what), g, c)
    gc, cc = gpu.getCounters(), cpu.getCounters()
    assert {k: gc[k] for k in RAYS} == {k: cc[k] for k in RAYS}, what


@pytest.mark.parametrize("mode", ["product_batched", "product_single", "counting"])
@pytest.mark.parametrize("scene", ["cornell", "rotated", "textured_lights", "zero_area"])
def test_one_leaf_scenes_equal_the_oracle(W, oracle_lib, gpu_renderer, scene, mode):
    b = _scene(W, scene)
    cpu = oracle_lib.OracleRenderer()
    pu.drive(cpu, W, b, W_, H_, DEPTH, 1, FRAMES, present=False)
    r = gpu_renderer
    r.setKernelVariant(1)          # the persistent kernel
    if mode == "counting":
        pu.drive(r, W, b, W_, H_, DEPTH, 1, FRAMES, present=False, detailed=True)
        pu.assert_parity(r, cpu, check_output=False)
        return
    r.buildPipeline(DEPTH, 1)
    W.upload_scene(r, b, W_, H_)
    r.setCounting(False)
    r.resetCounters()
    batch = 3 if mode == "product_batched" else 1
    _trace(r, FRAMES, batch)
    # the wide form where three workgroups of it fit the CU's LDS (tests/test_gpu_one_leaf_wide.py), else 256 threads
    wide = batch > 1 and dyn_lds(b) + 4 * WAVE_QUEUE + 8 * COL_PARK <= LDS_PER_CU // 3
    L = r.debugPtLaunch()
    assert L["threads"] == (512 if wide else 256), L
    assert scene == "zero_area" or wide == (batch > 1), "the scene was meant to take the wide form"
    check_product(r, cpu)


def _both(gpu, cpu, fn):
    for r in (gpu, cpu):
        fn(r)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("what", ["instance", "vertices"])
def test_records_follow_a_second_upload(W, oracle_lib, gpu_renderer, what, batch):
    """Trace, upload the instance again with another transform (or the vertices again, every triangle shrunk towards its
    centroid: half the edges, a quarter of the area), trace again."""
    b1 = _rotated_scaled(_one_leaf(1, 30), 7)
    gpu, cpu = gpu_renderer, oracle_lib.OracleRenderer()
    gpu.setKernelVariant(1)
    for r in (gpu, cpu):
        r.buildPipeline(DEPTH, 1)
        W.upload_scene(r, b1, W_, H_)
    gpu.setCounting(False)
    _both(gpu, cpu, lambda r: r.resetCounters())
    _both(gpu, cpu, lambda r: _trace(r, FRAMES, batch))
    _same_images(gpu, cpu, "first upload")
    first = gpu.readAccum().copy()
    if what == "instance":
        b2 = _rotated_scaled(b1, 11)
        _both(gpu, cpu, lambda r: (r.updateCombinedBVH(b2.tlas, b2.blas), r.updateBuffer("instance", b2.instances)))
    else:
        v = np.array(b1.vertices, np.float32).reshape(-1, 3, 4).copy()
        c = v[:, :, :3].mean(axis=1, keepdims=True)
        v[:, :, :3] = (c + np.float32(0.5) * (v[:, :, :3] - c)).astype(np.float32)
        b2 = _clone(b1, vertices=v.reshape(-1))
        _both(gpu, cpu, lambda r: r.updateCombinedGeometry(b2.vertices, b2.normals, b2.uvs))
    _both(gpu, cpu, lambda r: (r.recreateBindGroup(), r.resetAccumulation()))
    _both(gpu, cpu, lambda r: _trace(r, FRAMES, batch))
    _same_images(gpu, cpu, "second upload (%s)" % what)
    assert not np.array_equal(first, gpu.readAccum()), "the second upload did not change the picture"


@pytest.mark.parametrize("batch", [1, 3])
def test_records_follow_a_device_world_update(W, oracle_lib, gpu_renderer, batch):
    """A renderer that has traced a random one-leaf scene takes a device-resident World::update of another one-instance
    world (rt_world_update writes straight into the scene buffers); the oracle gets the arrays the host path of the same
    update makes."""
    b1 = _rotated_scaled(_one_leaf(1, 30), 7)
    gpu, cpu = gpu_renderer, oracle_lib.OracleRenderer()
    gpu.setKernelVariant(1)
    for r in (gpu, cpu):
        r.buildPipeline(DEPTH, 1)
        W.upload_scene(r, b1, W_, H_)
    gpu.setCounting(False)
    _both(gpu, cpu, lambda r: r.resetCounters())
    _both(gpu, cpu, lambda r: _trace(r, FRAMES, batch))
    _same_images(gpu, cpu, "uploaded scene")
    dev_b, host_b = W.WorldBridge(), W.WorldBridge()
    dev_b.setDeviceUpdater(gpu)
    dev_b.loadScene("cornell")
    host_b.loadScene("cornell")
    dev_b.update(0.25)
    host_b.update(0.25)
    assert dev_b.deviceResident, dev_b.deviceWarning
    assert len(gpu.worldRead("tlas")) // 8 == 1 and len(host_b.tlas) // 8 == 1, "not a one-leaf world"
    # the host path's upload for the oracle; the renderer already holds the arrays, as sync_world leaves it
    W.upload_scene(cpu, host_b, W_, H_)
    dev_b.updateCamera(W_, H_)
    gpu.updateSceneUniforms(dev_b.cameraData, 0, dev_b.lightCount)
    gpu.resetAccumulation()
    _both(gpu, cpu, lambda r: _trace(r, FRAMES, batch))
    _same_images(gpu, cpu, "after the world update")
