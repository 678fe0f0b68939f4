"""The plain form of the wide one-leaf path tracer (k_pathtrace_persistent_plain, csrc/k_pathtrace.hip.h).  When the host has
seen in the uploaded topology (csrc/scene_facts.h) nothing but untextured Lambertian triangles and lights, a batched dispatch
of a one-leaf scene runs the wide form compiled without the GGX and dielectric branches, the texture fetches and the emissive
length.  What is left is the generic form's arithmetic, so every image and every ray counter must equal the oracle's bit for
bit, and equal what the generic form gives when MI355RT_PLAIN_MATERIALS=0 switches the choice off; rt_debug_pt_form says
which form a dispatch took.

The one way this can go wrong silently is a fact that outlives the records it was read from.  One renderer is therefore taken
through uploads that change the answer and a device-resident world update the host cannot see, against an oracle given the
same sequence, and single triangles that break each clause of the condition are traced against the oracle too."""
import numpy as np
import pytest

import parity_util as pu
from test_gpu_product_build import RAYS, _run
from test_gpu_world_records import _both, _same_images, _scene, _trace

pytestmark = pytest.mark.gpu

FRAMES = (1, 2, 3, 4)


class _Retopologised:
    """The bridge `b` with another topology array."""
    def __init__(self, b, topo):
        self._b = b
        self.mesh_topology = topo

    def __getattr__(self, name):
        return getattr(self._b, name)


def _topology(b):
    return np.array(b.mesh_topology, np.uint32).reshape(-1, 20).copy()


def _cornell_with(W, word, value, tri):
    """Cornell with word `word` of triangle `tri`'s topology record set to the f32 `value`."""
    b = pu.bridge_for(W, "cornell")
    topo = _topology(b)
    topo.view(np.float32)[tri, word] = value
    return _Retopologised(b, topo.reshape(-1))


_in_view = []


def _lambertian_in_view(W, oracle_lib):
    """The Lambertian triangle of Cornell that covers most pixels of the primary pass."""
    if _in_view:
        return _in_view[0]
    b = pu.bridge_for(W, "cornell")
    cpu = oracle_lib.OracleRenderer()
    pu.drive(cpu, W, b, 32, 24, 1, 1, (1,), present=False)
    _, normal_id, depth = cpu.readGBuffer()
    tri = pu.bits(normal_id).reshape(-1, 4)[:, 2][np.asarray(depth).reshape(-1) < 1.0]
    mat = _topology(b).view(np.float32)[:, 7]
    tri = tri[mat[tri] == 0.0]
    assert tri.size
    _in_view.append(int(np.bincount(tri).argmax()))
    return _in_view[0]


def _render(W, b, w, h, depth, spp, batch, stripes=None):
    r = W.WebGPURenderer(0)
    if stripes:
        r.setStripes(*stripes)
    _run(W, r, b, w, h, depth, spp, FRAMES, batch, 1)
    return r


def _check(r, cpu, form, h, stripes=None):
    """The renderer's last dispatch took `form` in 512-thread workgroups, and its image and ray counters are the oracle's."""
    assert r.debugPtForm() == form
    assert r.debugPtLaunch()["threads"] == 512
    got, want = r.readAccum(), cpu.readAccum()
    if stripes:
        rows, rank, count = stripes
        owned = (np.arange(h) // rows) % count == rank
        assert not got[~owned].any(), "rank %d wrote outside its rows" % rank
        got, want = got[owned], want[owned]
    assert np.array_equal(pu.bits(got), pu.bits(want)), pu.describe_mismatch("accumulation buffer (%s form)" % form, got, want)
    gc, cc = r.getCounters(), cpu.getCounters()
    assert {k: gc[k] for k in RAYS} == {k: cc[k] for k in RAYS}, form
    return r.readAccum()


def _both_forms(W, oracle_lib, monkeypatch, b, w, h, depth, spp, batch, stripes=None, form="plain"):
    """`b` through a context with the choice on (which must take `form`) and one created with the knob off (generic)."""
    cpu = oracle_lib.OracleRenderer()
    if stripes:
        cpu.setStripes(*stripes)
    pu.drive(cpu, W, b, w, h, depth, spp, FRAMES, present=False)
    W._build.build_rt()
    images = []
    for knob, want_form in ((None, form), ("0", "generic")):
        if knob is not None:
            monkeypatch.setenv("MI355RT_PLAIN_MATERIALS", knob)
        r = _render(W, b, w, h, depth, spp, batch, stripes)
        try:
            images.append(_check(r, cpu, want_form, h, stripes))
        finally:
            r.destroy()
    assert np.array_equal(pu.bits(images[0]), pu.bits(images[1]))


# every size with two depths, both sample counts and both batch sizes; 5 x 3 and 8 x 8 are one tile, 37 x 29 twenty
CASES = [(8, 8, 8, 1, 2), (8, 8, 1, 3, 4), (5, 3, 8, 3, 2), (5, 3, 2, 1, 4), (9, 9, 2, 3, 2), (9, 9, 8, 1, 4),
         (37, 29, 8, 1, 4), (37, 29, 8, 3, 2), (37, 29, 1, 1, 2), (37, 29, 2, 3, 4)]


@pytest.mark.parametrize("w,h,depth,spp,batch", CASES)
def test_cornell_plain_form_equals_the_oracle_and_the_generic_form(W, oracle_lib, monkeypatch, w, h, depth, spp, batch):
    _both_forms(W, oracle_lib, monkeypatch, pu.bridge_for(W, "cornell"), w, h, depth, spp, batch)


def test_cornell_plain_form_on_a_striped_rank(W, oracle_lib, monkeypatch):
    _both_forms(W, oracle_lib, monkeypatch, pu.bridge_for(W, "cornell"), 21, 67, 8, 1, 2, stripes=(8, 1, 3))


def test_knob_on_is_the_default(W, oracle_lib, monkeypatch):
    monkeypatch.setenv("MI355RT_PLAIN_MATERIALS", "1")
    b = pu.bridge_for(W, "cornell")
    cpu = oracle_lib.OracleRenderer()
    pu.drive(cpu, W, b, 9, 9, 8, 1, FRAMES, present=False)
    r = _render(W, b, 9, 9, 8, 1, 4)
    try:
        assert r.debugPtForm() == "plain"
        # a single frame keeps the 256-thread form, which has no plain twin
        r.compute(5)
        cpu.compute(5)
        r.sync()
        assert r.debugPtForm() == "generic" and r.debugPtLaunch()["threads"] == 256
        assert np.array_equal(pu.bits(r.readAccum()), pu.bits(cpu.readAccum()))
    finally:
        r.destroy()


# word of the topology record, value, the form the dispatch must take
ODD_TRIANGLES = [
    (7, 1.0, "generic"),            # metal
    (7, 2.0, "generic"),            # dielectric
    (7, float("nan"), "plain"),     # the kernel's decode saturates a NaN word to 0: Lambertian
    (12, 0.0, "generic"),           # base-colour texture
    (13, 0.0, "generic"),           # metallic-roughness texture
    (14, 0.0, "generic"),           # normal map
    (15, 0.0, "generic"),           # emissive texture
    (12, float("nan"), "plain"),    # NaN > -0.5 is false: no texture
    (16, 0.5, "generic"),           # emission on a Lambertian triangle
]


@pytest.mark.parametrize("word,value,form", ODD_TRIANGLES)
def test_one_odd_triangle(W, oracle_lib, monkeypatch, word, value, form):
    tri = _lambertian_in_view(W, oracle_lib)
    _both_forms(W, oracle_lib, monkeypatch, _cornell_with(W, word, value, tri), 24, 16, 8, 1, 4, form=form)


def test_emission_on_a_light_stays_plain(W, oracle_lib, monkeypatch):
    b = pu.bridge_for(W, "cornell")
    light = int(np.flatnonzero(_topology(b).view(np.float32)[:, 7] == 3.0)[0])
    _both_forms(W, oracle_lib, monkeypatch, _cornell_with(W, 16, 0.5, light), 24, 16, 8, 1, 4, form="plain")


@pytest.mark.parametrize("scene", ["special", "textured_lights"])
def test_other_scenes_run_the_generic_form(W, oracle_lib, gpu_renderer, scene):
    """`special` has 528 light triangles (more than a one-leaf LDS scene can hold: not scanned); the textured instance is a
    one-leaf scene of every material with textures on its lights, which takes the wide form."""
    b = pu.bridge_for(W, "special") if scene == "special" else _scene(W, "textured_lights")
    w, h = 24, 16
    cpu = oracle_lib.OracleRenderer()
    pu.drive(cpu, W, b, w, h, 8, 1, FRAMES, present=False)
    _run(W, gpu_renderer, b, w, h, 8, 1, FRAMES, 4, 1)
    assert gpu_renderer.debugPtForm() == "generic"
    assert gpu_renderer.debugPtLaunch()["threads"] == (512 if scene == "textured_lights" else 256)
    got, want = gpu_renderer.readAccum(), cpu.readAccum()
    assert np.array_equal(pu.bits(got), pu.bits(want)), pu.describe_mismatch("accumulation buffer", got, want)
    gc, cc = gpu_renderer.getCounters(), cpu.getCounters()
    assert {k: gc[k] for k in RAYS} == {k: cc[k] for k in RAYS}


def test_no_dispatch_and_other_kernels_report_none(W, gpu_renderer):
    r = gpu_renderer
    assert r.debugPtForm() == "none"
    _run(W, r, pu.bridge_for(W, "cornell"), 9, 9, 8, 1, (1, 2), 2, 2, 0)   # the wavefront form
    assert r.debugPtForm() == "none"


def test_the_facts_follow_the_scene(W, oracle_lib, gpu_renderer):
    """Cornell (plain), its topology again with one metal triangle (generic), the first topology again (plain), then a
    device-resident world update, whose records the host never sees (generic): one renderer, one oracle, the same sequence."""
    w, h, depth, batch = 40, 30, 8, 4
    b = pu.bridge_for(W, "cornell")
    metal = _cornell_with(W, 7, 1.0, _lambertian_in_view(W, oracle_lib))
    gpu, cpu = gpu_renderer, oracle_lib.OracleRenderer()
    gpu.setKernelVariant(1)
    for r in (gpu, cpu):
        r.buildPipeline(depth, 1)
        W.upload_scene(r, b, w, h)
    gpu.setCounting(False)
    _both(gpu, cpu, lambda r: r.resetCounters())

    def trace(form, what):
        _both(gpu, cpu, lambda r: _trace(r, FRAMES, batch))
        assert gpu.debugPtForm() == form, what
        assert gpu.debugPtLaunch()["threads"] == 512, what
        _same_images(gpu, cpu, what)

    def upload_topology(topo):
        _both(gpu, cpu, lambda r: (r.updateBuffer("topology", topo), r.recreateBindGroup(), r.resetAccumulation()))

    trace("plain", "cornell")
    upload_topology(metal.mesh_topology)
    trace("generic", "one metal triangle")
    upload_topology(b.mesh_topology)
    trace("plain", "cornell again")

    dev_b, host_b = W.WorldBridge(), W.WorldBridge()
    dev_b.setDeviceUpdater(gpu)
    dev_b.loadScene("cornell")
    host_b.loadScene("cornell")
    dev_b.update(0.25)
    host_b.update(0.25)
    assert dev_b.deviceResident, dev_b.deviceWarning
    assert len(gpu.worldRead("tlas")) // 8 == 1, "not a one-leaf world"
    W.upload_scene(cpu, host_b, w, h)   # the host path's arrays for the oracle; the renderer already holds its own
    dev_b.updateCamera(w, h)
    gpu.updateSceneUniforms(dev_b.cameraData, 0, dev_b.lightCount)
    gpu.resetAccumulation()
    trace("generic", "after the device world update")
