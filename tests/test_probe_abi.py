"""Probe gathers (rt_gather_probes / rt_gather_probes_device / rt_probe_gather_stats), the parts that need no GPU: the three
symbols are declared, exported and bound; the record layouts are the documented 32 / 112 bytes with the slots of rt_ray; every
argument rule is refused with its code on a context-free call and - where a device is present - on a context without a scene;
the Node addon carries the binding."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_gather_abi import _fields

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_gather_probes", "rt_gather_probes_device", "rt_probe_gather_stats")
RT_ERR_INVALID, RT_ERR_NOT_READY = -1, -3


def test_symbols_are_declared_exported_and_bound(W):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mi355rt.h")).read(), flags=re.S)
    W._build.build_rt()
    lib = ctypes.CDLL(W._build.RT_LIB)
    from webgpu_raytracer_amd import renderer
    L = renderer.load_library()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert hasattr(lib, s), s
        assert s in renderer.EXPORTED_SYMBOLS
        assert getattr(L, s).argtypes is not None
    for m in ("gatherProbes", "gatherProbesDevice", "probeGatherStats"):
        assert callable(getattr(W.WebGPURenderer, m))
    assert callable(renderer.sh9_irradiance)
    assert re.search(r"#define\s+RT_PROBE_BATCH_SAMPLES\s+\(1u << 22\)", header)
    blob = open(W._build.RT_LIB, "rb").read()
    assert b"k_probe_rays" in blob and b"k_probe_project" in blob


def test_record_layouts(W):
    from webgpu_raytracer_amd import renderer as R
    P, S = R.PROBE_DTYPE, R.PROBE_SH9_DTYPE
    assert P.itemsize == 32 and S.itemsize == 112
    assert P.names == ("position", "t_max", "unused", "pad")
    assert [P.fields[k][1] for k in P.names] == [0, 12, 16, 28]
    assert S.names == ("sh", "hit_fraction") and S.fields["sh"][1] == 0 and S.fields["hit_fraction"][1] == 108
    assert S.fields["sh"][0].shape == (9, 3)
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    for name, size in (("rt_probe", 32), ("rt_probe_sh9", 112)):
        assert "static_assert(sizeof(%s) == %d" % (name, size) in layout
    # the probe has the slots of rt_ray, word for word
    assert _fields(layout, "rt_probe") == [("float", "position", 3), ("float", "t_max", None), ("float", "unused", 3),
                                           ("uint32_t", "pad", None)]
    assert [(t, n) for t, _, n in _fields(layout, "rt_probe")] == [(t, n) for t, _, n in _fields(layout, "rt_ray")]
    body = re.search(r"typedef struct rt_probe_sh9 \{(.*?)\} rt_probe_sh9;", layout, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.strip() for d in body.split(";") if d.strip()] == ["float sh[9][3]", "float hit_fraction"]


def test_calls_without_a_context_are_refused(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    probes = np.zeros((4, 8), np.float32)
    out = np.zeros(4, R.PROBE_SH9_DTYPE)
    st = R.RtRadianceStats()
    assert L.rt_gather_probes(None, probes.ctypes.data, 4, 4, 1, 0, out.ctypes.data, None) == RT_ERR_INVALID
    assert L.rt_gather_probes(None, probes.ctypes.data, 0, 4, 1, 0, out.ctypes.data, ctypes.addressof(st)) == RT_ERR_INVALID
    assert L.rt_gather_probes_device(None, probes.ctypes.data, 4, 4, 1, 0, out.ctypes.data) == RT_ERR_INVALID
    assert L.rt_probe_gather_stats(None, ctypes.addressof(st)) == RT_ERR_INVALID


def test_argument_rules_on_a_context_without_a_scene(W):
    """Every RT_ERR_INVALID and RT_ERR_NOT_READY rule of the entries, in the order the library checks them: the argument
    rules come before the scene, so a context without one shows them all.  Needs a device to make a context; without one the
    constructor's refusal is the result."""
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    if L.rt_device_count() == 0:
        with pytest.raises(W.RendererError):
            W.WebGPURenderer(0)
        return
    r = W.WebGPURenderer(0)
    try:
        probes = np.zeros((16, 8), np.float32)
        out = np.zeros(16, R.PROBE_SH9_DTYPE)
        st = R.RtRadianceStats()
        host, dev, stats = L.rt_gather_probes, L.rt_gather_probes_device, L.rt_probe_gather_stats
        p, o = probes.ctypes.data, out.ctypes.data

        def message():
            return L.rt_last_error(r.ctx)

        assert stats(r.ctx, ctypes.addressof(st)) == 0 and st.rays == 0 and st.workgroups == 0     # before any gather
        assert stats(r.ctx, None) == RT_ERR_INVALID
        for spp in (0, 65537):
            assert host(r.ctx, p, 16, 4, spp, 0, o, None) == RT_ERR_INVALID and message().startswith(b"probe gather:")
            assert dev(r.ctx, p, 16, 4, spp, 0, o) == RT_ERR_INVALID and b"spp" in message()
        assert host(r.ctx, p, 1 << 31, 4, 1, 0, o, None) == RT_ERR_INVALID and b"probes" in message()
        assert dev(r.ctx, p, 1 << 31, 4, 1, 0, o) == RT_ERR_INVALID
        # n == 0 is RT_OK, whatever the pointers, and reports empty stats
        assert host(r.ctx, None, 0, 4, 1, 0, None, ctypes.addressof(st)) == 0 and st.rays == 0 and st.samples == 0
        assert dev(r.ctx, None, 0, 4, 1, 0, None) == 0
        assert host(r.ctx, p, 0, 4, 0, 0, o, None) == RT_ERR_INVALID                               # ... but spp is still checked
        assert host(r.ctx, None, 16, 4, 1, 0, o, None) == RT_ERR_INVALID and message().startswith(b"probe gather: NULL")
        assert host(r.ctx, p, 16, 4, 1, 0, None, None) == RT_ERR_INVALID
        assert dev(r.ctx, None, 16, 4, 1, 0, o) == RT_ERR_INVALID and message().startswith(b"probe gather: NULL")
        assert dev(r.ctx, p, 16, 4, 1, 0, None) == RT_ERR_INVALID
        # no scene
        assert host(r.ctx, p, 16, 4, 1, 0, o, None) == RT_ERR_NOT_READY and message().startswith(b"probe gather: no scene")
        assert host(r.ctx, p, 16, 4, 65536, 0, o, ctypes.addressof(st)) == RT_ERR_NOT_READY
    finally:
        r.destroy()


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                    reason="node / node_api.h not present")
def test_node_addon_exports_the_binding(W):
    W._build.build_scene()
    W._build.build_tex()
    W._build.build_rt()
    path = W._build.build_node_addon(force=True)
    assert path and os.path.exists(path)
    node_dir = os.path.dirname(path)
    js = ("const m=require('%s/index.js');console.log(typeof m.native.rtGatherProbes,"
          "typeof m.WebGPURenderer.prototype.gatherProbes)" % node_dir)
    out = subprocess.run([shutil.which("node"), "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ["function"] * 2
    assert os.path.exists(os.path.join(node_dir, "gather_probes.js"))
    assert "gatherProbes(" in open(os.path.join(node_dir, "index.d.ts")).read()
