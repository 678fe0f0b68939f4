"""Directional gathers and bakes (rt_gather_directional / _device / rt_directional_gather_stats, rt_bake_atlas_directional /
_lightmap), the parts that need no GPU: the five symbols are declared, exported and bound; the result record is the documented
64 bytes, four rows in the shape of an rt_irradiance; every argument rule is refused with its code on a context-free call and
- where a device is present - on a context without a scene; the Node addon carries the bindings."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_gather_directional", "rt_gather_directional_device", "rt_directional_gather_stats", "rt_bake_atlas_directional",
           "rt_bake_atlas_directional_lightmap")
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
    for m in ("gatherDirectional", "gatherDirectionalDevice", "directionalGatherStats", "bakeAtlasDirectional",
              "bakeAtlasDirectionalLightmap"):
        assert callable(getattr(W.WebGPURenderer, m))
    assert callable(renderer.sh4_irradiance)
    assert re.search(r"#define\s+RT_DIRECTIONAL_BATCH_SAMPLES\s+\(1u << 22\)", header)
    blob = open(W._build.RT_LIB, "rb").read()
    assert b"k_dir_rays" in blob and b"k_dir_project" in blob and b"k_dir_scatter" in blob


def test_record_layout(W):
    from webgpu_raytracer_amd import renderer as R
    D = R.DIRECTIONAL_DTYPE
    assert D.itemsize == 64 and D.names == ("layer",) and D.fields["layer"][0].shape == (4, 4) and D.fields["layer"][1] == 0
    assert R.IRRADIANCE_DTYPE.itemsize * 4 == D.itemsize           # a row is a texel of an atlas layer
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    assert "static_assert(sizeof(rt_directional) == 64" in layout
    body = re.search(r"typedef struct rt_directional \{(.*?)\} rt_directional;", layout, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.strip() for d in body.split(";") if d.strip()] == ["float layer[4][4]"]


def test_calls_without_a_context_are_refused(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    points = np.zeros((4, 8), np.float32)
    out = np.zeros(4, R.DIRECTIONAL_DTYPE)
    st = R.RtRadianceStats()
    assert L.rt_gather_directional(None, points.ctypes.data, 4, 4, 1, 0, out.ctypes.data, None) == RT_ERR_INVALID
    assert L.rt_gather_directional(None, points.ctypes.data, 0, 4, 1, 0, out.ctypes.data, ctypes.addressof(st)) == RT_ERR_INVALID
    assert L.rt_gather_directional_device(None, points.ctypes.data, 4, 4, 1, 0, out.ctypes.data) == RT_ERR_INVALID
    assert L.rt_directional_gather_stats(None, ctypes.addressof(st)) == RT_ERR_INVALID
    d, m = R.RtBakeAtlasDesc(), R.RtLightmapDesc()
    rects = np.zeros((1, 8), np.uint32)
    layers = np.zeros((4, 2, 2), R.IRRADIANCE_DTYPE)
    assert L.rt_bake_atlas_directional(None, ctypes.addressof(d), rects.ctypes.data, None, 0, 1, 1, 0, layers.ctypes.data, None,
                                       None) == RT_ERR_INVALID
    assert L.rt_bake_atlas_directional_lightmap(None, ctypes.addressof(m), rects.ctypes.data, None, 0, layers.ctypes.data,
                                                layers.nbytes, None, None, None) == RT_ERR_INVALID


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
        points = np.zeros((16, 8), np.float32)
        out = np.zeros(16, R.DIRECTIONAL_DTYPE)
        st = R.RtRadianceStats()
        host, dev, stats = L.rt_gather_directional, L.rt_gather_directional_device, L.rt_directional_gather_stats
        p, o = points.ctypes.data, out.ctypes.data

        def message():
            return L.rt_last_error(r.ctx)

        assert stats(r.ctx, ctypes.addressof(st)) == 0 and st.rays == 0 and st.workgroups == 0     # before any gather
        assert stats(r.ctx, None) == RT_ERR_INVALID
        for spp in (0, 65537):
            assert host(r.ctx, p, 16, 4, spp, 0, o, None) == RT_ERR_INVALID and message().startswith(b"directional gather:")
            assert dev(r.ctx, p, 16, 4, spp, 0, o) == RT_ERR_INVALID and b"spp" in message()
        assert host(r.ctx, p, 1 << 31, 4, 1, 0, o, None) == RT_ERR_INVALID and b"points" in message()
        assert dev(r.ctx, p, 1 << 31, 4, 1, 0, o) == RT_ERR_INVALID
        # n == 0 is RT_OK, whatever the pointers, and reports empty stats
        assert host(r.ctx, None, 0, 4, 1, 0, None, ctypes.addressof(st)) == 0 and st.rays == 0 and st.samples == 0
        assert dev(r.ctx, None, 0, 4, 1, 0, None) == 0
        assert host(r.ctx, p, 0, 4, 0, 0, o, None) == RT_ERR_INVALID                               # ... but spp is still checked
        assert host(r.ctx, None, 16, 4, 1, 0, o, None) == RT_ERR_INVALID and message().startswith(b"directional gather: NULL")
        assert host(r.ctx, p, 16, 4, 1, 0, None, None) == RT_ERR_INVALID
        assert dev(r.ctx, None, 16, 4, 1, 0, o) == RT_ERR_INVALID and message().startswith(b"directional gather: NULL")
        assert dev(r.ctx, p, 16, 4, 1, 0, None) == RT_ERR_INVALID
        # no scene
        assert host(r.ctx, p, 16, 4, 1, 0, o, None) == RT_ERR_NOT_READY and message().startswith(b"directional gather: no scene")
        assert host(r.ctx, p, 16, 4, 65536, 0, o, ctypes.addressof(st)) == RT_ERR_NOT_READY
        # the bakes: an atlas bake's rules behind their own prefixes
        d, rects = r._atlas_args([(0, 0, 0, 8, 8)], 8, 8, 1e30, 0)
        layers = np.zeros((4, 8, 8), R.IRRADIANCE_DTYPE)
        bake, lightmap = L.rt_bake_atlas_directional, L.rt_bake_atlas_directional_lightmap
        da, ra, la = ctypes.addressof(d), rects.ctypes.data, layers.ctypes.data
        assert bake(r.ctx, None, ra, None, 0, 1, 1, 0, la, None, None) == RT_ERR_INVALID
        assert message().startswith(b"bake directional: bake atlas: NULL descriptor")
        assert bake(r.ctx, da, ra, None, 0, 1, 1, 0, None, None, None) == RT_ERR_INVALID and message().startswith(b"bake directional: NULL")
        assert bake(r.ctx, da, ra, None, 0, 1, 0, 0, la, None, None) == RT_ERR_INVALID and b"spp" in message()
        assert bake(r.ctx, da, ra, None, 0, 1, 1, 0, la, None, None) == RT_ERR_NOT_READY and message().startswith(b"bake directional:")
        m = r._lightmap_desc(d, 1, 1, 0, None, 0, R.RT_LIGHTMAP_F32)
        ma = ctypes.addressof(m)
        assert lightmap(r.ctx, ma, ra, None, 0, la, layers.nbytes - 1, None, None, None) == RT_ERR_INVALID
        assert message().startswith(b"directional lightmap: out_bytes")
        assert lightmap(r.ctx, ma, ra, None, 0, None, layers.nbytes, None, None, None) == RT_ERR_INVALID
        assert lightmap(r.ctx, ma, ra, None, 0, la, layers.nbytes, None, None, None) == RT_ERR_NOT_READY
        m.format = R.RT_LIGHTMAP_RGBE8
        assert lightmap(r.ctx, ma, ra, None, 0, la, layers.nbytes, None, None, None) == RT_ERR_INVALID
        assert message().startswith(b"directional lightmap: format")
        m.format, m.passes, m.step = R.RT_LIGHTMAP_F32, 4, 1
        assert lightmap(r.ctx, ma, ra, None, 0, la, layers.nbytes, None, None, None) == RT_ERR_INVALID
        assert message().startswith(b"directional lightmap: lightmap: passes")
    finally:
        r.destroy()


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                    reason="node / node_api.h not present")
def test_node_addon_exports_the_bindings(W):
    W._build.build_scene()
    W._build.build_tex()
    W._build.build_rt()
    path = W._build.build_node_addon(force=True)
    assert path and os.path.exists(path)
    node_dir = os.path.dirname(path)
    js = ("const m=require('%s/index.js');console.log(typeof m.native.rtGatherDirectional,"
          "typeof m.native.rtBakeAtlasDirectionalLightmap,typeof m.WebGPURenderer.prototype.gatherDirectional,"
          "typeof m.WebGPURenderer.prototype.bakeAtlasDirectionalLightmap)" % node_dir)
    out = subprocess.run([shutil.which("node"), "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ["function"] * 4
    assert os.path.exists(os.path.join(node_dir, "directional_lightmap.js"))
    dts = open(os.path.join(node_dir, "index.d.ts")).read()
    assert "gatherDirectional(" in dts and "bakeAtlasDirectionalLightmap(" in dts
