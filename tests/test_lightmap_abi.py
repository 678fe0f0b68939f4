"""Lightmaps (rt_bake_atlas_lightmap / _device, rt_encode_atlas / _device), the parts that need no GPU: the four symbols are
declared, exported and bound; the descriptor is the documented 64 bytes with its fields where the header puts them; the
format constants are 0, 1, 2; a call without a context is refused with the error code; the methods take the documented
arguments and the slow route keeps its own; the Node addon carries the bindings and the tool."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_bake_atlas_lightmap", "rt_bake_atlas_lightmap_device", "rt_encode_atlas", "rt_encode_atlas_device")
RT_ERR_INVALID = -1


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
    for m in ("bakeAtlasLightmap", "bakeLightmap", "bakeAtlasLightmapDevice", "encodeAtlas", "encodeAtlasDevice"):
        assert callable(getattr(W.WebGPURenderer, m)), m
    assert callable(W.decode_rgbe) and callable(W.write_hdr)
    assert b"k_encode_atlas" in open(W._build.RT_LIB, "rb").read()


def test_descriptor_layout(W):
    from webgpu_raytracer_amd import renderer as R
    D = R.RtLightmapDesc
    assert ctypes.sizeof(D) == 64
    assert [(n, getattr(D, n).offset) for n, _ in D._fields_] == [
        ("width", 0), ("height", 4), ("pad_base", 8), ("t_max", 12), ("n_entries", 16), ("max_depth", 20), ("spp", 24),
        ("seed", 28), ("passes", 32), ("step", 36), ("normal_cos", 40), ("plane_eps", 44), ("max_dist", 48),
        ("dilate_radius", 52), ("format", 56), ("reserved", 60)]
    assert D.reserved.size == 4
    assert [n for n, t in D._fields_ if t is ctypes.c_float] == ["t_max", "normal_cos", "plane_eps", "max_dist"]
    # the first five fields are rt_bake_atlas_desc's, in its order
    assert [n for n, _ in D._fields_][:5] == [n for n, _ in R.RtBakeAtlasDesc._fields_][:5]
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    assert "static_assert(sizeof(rt_lightmap_desc) == 64" in layout
    for name, value in (("RT_LIGHTMAP_F32", 0), ("RT_LIGHTMAP_F16", 1), ("RT_LIGHTMAP_RGBE8", 2)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, value), layout), name
        assert getattr(R, name) == value
    assert R.LIGHTMAP_TEXEL_BYTES == {0: 16, 1: 8, 2: 4}
    body = re.search(r"typedef struct rt_lightmap_desc \{(.*?)\} rt_lightmap_desc;", layout, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.strip() for d in body.split(";") if d.strip()] == [
        "uint32_t width, height", "uint32_t pad_base", "float t_max", "uint32_t n_entries", "uint32_t max_depth, spp, seed",
        "uint32_t passes", "uint32_t step", "float normal_cos", "float plane_eps", "float max_dist", "uint32_t dilate_radius",
        "uint32_t format", "uint32_t reserved[1]"]


def test_the_methods_take_the_documented_arguments(W):
    p = inspect.signature(W.WebGPURenderer.bakeAtlasLightmap).parameters
    assert list(p) == ["self", "entries", "width", "height", "max_depth", "spp", "seed", "t_max", "pad_base", "atlas_uv", "denoise",
                       "dilate", "format", "stats"]
    assert (p["seed"].default, p["pad_base"].default, p["atlas_uv"].default, p["denoise"].default, p["dilate"].default,
            p["format"].default, p["stats"].default) == (0, 0, None, None, 0, "f32", False)
    q = inspect.signature(W.WebGPURenderer.bakeLightmap).parameters
    assert list(q) == ["self", "inst"] + list(p)[2:]
    # the slow route is what it was
    for m in ("bakeIrradiance", "bakeAtlasIrradiance"):
        s = inspect.signature(getattr(W.WebGPURenderer, m)).parameters
        assert s["denoise"].default is None and s["dilate"].default == 0, m
        assert "extra point pass" in getattr(W.WebGPURenderer, m).__doc__, m
    from webgpu_raytracer_amd import renderer as R
    with pytest.raises(ValueError):
        R._lightmap_format("rgbm")
    assert [R._lightmap_format(f) for f in ("f32", "F16", "rgbe", "rgbe8", 2)] == [0, 1, 2, 2, 2]


def test_calls_without_a_context_are_refused(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    atlas = np.zeros((4, 4, 4), np.float32)
    out = np.zeros((4, 4, 4), np.float32)
    d = R.RtLightmapDesc(4, 4, 0, 1e30, 1, 2, 4, 0)
    rect = R.RtBakeRect(0, 0, 0, 4, 4)
    n = ctypes.c_uint32(0)
    for call in (L.rt_bake_atlas_lightmap,):
        assert call(None, ctypes.addressof(d), ctypes.addressof(rect), None, 0, out.ctypes.data, out.nbytes, ctypes.addressof(n),
                    None, None) == RT_ERR_INVALID
    assert L.rt_bake_atlas_lightmap_device(None, ctypes.addressof(d), ctypes.addressof(rect), None, out.ctypes.data, out.nbytes,
                                           None, None, None) == RT_ERR_INVALID
    for call in (L.rt_encode_atlas, L.rt_encode_atlas_device):
        assert call(None, 4, 4, 1, atlas.ctypes.data, out.ctypes.data, out.nbytes) == RT_ERR_INVALID


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                    reason="node / node_api.h not present")
def test_node_addon_exports_the_binding(W):
    W._build.build_scene()
    W._build.build_tex()
    W._build.build_rt()
    path = W._build.build_node_addon(force=True)
    assert path and os.path.exists(path)
    node_dir = os.path.dirname(path)
    js = ("const m=require('%s/index.js');console.log(typeof m.native.rtBakeAtlasLightmap,typeof m.native.rtEncodeAtlas,"
          "typeof m.WebGPURenderer.prototype.bakeAtlasLightmap,typeof m.WebGPURenderer.prototype.encodeAtlas)" % node_dir)
    out = subprocess.run([shutil.which("node"), "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ["function"] * 4
    dts = open(os.path.join(node_dir, "index.d.ts")).read()
    assert "bakeAtlasLightmap(" in dts and "encodeAtlas(" in dts
    tool = open(os.path.join(node_dir, "lightmap.js")).read()
    for flag in ("--format", "--denoise", "--dilate", "--out"):
        assert flag in tool, flag
