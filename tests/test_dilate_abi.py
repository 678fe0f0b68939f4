"""Atlas dilation (rt_dilate_atlas / rt_dilate_atlas_device), the parts that need no GPU: the two symbols are declared,
exported and bound; the descriptor is the documented 32 bytes with its fields where the header puts them; a call without a
context is refused with the error code; the Node addon carries the binding."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_dilate_atlas", "rt_dilate_atlas_device")
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
    for m in ("dilateAtlas", "dilateAtlasDevice"):
        assert callable(getattr(W.WebGPURenderer, m))
    blob = open(W._build.RT_LIB, "rb").read()
    for k in (b"k_dilate_mask", b"k_dilate_source", b"k_dilate_apply"):
        assert k in blob, k


def test_descriptor_layout(W):
    from webgpu_raytracer_amd import renderer as R
    D = R.RtDilateDesc
    assert ctypes.sizeof(D) == 32
    assert [(n, getattr(D, n).offset) for n, _ in D._fields_] == [("width", 0), ("height", 4), ("radius", 8), ("reserved", 12)]
    assert D.reserved.size == 20
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    assert "static_assert(sizeof(rt_dilate_desc) == 32" in layout
    assert re.search(r"#define\s+RT_DILATE_MAX_RADIUS\s+24u", layout)
    body = re.search(r"typedef struct rt_dilate_desc \{(.*?)\} rt_dilate_desc;", layout, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.strip() for d in body.split(";") if d.strip()] == ["uint32_t width, height", "uint32_t radius", "uint32_t reserved[5]"]


def test_the_bake_methods_take_dilate(W):
    import inspect
    for m in ("bakeIrradiance", "bakeAtlasIrradiance"):
        p = inspect.signature(getattr(W.WebGPURenderer, m)).parameters
        assert p["dilate"].default == 0, m


def test_calls_without_a_context_are_refused(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    atlas = np.zeros((4, 4, 4), np.float32)
    src = np.zeros((4, 4), np.uint32)
    n = ctypes.c_uint32(0)
    d = R.RtDilateDesc(4, 4, 2)
    assert L.rt_dilate_atlas(None, ctypes.addressof(d), atlas.ctypes.data, src.ctypes.data, ctypes.addressof(n)) == RT_ERR_INVALID
    assert L.rt_dilate_atlas(None, ctypes.addressof(d), atlas.ctypes.data, None, None) == RT_ERR_INVALID
    assert L.rt_dilate_atlas_device(None, ctypes.addressof(d), atlas.ctypes.data, None, None) == RT_ERR_INVALID


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                    reason="node / node_api.h not present")
def test_node_addon_exports_the_binding(W):
    W._build.build_scene()
    W._build.build_tex()
    W._build.build_rt()
    path = W._build.build_node_addon(force=True)
    assert path and os.path.exists(path)
    node_dir = os.path.dirname(path)
    js = ("const m=require('%s/index.js');console.log(typeof m.native.rtDilateAtlas,"
          "typeof m.WebGPURenderer.prototype.dilateAtlas)" % node_dir)
    out = subprocess.run([shutil.which("node"), "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ["function"] * 2
    assert "dilateAtlas(" in open(os.path.join(node_dir, "index.d.ts")).read()
    for tool in ("bake_lightmap.js", "bake_atlas.js"):
        assert "--dilate" in open(os.path.join(node_dir, tool)).read(), tool
