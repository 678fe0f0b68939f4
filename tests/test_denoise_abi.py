"""Atlas denoise (rt_denoise_atlas / rt_denoise_atlas_device), the parts that need no GPU: the two symbols are declared,
exported and bound; the descriptor is the documented 32 bytes with its fields where the header puts them; RT_DENOISE_MAX_STEP
is 4; a call without a context is refused with the error code; the bakes take denoise=; the Node addon carries the binding."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_denoise_atlas", "rt_denoise_atlas_device")
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
    for m in ("denoiseAtlas", "denoiseAtlasDevice"):
        assert callable(getattr(W.WebGPURenderer, m))
    blob = open(W._build.RT_LIB, "rb").read()
    for k in (b"k_denoise_index", b"k_denoise_pass"):
        assert k in blob, k


def test_descriptor_layout(W):
    from webgpu_raytracer_amd import renderer as R
    D = R.RtDenoiseDesc
    assert ctypes.sizeof(D) == 32
    assert [(n, getattr(D, n).offset) for n, _ in D._fields_] == [
        ("width", 0), ("height", 4), ("step", 8), ("passes", 12), ("normal_cos", 16), ("plane_eps", 20), ("max_dist", 24),
        ("reserved", 28)]
    assert D.reserved.size == 4
    assert [t for _, t in D._fields_][4:7] == [ctypes.c_float] * 3
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    assert "static_assert(sizeof(rt_denoise_desc) == 32" in layout
    assert re.search(r"#define\s+RT_DENOISE_MAX_STEP\s+4u", layout)
    body = re.search(r"typedef struct rt_denoise_desc \{(.*?)\} rt_denoise_desc;", layout, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.strip() for d in body.split(";") if d.strip()] == [
        "uint32_t width, height", "uint32_t step", "uint32_t passes", "float normal_cos", "float plane_eps", "float max_dist",
        "uint32_t reserved[1]"]


def test_the_methods_take_the_documented_arguments(W):
    for m in ("bakeIrradiance", "bakeAtlasIrradiance"):
        p = inspect.signature(getattr(W.WebGPURenderer, m)).parameters
        assert p["denoise"].default is None, m
        assert "extra point pass" in getattr(W.WebGPURenderer, m).__doc__, m
    p = inspect.signature(W.WebGPURenderer.denoiseAtlas).parameters
    assert list(p)[:4] == ["self", "atlas", "points", "texels"]
    for name, default in (("plane_eps", inspect.Parameter.empty), ("max_dist", inspect.Parameter.empty), ("normal_cos", 0.9),
                          ("passes", 3), ("step", 1)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, name


def test_calls_without_a_context_are_refused(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    atlas = np.zeros((4, 4, 4), np.float32)
    out = np.zeros((4, 4, 4), np.float32)
    d = R.RtDenoiseDesc(4, 4, 1, 1, 0.9, 0.01, 1.0)
    for call in (L.rt_denoise_atlas, L.rt_denoise_atlas_device):
        assert call(None, ctypes.addressof(d), atlas.ctypes.data, None, None, 0, out.ctypes.data) == RT_ERR_INVALID


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                    reason="node / node_api.h not present")
def test_node_addon_exports_the_binding(W):
    W._build.build_scene()
    W._build.build_tex()
    W._build.build_rt()
    path = W._build.build_node_addon(force=True)
    assert path and os.path.exists(path)
    node_dir = os.path.dirname(path)
    js = ("const m=require('%s/index.js');console.log(typeof m.native.rtDenoiseAtlas,"
          "typeof m.WebGPURenderer.prototype.denoiseAtlas)" % node_dir)
    out = subprocess.run([shutil.which("node"), "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ["function"] * 2
    assert "denoiseAtlas(" in open(os.path.join(node_dir, "index.d.ts")).read()
    for tool in ("bake_lightmap.js", "bake_atlas.js"):
        text = open(os.path.join(node_dir, tool)).read()
        for flag in ("--denoise", "--plane-eps", "--max-dist", "--normal-cos"):
            assert flag in text, (tool, flag)
