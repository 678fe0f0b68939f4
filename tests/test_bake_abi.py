"""Lightmap bakes (rt_bake_points / rt_bake_points_device / rt_bake_irradiance), the parts that need no GPU: the three symbols
are declared, exported and bound; rt_bake_desc is the documented 32 bytes; calls without a context are refused; the Node
addon carries the bindings and the example exists."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_bake_points", "rt_bake_points_device", "rt_bake_irradiance")


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
    for m in ("bakePoints", "bakePointsDevice", "bakeIrradiance"):
        assert callable(getattr(W.WebGPURenderer, m))


def test_descriptor_layout(W):
    from webgpu_raytracer_amd import renderer as R
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    assert "static_assert(sizeof(rt_bake_desc) == 32" in layout
    body = re.search(r"typedef struct rt_bake_desc \{(.*?)\} rt_bake_desc;", layout, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().split("[")[0] for d in body.split(";") if d.strip() for n in d.strip().split(None, 1)[1].split(",")]
    assert names == ["inst", "width", "height", "pad_base", "t_max", "reserved"]
    assert ctypes.sizeof(R.RtBakeDesc) == 32
    assert [f[0] for f in R.RtBakeDesc._fields_] == names
    assert [getattr(R.RtBakeDesc, n).offset for n in names] == [0, 4, 8, 12, 16, 20]


def test_calls_without_a_context_are_refused(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    d = R.RtBakeDesc(0, 4, 4, 0, 1e30)
    points = np.zeros((16, 8), np.float32)
    texels = np.zeros(16, np.uint32)
    atlas = np.zeros(16, R.IRRADIANCE_DTYPE)
    n = ctypes.c_uint32(0)
    RT_ERR_INVALID = -1
    assert L.rt_bake_points(None, ctypes.addressof(d), None, 0, points.ctypes.data, texels.ctypes.data, 16, ctypes.addressof(n),
                            None) == RT_ERR_INVALID
    assert L.rt_bake_points_device(None, ctypes.addressof(d), None, points.ctypes.data, texels.ctypes.data, 16,
                                   ctypes.addressof(n), None) == RT_ERR_INVALID
    assert L.rt_bake_irradiance(None, ctypes.addressof(d), None, 0, 4, 1, 0, atlas.ctypes.data, ctypes.addressof(n),
                                None) == RT_ERR_INVALID


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                    reason="node / node_api.h not present")
def test_node_addon_exports_the_bindings(W):
    W._build.build_scene()
    W._build.build_tex()
    W._build.build_rt()
    path = W._build.build_node_addon(force=True)
    assert path and os.path.exists(path)
    node_dir = os.path.dirname(path)
    js = ("const m=require('%s/index.js');console.log(typeof m.native.rtBakePoints,typeof m.native.rtBakeIrradiance,"
          "typeof m.WebGPURenderer.prototype.bakePoints,typeof m.WebGPURenderer.prototype.bakeIrradiance)" % node_dir)
    out = subprocess.run([shutil.which("node"), "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ["function"] * 4
    assert os.path.exists(os.path.join(node_dir, "bake_lightmap.js"))
    dts = open(os.path.join(node_dir, "index.d.ts")).read()
    assert "bakePoints(" in dts and "bakeIrradiance(" in dts
