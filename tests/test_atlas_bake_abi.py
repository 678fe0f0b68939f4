"""Atlas bakes (rt_bake_atlas_points / rt_bake_atlas_points_device / rt_bake_atlas_irradiance), the parts that need no GPU: the
three symbols are declared, exported and bound; rt_bake_atlas_desc and rt_bake_rect are the documented 32 bytes, with the
same fields in the header and in ctypes; calls without a context are refused; the Node addon carries the bindings and the
example exists."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_bake_atlas_points", "rt_bake_atlas_points_device", "rt_bake_atlas_irradiance")


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
    for m in ("bakeAtlasPoints", "bakeAtlasPointsDevice", "bakeAtlasIrradiance"):
        assert callable(getattr(W.WebGPURenderer, m))


@pytest.mark.parametrize("struct,mirror,names,offsets", [
    ("rt_bake_atlas_desc", "RtBakeAtlasDesc", ["width", "height", "pad_base", "t_max", "n_entries", "reserved"], [0, 4, 8, 12, 16, 20]),
    ("rt_bake_rect", "RtBakeRect", ["inst", "x", "y", "width", "height", "reserved"], [0, 4, 8, 12, 16, 20])])
def test_struct_layouts(W, struct, mirror, names, offsets):
    from webgpu_raytracer_amd import renderer as R
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    assert "static_assert(sizeof(%s) == 32" % struct in layout
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), layout, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n.strip().split("[")[0] for d in body.split(";") if d.strip() for n in d.strip().split(None, 1)[1].split(",")]
    assert declared == names
    S = getattr(R, mirror)
    assert ctypes.sizeof(S) == 32
    assert [f[0] for f in S._fields_] == names
    assert [getattr(S, n).offset for n in names] == offsets


def test_the_python_binding_lays_the_entries_out_as_rects(W):
    d, rects = W.WebGPURenderer._atlas_args([(3, 1, 2, 4, 5), (0, 0, 0, 1, 1)], 9, 8, 2.5, 7)
    assert (d.width, d.height, d.pad_base, d.t_max, d.n_entries, list(d.reserved)) == (9, 8, 7, 2.5, 2, [0, 0, 0])
    assert rects.dtype == np.uint32 and rects.tolist() == [[3, 1, 2, 4, 5, 0, 0, 0], [0, 0, 0, 1, 1, 0, 0, 0]]
    with pytest.raises(ValueError):
        W.WebGPURenderer._atlas_args([(0, -1, 0, 4, 4)], 8, 8, 1.0, 0)


def test_calls_without_a_context_are_refused(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    d = R.RtBakeAtlasDesc(4, 4, 0, 1e30, 1)
    q = R.RtBakeRect(0, 0, 0, 4, 4)
    points = np.zeros((16, 8), np.float32)
    texels = np.zeros(16, np.uint32)
    atlas = np.zeros(16, R.IRRADIANCE_DTYPE)
    n = ctypes.c_uint32(0)
    RT_ERR_INVALID = -1
    assert L.rt_bake_atlas_points(None, ctypes.addressof(d), ctypes.addressof(q), None, 0, points.ctypes.data, texels.ctypes.data,
                                  16, ctypes.addressof(n), None) == RT_ERR_INVALID
    assert L.rt_bake_atlas_points_device(None, ctypes.addressof(d), ctypes.addressof(q), None, points.ctypes.data,
                                         texels.ctypes.data, 16, ctypes.addressof(n), None) == RT_ERR_INVALID
    assert L.rt_bake_atlas_irradiance(None, ctypes.addressof(d), ctypes.addressof(q), None, 0, 4, 1, 0, atlas.ctypes.data,
                                      ctypes.addressof(n), None) == RT_ERR_INVALID


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                    reason="node / node_api.h not present")
def test_node_addon_exports_the_bindings(W):
    W._build.build_scene()
    W._build.build_tex()
    W._build.build_rt()
    path = W._build.build_node_addon(force=True)
    assert path and os.path.exists(path)
    node_dir = os.path.dirname(path)
    js = ("const m=require('%s/index.js');console.log(typeof m.native.rtBakeAtlasPoints,typeof m.native.rtBakeAtlasIrradiance,"
          "typeof m.WebGPURenderer.prototype.bakeAtlasPoints,typeof m.WebGPURenderer.prototype.bakeAtlasIrradiance);"
          "console.log(JSON.stringify(Array.from(m.WebGPURenderer._atlasEntries([[3,1,2,4,5],[0,0,0,1,1]]))))" % node_dir)
    out = subprocess.run([shutil.which("node"), "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split()[0:4] == ["function"] * 4
    assert out.split()[4] == "[3,1,2,4,5,0,0,0,0,0,0,1,1,0,0,0]"
    assert os.path.exists(os.path.join(node_dir, "bake_atlas.js"))
    dts = open(os.path.join(node_dir, "index.d.ts")).read()
    assert "bakeAtlasPoints(" in dts and "bakeAtlasIrradiance(" in dts
