"""Irradiance gathers (rt_gather_irradiance / rt_gather_irradiance_device / rt_irradiance_gather_stats), the parts that need
no GPU: the three symbols are declared, exported and bound; the record layouts are the documented 32 / 16 bytes with the
slots of rt_ray; calls without a context are refused; the Node addon carries the binding."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_gather_irradiance", "rt_gather_irradiance_device", "rt_irradiance_gather_stats")


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
    for m in ("gatherIrradiance", "gatherIrradianceDevice", "irradianceGatherStats"):
        assert callable(getattr(W.WebGPURenderer, m))


def _fields(layout, name):
    """[(type, field, array length or None)] of a struct as the layout header declares it"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), layout, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            typ, rest = decl.strip().split(None, 1)
            m = re.match(r"(\w+)(?:\[(\d+)\])?$", rest.strip())
            out.append((typ, m.group(1), int(m.group(2)) if m.group(2) else None))
    return out


def test_record_layouts(W):
    from webgpu_raytracer_amd import renderer as R
    D = R.IRRADIANCE_DTYPE
    assert D.itemsize == 16
    assert D.fields["rgb"][1] == 0 and D.fields["hit_fraction"][1] == 12 and D.names == ("rgb", "hit_fraction")
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    for name, size in (("rt_gather_point", 32), ("rt_irradiance", 16)):
        assert "static_assert(sizeof(%s) == %d" % (name, size) in layout
    # the point has the slots of rt_ray, word for word
    assert _fields(layout, "rt_gather_point") == [("float", "position", 3), ("float", "t_max", None), ("float", "normal", 3),
                                                  ("uint32_t", "pad", None)]
    assert [(t, n) for t, _, n in _fields(layout, "rt_gather_point")] == [(t, n) for t, _, n in _fields(layout, "rt_ray")]
    assert _fields(layout, "rt_irradiance") == [("float", "rgb", 3), ("float", "hit_fraction", None)]


def test_calls_without_a_context_are_refused(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    points = np.zeros((4, 8), np.float32)
    out = np.zeros(4, R.IRRADIANCE_DTYPE)
    st = R.RtRadianceStats()
    RT_ERR_INVALID = -1
    assert L.rt_gather_irradiance(None, points.ctypes.data, 4, 4, 1, 0, out.ctypes.data, None) == RT_ERR_INVALID
    assert L.rt_gather_irradiance(None, points.ctypes.data, 0, 4, 1, 0, out.ctypes.data, ctypes.addressof(st)) == RT_ERR_INVALID
    assert L.rt_gather_irradiance_device(None, points.ctypes.data, 4, 4, 1, 0, out.ctypes.data) == RT_ERR_INVALID
    assert L.rt_irradiance_gather_stats(None, ctypes.addressof(st)) == RT_ERR_INVALID


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                    reason="node / node_api.h not present")
def test_node_addon_exports_the_binding(W):
    W._build.build_rt()
    path = W._build.build_node_addon(force=True)
    assert path and os.path.exists(path)
    node_dir = os.path.dirname(path)
    js = ("const m=require('%s/index.js');console.log(typeof m.native.rtGatherIrradiance,"
          "typeof m.WebGPURenderer.prototype.gatherIrradiance)" % node_dir)
    out = subprocess.run([shutil.which("node"), "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ["function"] * 2
    assert os.path.exists(os.path.join(node_dir, "gather_irradiance.js"))
    assert "gatherIrradiance(" in open(os.path.join(node_dir, "index.d.ts")).read()
