"""Radiance queries (rt_trace_radiance / rt_trace_radiance_device / rt_radiance_query_stats), the parts that need no GPU: the
three symbols are declared, exported and bound; the record layouts are the documented 16 / 72 bytes; calls without a
context are refused; the Node addon carries the binding."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_trace_radiance", "rt_trace_radiance_device", "rt_radiance_query_stats")


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
    for m in ("traceRadiance", "traceRadianceDevice", "radianceQueryStats"):
        assert callable(getattr(W.WebGPURenderer, m))


def test_record_layouts(W):
    from webgpu_raytracer_amd import renderer as R
    S = R.RtRadianceStats
    assert ctypes.sizeof(S) == 72
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 60, 64]
    assert [f for f, _ in S._fields_] == ["rays", "samples", "extension_rays", "shadow_rays", "shaded_hits", "nodes_visited",
                                          "tris_tested", "lds", "workgroups", "kernel_ms"]
    assert R.RADIANCE_DTYPE.itemsize == 16
    assert R.RADIANCE_DTYPE.fields["rgb"][1] == 0 and R.RADIANCE_DTYPE.fields["t"][1] == 12
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    for name, size in (("rt_radiance", 16), ("rt_radiance_stats", 72)):
        assert "static_assert(sizeof(%s) == %d" % (name, size) in layout
    # the struct as the header declares it: field order of rt_radiance_stats
    body = re.search(r"typedef struct rt_radiance_stats \{(.*?)\} rt_radiance_stats;", layout, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f for f, _ in S._fields_]


def test_calls_without_a_context_are_refused(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    rays = np.zeros((4, 8), np.float32)
    out = np.zeros(4, R.RADIANCE_DTYPE)
    st = R.RtRadianceStats()
    RT_ERR_INVALID = -1
    assert L.rt_trace_radiance(None, rays.ctypes.data, 4, 4, 1, 0, out.ctypes.data, None) == RT_ERR_INVALID
    assert L.rt_trace_radiance(None, rays.ctypes.data, 0, 4, 1, 0, out.ctypes.data, ctypes.addressof(st)) == RT_ERR_INVALID
    assert L.rt_trace_radiance_device(None, rays.ctypes.data, 4, 4, 1, 0, out.ctypes.data) == RT_ERR_INVALID
    assert L.rt_radiance_query_stats(None, ctypes.addressof(st)) == RT_ERR_INVALID


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                    reason="node / node_api.h not present")
def test_node_addon_exports_the_binding(W):
    W._build.build_rt()
    path = W._build.build_node_addon(force=True)
    assert path and os.path.exists(path)
    node_dir = os.path.dirname(path)
    js = ("const m=require('%s/index.js');console.log(typeof m.native.rtTraceRadiance,"
          "typeof m.WebGPURenderer.prototype.traceRadiance)" % node_dir)
    out = subprocess.run([shutil.which("node"), "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ["function"] * 2
    assert os.path.exists(os.path.join(node_dir, "trace_radiance.js"))
    assert "traceRadiance(" in open(os.path.join(node_dir, "index.d.ts")).read()
