"""Ray queries (rt_trace_rays / rt_trace_rays_device / rt_ray_query_stats), the parts that need no GPU: the three symbols
are declared, exported and bound; the record layouts are the documented 32 / 16 / 48 bytes; calls without a context are
refused; the Node addon carries the binding; and the degenerate rays the GPU test sends are first put through the host
compilation of the pair walk and through the oracle, which must both terminate and agree."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pair_layout
import parity_util as pu
import ray_query_util as rq
from test_pairwalk_model import model_lib, _p

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_trace_rays", "rt_trace_rays_device", "rt_ray_query_stats")


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
    assert "RT_RAYS_CLOSEST = 0" in header and "RT_RAYS_ANY = 1" in header
    for m in ("traceRays", "traceRaysDevice", "rayQueryStats"):
        assert callable(getattr(W.WebGPURenderer, m))


def test_record_layouts(W):
    from webgpu_raytracer_amd import renderer as R
    assert ctypes.sizeof(R.RtRay) == 32 and ctypes.sizeof(R.RtRayHit) == 16 and ctypes.sizeof(R.RtRayStats) == 48
    assert R.RtRay.t_max.offset == 12 and R.RtRay.dir.offset == 16          # {o, t_max} {d, pad}: the queue record
    assert (R.RtRayHit.t.offset, R.RtRayHit.tri.offset, R.RtRayHit.inst.offset, R.RtRayHit.hit.offset) == (0, 4, 8, 12)
    assert R.RtRayStats.walk.offset == 24 and R.RtRayStats.kernel_ms.offset == 40
    assert R.RAY_HIT_DTYPE.itemsize == 16
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    for name, size in (("rt_ray", 32), ("rt_ray_hit", 16), ("rt_ray_stats", 48)):
        assert "static_assert(sizeof(%s) == %d" % (name, size) in layout


def test_calls_without_a_context_are_refused(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    rays = np.zeros((4, 8), np.float32)
    hits = np.zeros(4, R.RAY_HIT_DTYPE)
    st = R.RtRayStats()
    RT_ERR_INVALID = -1
    assert L.rt_trace_rays(None, rays.ctypes.data, 4, 0, 0.001, hits.ctypes.data, None) == RT_ERR_INVALID
    assert L.rt_trace_rays(None, rays.ctypes.data, 0, 0, 0.001, hits.ctypes.data, ctypes.addressof(st)) == RT_ERR_INVALID
    assert L.rt_trace_rays_device(None, rays.ctypes.data, 4, 1, 0.001, hits.ctypes.data) == RT_ERR_INVALID
    assert L.rt_ray_query_stats(None, ctypes.addressof(st)) == RT_ERR_INVALID


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                    reason="node / node_api.h not present")
def test_node_addon_exports_the_binding(W):
    W._build.build_rt()
    path = W._build.build_node_addon(force=True)
    assert path and os.path.exists(path)
    node_dir = os.path.dirname(path)
    js = ("const m=require('%s/index.js');console.log(typeof m.native.rtTraceRays, typeof m.native.rtRayQueryStats,"
          "typeof m.WebGPURenderer.prototype.traceRays, typeof m.WebGPURenderer.prototype.rayQueryStats)" % node_dir)
    out = subprocess.run([shutil.which("node"), "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ["function"] * 4
    assert os.path.exists(os.path.join(node_dir, "trace_rays.js"))
    assert "traceRays(" in open(os.path.join(node_dir, "index.d.ts")).read()


@pytest.mark.parametrize("scene", ["cornell", "mixed", "instanced1000", "special"])
def test_degenerate_rays_terminate_and_agree_on_the_cpu(W, oracle_lib, scene):
    """The rays of tests/test_gpu_ray_query.py::test_degenerate_rays through the host-compiled pair walk (stack 1 and 8) and
    the oracle: both come back, with the same results.  (Counters are not compared: they differ on a NaN t_max.)"""
    b = pu.bridge_for(W, scene)
    pairs, troot, inst_root = pair_layout.build(b.tlas, b.blas, b.instances)
    tri, inst_trav = pair_layout.traversal_records(b)
    L = model_lib()
    cpu = rq.oracle_for(W, oracle_lib, b)
    for shadow in (False, True):
        rays = rq.degenerate_rays(b, shadow)
        n = rays.shape[0]
        assert n == 8 * (7 * 8 + 1)
        ref, _ = cpu.traceRays(rays, any_hit=shadow)
        for k in (1, 8):
            out = np.zeros((n, 4), np.float32)
            counts = np.zeros((n, 2), np.uint64)
            stats = np.zeros(4, np.uint64)
            L.pwm_trace(_p(pairs), _p(troot), _p(inst_trav), _p(inst_root), _p(tri), _p(rays), n, int(shadow), k, 1,
                        _p(out), _p(counts), _p(stats))
            if shadow:
                assert np.array_equal(out[:, 3], ref[:, 3]), (scene, k)
            else:
                hit = ref[:, 1] >= 0
                assert np.array_equal(out[:, 1:3], ref[:, 1:3]), (scene, k)
                assert np.array_equal(rq.u32(out[:, 0])[hit], rq.u32(ref[:, 0])[hit]), (scene, k)
