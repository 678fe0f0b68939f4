"""Shared pieces of the ray-query tests (rt_trace_rays): ray sets, the two ray layouts, and the comparison with the CPU
oracle's literal traversal loop (OracleRenderer.traceRays), which is the reference of every check."""
import numpy as np

from test_bvh_independent import _random_rays
from test_pairwalk_model import rays_for

SCENES = ["cornell", "viewer_diamond", "special", "mixed", "mesh", "instanced1000", "sponza_like", "glass_blob"]
T_MIN = 0.001


def to_rt_rays(oracle_rays):
    """oracle layout {o, t_min, d, t_max} -> rt_ray layout {o, t_max, d, pad}"""
    o = np.ascontiguousarray(oracle_rays, np.float32)
    r = np.zeros_like(o)
    r[:, 0:3], r[:, 3], r[:, 4:7] = o[:, 0:3], o[:, 7], o[:, 4:7]
    return r


def to_oracle_rays(rt_rays, t_min):
    """rt_ray layout -> oracle layout with the call's t_min"""
    r = np.ascontiguousarray(rt_rays, np.float32)
    o = np.empty_like(r)
    o[:, 0:3], o[:, 3], o[:, 4:7], o[:, 7] = r[:, 0:3], np.float32(t_min), r[:, 4:7], r[:, 3]
    return o


def scene_rays(bridge, shadow, n_a=12000, n_b=8000):
    """rays_for (random origins in the world box, some exactly axis-parallel components; shadow rays with finite t_max)
    plus _random_rays (a fifth nearly axis-parallel), in the oracle's layout: n_a + n_b >= 20 000 per scene."""
    return np.concatenate([rays_for(bridge, n_a, 11, shadow), _random_rays(bridge, n_b, 5)]).astype(np.float32)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 3e38, -3e38], np.float32)


def degenerate_rays(bridge, shadow, n_base=8, seed=3):
    """Every one of n_base ordinary rays with ONE component (origin, direction or t_max) replaced by NaN, +-inf, +-0, a
    denormal or +-3e38, and each base ray once with an all-zero direction.  Oracle layout."""
    base = rays_for(bridge, n_base + 16, seed, shadow)[16:]    # past the block with an exactly zero component
    out = []
    for b in base:
        for comp in (0, 1, 2, 4, 5, 6, 7):
            for v in SPECIALS:
                r = b.copy()
                r[comp] = v
                out.append(r)
        r = b.copy()
        r[4:7] = 0.0
        out.append(r)
    return np.ascontiguousarray(np.stack(out), np.float32)


def check_closest(hits, oracle_rays, ref, tag):
    """hits: structured (t, tri, inst, hit); ref: the oracle's (n, 4) f32 {t, tri, inst, -}"""
    ref_tri = ref[:, 1].astype(np.int64)
    hit = ref_tri >= 0
    assert np.array_equal(hits["hit"] != 0, hit), (tag, "hit flag", int(((hits["hit"] != 0) != hit).sum()))
    assert np.array_equal(hits["tri"].astype(np.int64), np.where(hit, ref_tri, -1)), (tag, "tri")
    assert np.array_equal(hits["inst"].astype(np.int64), np.where(hit, ref[:, 2].astype(np.int64), -1)), (tag, "inst")
    assert np.array_equal(u32(hits["t"])[hit], u32(ref[:, 0])[hit]), (tag, "t of hits")
    assert np.array_equal(u32(hits["t"])[~hit], u32(oracle_rays[:, 7])[~hit]), (tag, "t of misses = t_max bits")
    assert set(np.unique(hits["hit"])) <= {0, 1}, tag


def check_any(hits, ref, tag):
    occ = ref[:, 3] != 0
    assert np.array_equal(hits["hit"] != 0, occ), (tag, "occluded", int(((hits["hit"] != 0) != occ).sum()))
    assert set(np.unique(hits["hit"])) <= {0, 1}, tag
    assert np.all(u32(hits["t"]) == 0) and np.all(hits["tri"] == -1) and np.all(hits["inst"] == -1), tag


def form_of(stats):
    """name of the kernel form a query ran in, from rt_ray_stats"""
    if stats["walk"] == 1:
        return "pair_lds" if stats["lds"] else "pair_global"
    if stats["lds"]:
        return "node_lds"
    return "node_rayreg" if stats["rayreg"] else "node_mixed"


FORMS = ("node_lds", "node_mixed", "node_rayreg", "pair_lds", "pair_global")
# (rt_set_walk, MI355RT_NO_LDS_STAGING, MI355RT_WF_RAYREG): walk 0 / 1 / 2 x unset / 1 x 0 / 1; the RAYREG knob does not
# reach the pair walk, so walk 1 takes it once
CONFIGS = [(walk, no_lds, rayreg) for walk in (0, 1, 2) for no_lds in (None, "1") for rayreg in ("0", "1")
           if not (walk == 1 and rayreg == "1")]


def make_renderer(W, monkeypatch, bridge, walk, no_lds, rayreg):
    """a context created AFTER the env knobs are set, with the scene uploaded (no screen, no pipeline: a query needs neither)"""
    if no_lds is None:
        monkeypatch.delenv("MI355RT_NO_LDS_STAGING", raising=False)
    else:
        monkeypatch.setenv("MI355RT_NO_LDS_STAGING", no_lds)
    monkeypatch.setenv("MI355RT_WF_RAYREG", rayreg)
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    r.setWalk(walk)
    r.updateCombinedGeometry(bridge.vertices, bridge.normals, bridge.uvs)
    r.updateCombinedBVH(bridge.tlas, bridge.blas)
    r.updateBuffer("topology", bridge.mesh_topology)
    r.updateBuffer("instance", bridge.instances)
    r.updateBuffer("lights", bridge.lights)
    return r


def oracle_for(W, oracle_lib, bridge):
    cpu = oracle_lib.OracleRenderer()
    cpu.buildPipeline(4, 1)
    W.upload_scene(cpu, bridge, 16, 16)
    return cpu
