"""Shared pieces of the radiance-query tests (rt_trace_radiance): the reference model (tests/model/radiance_model.cpp: the
oracle's translation unit plus the bounce loop restated once, with one surface-frame function and a switch between the
oracle's G-buffer depth 0 and the traced depth 0 of a query), built with the flags of oracle/Makefile and driven through an
OracleRenderer that loads the model library instead of librt_oracle.so."""
import ctypes
import functools
import os

import numpy as np

import model_build
import oracle_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "model", "radiance_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libradiance_model.so")
# CXXFLAGS of oracle/Makefile
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra", "-pthread"]
COUNT_NAMES = ("extension_rays", "shadow_rays", "shaded_hits", "nodes_visited", "tris_tested")
PAD_STEP, PAD_0, SEED = 7, 3, 5


def bind_model(path):
    """a library that holds the radiance model's translation unit: every oracle_* entry declared as oracle_lib declares it,
    plus the two radiance_model_* ones"""
    L = oracle_lib.bind(path)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.radiance_model_trace.argtypes = [vp, vp, u32, u32, u32, u32, ctypes.c_int, vp, vp]
    L.radiance_model_trace.restype = None
    L.radiance_model_camera_rays.argtypes = [vp, vp]
    L.radiance_model_camera_rays.restype = None
    return L


@functools.lru_cache(maxsize=None)
def model_lib():
    return bind_model(model_build.build(SRC, LIB, FLAGS + ["-shared"]))


class ModelRenderer(oracle_lib.OracleRenderer):
    """OracleRenderer on the model library: the whole oracle, plus traceRadiance / cameraRays"""
    _library = staticmethod(model_lib)

    def traceRadiance(self, rays, max_depth, spp, seed, gbuffer_depth0=False):
        """rays (n, 8) f32 in the rt_ray layout -> (out (n, 4) f32 {r, g, b, t}, counts (n, 5) u64 COUNT_NAMES)"""
        r = np.ascontiguousarray(rays, dtype=np.float32)
        n = r.shape[0]
        out = np.empty((n, 4), np.float32)
        counts = np.empty((n, 5), np.uint64)
        self.L.radiance_model_trace(self.ctx, r.ctypes.data, n, max_depth, spp, seed & 0xffffffff, 1 if gbuffer_depth0 else 0,
                                    out.ctypes.data, counts.ctypes.data)
        return out, counts

    def cameraRays(self):
        """the pinhole rays of the frame computed last, (width * height, 8) f32 in the rt_ray layout, pad = pixel index"""
        out = np.empty((self.width * self.height, 8), np.float32)
        self.L.radiance_model_camera_rays(self.ctx, out.ctypes.data)
        return out


def model_for(W, bridge, width=16, height=16, cls=ModelRenderer):
    """a model of class `cls` with the scene uploaded as upload_scene does it (textures, light count of the bridge)"""
    m = cls()
    m.buildPipeline(4, 1)
    W.upload_scene(m, bridge, width, height)
    return m


def with_pads(rt_rays, step=PAD_STEP, first=PAD_0):
    """rt_ray layout with pad = step * i + first (the ray's RNG stream id) in the eighth word"""
    r = np.ascontiguousarray(rt_rays, np.float32).copy()
    r.view(np.uint32)[:, 7] = (np.arange(r.shape[0], dtype=np.uint64) * step + first).astype(np.uint32)
    return r


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def result_words(res, width=4):
    """structured result records (n,) of `width` words each (RADIANCE_DTYPE, IRRADIANCE_DTYPE: 4) -> (n, width) u32"""
    return np.ascontiguousarray(res).view(np.uint32).reshape(-1, width)


def check_against_model(res, ref, tag, nan_as_class=False):
    """res: RADIANCE_DTYPE (n,); ref: the model's (n, 4) f32.  Bit for bit, ray by ray (NaNs as a class on request)."""
    got, want = result_words(res), u32(ref)
    if nan_as_class:
        gf, wf = got.view(np.float32), want.view(np.float32)
        both_nan = np.isnan(gf) & np.isnan(wf)
        bad = (got != want) & ~both_nan
    else:
        bad = got != want
    rows = np.nonzero(bad.any(axis=1))[0]
    assert rows.size == 0, (tag, "rays that differ", int(rows.size), rows[:8].tolist(),
                            got[rows[:4]].view(np.float32).tolist(), want[rows[:4]].view(np.float32).tolist())


def check_records_against_model(res, ref, tag, nan_as_class=False, width=4, what="points", shown=4):
    """The rule of the gathers: res: structured records (n,); ref: the model's (n, width) f32.  Bit for bit, record by record.
    nan_as_class: in rows where the MODEL has a NaN, NaNs compare as a class; every other row stays bit-exact."""
    got, want = result_words(res, width), u32(ref)
    bad = got != want
    if nan_as_class:
        gf, wf = got.view(np.float32), want.view(np.float32)
        model_nan_row = np.isnan(wf).any(axis=1)
        bad &= ~(np.isnan(gf) & np.isnan(wf) & model_nan_row[:, None])
    rows = np.nonzero(bad.any(axis=1))[0]
    assert rows.size == 0, (tag, what + " that differ", int(rows.size), rows[:8].tolist(),
                            got[rows[:shown]].view(np.float32).tolist(), want[rows[:shown]].view(np.float32).tolist())


def check_counts(stats, counts, n, spp, tag):
    assert stats["rays"] == n and stats["samples"] == n * spp, (tag, stats)
    for k, name in enumerate(COUNT_NAMES):
        assert stats[name] == int(counts[:, k].sum()), (tag, name, stats[name], int(counts[:, k].sum()))
