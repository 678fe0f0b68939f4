"""Shared pieces of the irradiance-gather tests (rt_gather_irradiance): the reference model (tests/model/gather_model.cpp:
the radiance model's translation unit plus the gather stated once on its first-hit and bounce functions), built with the
flags of oracle/Makefile and driven through a ModelRenderer that loads the gather library instead; and the point set of the
GPU tests."""
import ctypes
import functools
import os

import numpy as np

import model_build
import radiance_util as ru
import ray_query_util as rq

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "model", "gather_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libgather_model.so")
COUNT_NAMES = ru.COUNT_NAMES
SEED = ru.SEED


def bind_model(path):
    """a library that holds the gather model's translation unit: every oracle_* and radiance_model_* entry declared as
    radiance_util declares it, plus the two gather_model_* ones"""
    L = ru.bind_model(path)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.gather_model_directions.argtypes = [vp, u32, u32, u32, vp]
    L.gather_model_directions.restype = None
    L.gather_model_gather.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, vp]
    L.gather_model_gather.restype = None
    return L


@functools.lru_cache(maxsize=None)
def model_lib():
    return bind_model(model_build.build(SRC, LIB, ru.FLAGS + ["-shared"]))


class GatherModel(ru.ModelRenderer):
    """ModelRenderer on the gather library: the oracle, traceRadiance / cameraRays, plus gatherDirections / gatherIrradiance"""
    _library = staticmethod(model_lib)

    def gatherDirections(self, points, spp, seed):
        """points (n, 8) f32 in the rt_gather_point layout -> (n, spp, 3) f32: the direction of every sample"""
        p = np.ascontiguousarray(points, dtype=np.float32)
        out = np.empty((p.shape[0], spp, 3), np.float32)
        self.L.gather_model_directions(p.ctypes.data, p.shape[0], spp, seed & 0xffffffff, out.ctypes.data)
        return out

    def gatherIrradiance(self, points, max_depth, spp, seed):
        """-> (out (n, 4) f32 {r, g, b, hit_fraction}, hits (n,) u32, counts (n, 5) u64 COUNT_NAMES)"""
        p = np.ascontiguousarray(points, dtype=np.float32)
        n = p.shape[0]
        out = np.empty((n, 4), np.float32)
        hits = np.empty(n, np.uint32)
        counts = np.empty((n, 5), np.uint64)
        self.L.gather_model_gather(self.ctx, p.ctypes.data, n, max_depth, spp, seed & 0xffffffff, out.ctypes.data,
                                   hits.ctypes.data, counts.ctypes.data)
        return out, hits, counts


model_for = functools.partial(ru.model_for, cls=GatherModel)


def sample_rays(points, dirs, s):
    """the rays {position, t_max, direction of sample s, pad} of every point, in the rt_ray layout"""
    r = np.ascontiguousarray(points, np.float32).copy()
    r[:, 4:7] = dirs[:, s, :]
    return r


def compose(trace, points, dirs, max_depth, spp, seed):
    """The gather as the composition of radiance queries: trace(rays, max_depth, 1, seed * spp + s) -> ((n, 4) f32 {r, g, b,
    t}, extra) for every sample on the given directions; the in-order float32 sum and division.  Returns (out (n, 4) f32,
    hits (n,) u32, [extra of every call])."""
    n = points.shape[0]
    col = np.zeros((n, 3), np.float32)
    hits = np.zeros(n, np.uint32)
    extras = []
    for s in range(spp):
        rays = sample_rays(points, dirs, s)
        res, extra = trace(rays, max_depth, 1, (seed * spp + s) & 0xffffffff)
        extras.append(extra)
        col = col + np.ascontiguousarray(res[:, :3], np.float32)
        with np.errstate(invalid="ignore"):
            hits += (res[:, 3] < rays[:, 3]).astype(np.uint32)
    if spp != 1:
        col = col / np.float32(spp)
    assert col.dtype == np.float32
    out = np.empty((n, 4), np.float32)
    out[:, :3] = col
    out[:, 3] = hits.astype(np.float32) / np.float32(spp)
    return out, hits, extras


def points_from_rays(model, rt_rays):
    """The point set of the GPU tests from rays in the rt_ray layout (pads kept): a ray that hits gives the point
    o + d (0.999 t) with normal -d / |d|, a ray that misses the point o with normal d / |d|; t_max = 1e30."""
    rays = np.ascontiguousarray(rt_rays, np.float32)
    first, _ = model.traceRadiance(rays, 0, 1, 0)
    t = first[:, 3]
    hit = t < rays[:, 3]
    o, d = rays[:, 0:3], rays[:, 4:7]
    unit = d / np.linalg.norm(d.astype(np.float64), axis=1)[:, None].astype(np.float32)
    p = rays.copy()
    p[:, 0:3] = np.where(hit[:, None], o + d * (np.float32(0.999) * t)[:, None], o)
    p[:, 3] = np.float32(1e30)
    p[:, 4:7] = np.where(hit[:, None], -unit, unit)
    return np.ascontiguousarray(p, np.float32)


def scene_points(model, bridge):
    """1 024 points of a scene, pads 7 i + 3"""
    return points_from_rays(model, ru.with_pads(rq.to_rt_rays(rq.scene_rays(bridge, False, 700, 324))))


result_words = ru.result_words                          # IRRADIANCE_DTYPE (n,) -> (n, 4) u32
check_against_model = ru.check_records_against_model    # res: IRRADIANCE_DTYPE (n,); ref: the model's (n, 4) f32
check_counts = ru.check_counts
