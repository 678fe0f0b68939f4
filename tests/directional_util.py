"""Shared pieces of the directional-gather tests (rt_gather_directional): the reference model (tests/model/
directional_model.cpp: the radiance model's translation unit plus the directional gather stated once on its first-hit and
bounce functions), built with the flags of oracle/Makefile and driven through a ModelRenderer that loads the directional
library instead; and the numpy restatement of the projection (band 0 .. 1 basis, fixed summation tree) that the composition
tests put behind radiance queries."""
import ctypes
import functools
import os

import numpy as np

import model_build
import probe_util as prb
import radiance_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "model", "directional_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libdirectional_model.so")
COUNT_NAMES = ru.COUNT_NAMES
SEED = ru.SEED
TWO_PI = np.float32(6.283185307)
Y0 = np.float32(0.282094792)
Y1 = np.float32(0.488602512)


@functools.lru_cache(maxsize=None)
def model_lib():
    """the directional library: every oracle_* and radiance_model_* entry declared as radiance_util declares it, plus the
    two directional_model_* ones"""
    L = ru.bind_model(model_build.build(SRC, LIB, ru.FLAGS + ["-shared"]))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.directional_model_directions.argtypes = [vp, u32, u32, u32, vp]
    L.directional_model_directions.restype = None
    L.directional_model_gather.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, vp]
    L.directional_model_gather.restype = None
    return L


class DirectionalModel(ru.ModelRenderer):
    """ModelRenderer on the directional library: the oracle, traceRadiance / cameraRays, plus directions / gatherDirectional"""
    _library = staticmethod(model_lib)

    def directions(self, points, spp, seed):
        """points (n, 8) f32 in the rt_gather_point layout -> (n, spp, 3) f32: the direction of every sample"""
        p = np.ascontiguousarray(points, dtype=np.float32)
        out = np.empty((p.shape[0], spp, 3), np.float32)
        self.L.directional_model_directions(p.ctypes.data, p.shape[0], spp, seed & 0xffffffff, out.ctypes.data)
        return out

    def gatherDirectional(self, points, max_depth, spp, seed):
        """-> (out (n, 16) f32, rt_directional: row k {sh[k].rgb, hit_fraction}; hits (n,) u32; counts (n, 5) u64 COUNT_NAMES)"""
        p = np.ascontiguousarray(points, dtype=np.float32)
        n = p.shape[0]
        out = np.empty((n, 16), np.float32)
        hits = np.empty(n, np.uint32)
        counts = np.empty((n, 5), np.uint64)
        self.L.directional_model_gather(self.ctx, p.ctypes.data, n, max_depth, spp, seed & 0xffffffff, out.ctypes.data,
                                        hits.ctypes.data, counts.ctypes.data)
        return out, hits, counts


model_for = functools.partial(ru.model_for, cls=DirectionalModel)


def make_points(positions, normals, t_max=1e30, pad_step=ru.PAD_STEP, pad_first=ru.PAD_0):
    """(n, 3) positions and normals -> (n, 8) f32 in the rt_gather_point layout, pads pad_step * i + pad_first"""
    pos = np.asarray(positions, np.float32)
    p = np.zeros((pos.shape[0], 8), np.float32)
    p[:, 0:3] = pos
    p[:, 3] = np.float32(t_max)
    p[:, 4:7] = np.asarray(normals, np.float32)
    return ru.with_pads(p, pad_step, pad_first)


def sh4_basis_f32(d):
    """(..., 3) f32 -> (..., 4) f32: bands 0 and 1 of the probe rule's basis, every operation a float32 one"""
    d = np.asarray(d, np.float32)
    Y = np.empty(d.shape[:-1] + (4,), np.float32)
    Y[..., 0] = Y0
    Y[..., 1] = Y1 * d[..., 1]
    Y[..., 2] = Y1 * d[..., 2]
    Y[..., 3] = Y1 * d[..., 0]
    return Y


def project(radiance, dirs, t_max):
    """The projection of the directional rule in numpy float32: radiance (n, spp, 4) f32 {r, g, b, t}, dirs (n, spp, 3) f32,
    t_max (n,) f32 -> (out (n, 16) f32 in the rt_directional layout, hits (n,) u32).  Lane partials in ascending sample order
    from +0, the six butterfly steps, lane 0, rt_div by spp, times 2 pi."""
    rad = np.ascontiguousarray(radiance, np.float32)
    n, spp = rad.shape[:2]
    with np.errstate(invalid="ignore", over="ignore"):
        terms = (rad[:, :, None, :3] * sh4_basis_f32(dirs)[:, :, :, None]).reshape(n, spp, 12)
        assert terms.dtype == np.float32
        P = np.zeros((n, 64, 12), np.float32)
        for s in range(spp):
            P[:, s % 64, :] = P[:, s % 64, :] + terms[:, s, :]
        lanes = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            P = P + P[:, lanes ^ m, :]
        assert P.dtype == np.float32
        hits = (rad[:, :, 3] < np.asarray(t_max, np.float32)[:, None]).sum(axis=1).astype(np.uint32)
        out = np.empty((n, 4, 4), np.float32)
        out[:, :, :3] = ((P[:, 0, :] / np.float32(spp)) * TWO_PI).reshape(n, 4, 3)
        out[:, :, 3] = (hits.astype(np.float32) / np.float32(spp))[:, None]
    return out.reshape(n, 16), hits


def compose(trace, points, dirs, max_depth, spp, seed):
    """The directional gather as the composition of radiance queries on the PLAIN rays: trace(rays, max_depth, 1, f) -> ((n,
    4) f32 {r, g, b, t}, extra) for every sample, then project().  Returns (out, hits, [extra of every call])."""
    points = np.ascontiguousarray(points, np.float32)
    n = points.shape[0]
    rad = np.empty((n, spp, 4), np.float32)
    extras = []
    for s, f in enumerate(prb.sample_frames(spp, seed)):
        res, extra = trace(prb.plain_rays(points, dirs, s), max_depth, 1, int(f))
        rad[:, s, :] = res
        extras.append(extra)
    out, hits = project(rad, dirs, points[:, 3])
    return out, hits, extras


def compose_pad_prime(trace, points, dirs, max_depth, spp, seed):
    """The same through ONE radiance query on the pad' rays at seed = 0, spp = 1.  Returns (out, hits, extra)."""
    points = np.ascontiguousarray(points, np.float32)
    n = points.shape[0]
    res, extra = trace(prb.pad_prime_rays(points, dirs, spp, seed), max_depth, 1, 0)
    out, hits = project(np.ascontiguousarray(res, np.float32).reshape(n, spp, 4), dirs, points[:, 3])
    return out, hits, extra


result_words = functools.partial(ru.result_words, width=16)   # DIRECTIONAL_DTYPE (n,) -> (n, 16) u32
# res: DIRECTIONAL_DTYPE (n,); ref: (n, 16) f32; the rule of the gathers
check_against_model = functools.partial(ru.check_records_against_model, width=16, what="points", shown=2)
check_counts = ru.check_counts
