"""Shared pieces of the lightmap-bake tests (rt_bake_points / rt_bake_irradiance): the reference model (tests/model/
bake_model.cpp: the gather model's translation unit plus the texel rule of include/mi355rt.h restated once for the CPU),
built with the flags of oracle/Makefile and driven through a GatherModel that loads the bake library instead; a bake of the
model is its points followed by its gather.  Also grid_uv, an override UV layout with one triangle per grid cell."""
import ctypes
import functools
import math
import os

import numpy as np

import gather_util as gu
import model_build
import radiance_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "model", "bake_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libbake_model.so")
SEED = gu.SEED


class BakeDesc(ctypes.Structure):
    """rt_bake_desc"""
    _fields_ = [("inst", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("pad_base", ctypes.c_uint32),
                ("t_max", ctypes.c_float), ("reserved", ctypes.c_uint32 * 3)]


@functools.lru_cache(maxsize=None)
def model_lib():
    """the bake library: everything gather_util declares on its own, plus bake_model_points"""
    L = gu.bind_model(model_build.build(SRC, LIB, ru.FLAGS + ["-shared"]))
    vp = ctypes.c_void_p
    L.bake_model_points.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.bake_model_points.restype = ctypes.c_uint32
    return L


class BakeModel(gu.GatherModel):
    """GatherModel on the bake library, plus bakePoints / bakeIrradiance"""
    _library = staticmethod(model_lib)

    def bakePoints(self, inst, width, height, t_max=1e30, pad_base=0, atlas_uv=None, weights=False):
        """-> (points (n, 8) f32 in the rt_gather_point layout, texels (n,) u32, owner (height, width) i32); weights=True:
        a fourth item, (n, 2) f32, the barycentric weights (bu, bv) of every point"""
        d = BakeDesc(int(inst), int(width), int(height), int(pad_base), float(t_max))
        uv = None if atlas_uv is None else np.ascontiguousarray(atlas_uv, np.float32)
        points = np.empty((width * height, 8), np.float32)
        texels = np.empty(width * height, np.uint32)
        owner = np.empty((height, width), np.int32)
        wts = np.empty((width * height, 2), np.float32)
        n = self.L.bake_model_points(self.ctx, ctypes.addressof(d), None if uv is None else uv.ctypes.data, points.ctypes.data,
                                     texels.ctypes.data, owner.ctypes.data, wts.ctypes.data)
        assert n != 0xffffffff, "no such instance, or no draw commands"
        out = (points[:n].copy(), texels[:n].copy(), owner)
        return out + (wts[:n].copy(),) if weights else out

    def bakeIrradiance(self, inst, width, height, max_depth, spp, seed, t_max=1e30, pad_base=0, atlas_uv=None):
        """model points, then the model gather on them, scattered: -> (atlas (height, width, 4) f32 with {0, 0, 0, -1} in
        uncovered texels, points, texels, counts (n, 5) u64 of the gather)"""
        points, texels, _ = self.bakePoints(inst, width, height, t_max, pad_base, atlas_uv)
        atlas = np.zeros((width * height, 4), np.float32)
        atlas[:, 3] = -1.0
        counts = np.zeros((0, 5), np.uint64)
        if len(points):
            res, _, counts = self.gatherIrradiance(points, max_depth, spp, seed)
            atlas[texels] = res
        return atlas.reshape(height, width, 4), points, texels, counts


model_for = functools.partial(ru.model_for, cls=BakeModel)


def instance_triangles(bridge, inst):
    """(first, count) of the global triangles of TLAS-order instance `inst`, from its draw command"""
    dc = np.asarray(bridge.draw_commands, np.uint32).reshape(-1, 4)[inst]
    return int(dc[2]) // 3, int(dc[0]) // 3


def grid_uv(bridge, inst):
    """An override layout, (vertex_count, 2) f32: triangle k of the instance gets cell k of a ceil(sqrt(n)) grid of the unit
    square, as the triangle (0.11, 0.13) (0.89, 0.12) (0.12, 0.87) of its cell (no edge along a row, a column or a diagonal
    of texel centres) - unique charts with gaps between them.  Every
    vertex no triangle of the instance uses lies at (-1, -1).  (Built for meshes whose triangles share no vertices across
    cells; a shared vertex keeps the cell of the last triangle that names it.)"""
    first, count = instance_triangles(bridge, inst)
    topo = np.asarray(bridge.mesh_topology, np.uint32).reshape(-1, 20)
    n_verts = np.asarray(bridge.uvs).size // 2
    uv = np.full((n_verts, 2), -1.0, np.float32)
    g = max(1, math.ceil(math.sqrt(max(count, 1))))
    corner = np.array([[0.11, 0.13], [0.89, 0.12], [0.12, 0.87]])
    for j in range(min(count, len(topo) - first)):
        cell = np.array([j % g, j // g], np.float64)
        uv[topo[first + j, 0:3]] = ((cell + corner) / g).astype(np.float32)
    return uv


# ---- hand-worked cases: a few triangles with written-out answers, laid over the first triangles of an instance
QUAD = [[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]]   # add_quad's uvs (0,0) (1,0) (1,1) (0,1): triangles (0,1,2), (0,2,3)
NAN, INF = float("nan"), float("inf")


def hand_cases():
    """name -> (uvs of the case's triangles (n, 3, 2), width, height, expected owner map as nested lists: the index of the
    owning triangle WITHIN the case, -1 = none)"""
    def diag(n):
        return [[0 if x >= y else 1 for x in range(n)] for y in range(n)]
    upper = [[0 if x >= y else -1 for x in range(8)] for y in range(8)]
    none8 = [[-1] * 8 for _ in range(8)]
    right = [(0, 0), (1, 0), (1, 1)]
    return {
        # the diagonal passes through the centres x == y, where E == 0 exactly for both triangles: the lower index owns them,
        # and every texel is covered once
        "quad_diagonal": (QUAD, 8, 8, diag(8)),
        "whole_atlas": ([[(-1, -1), (3, -1), (-1, 3)]], 5, 3, [[0] * 5 for _ in range(3)]),
        # texel-space 1.04 .. 1.44: between the centres 0.5 and 1.5
        "misses_every_centre": ([[(0.13, 0.13), (0.18, 0.13), (0.13, 0.18)]], 8, 8, none8),
        "zero_area": ([[(0, 0), (0.5, 0.5), (1, 1)]], 8, 8, none8),
        "duplicate": ([right, right], 8, 8, upper),
        "other_winding": ([[(0, 0), (1, 1), (1, 0)]], 8, 8, upper),
        # 0.3125 * 8 = 2.5: vertex a is the centre of texel (2, 2); the box ends below the next centres
        "vertex_on_a_centre": ([[(0.3125, 0.3125), (0.4, 0.33), (0.33, 0.4)]], 8, 8,
                               [[0 if (x, y) == (2, 2) else -1 for x in range(8)] for y in range(8)]),
        "nan_uv": ([[(NAN, 0), (1, 0), (1, 1)]], 8, 8, none8),
        "inf_uv": ([[(INF, 0), (1, 0), (1, 1)], [(0, -INF), (1, 0), (1, 1)]], 8, 8, none8),
        "huge_uv": ([[(3e38, 0), (1, 0), (1, 1)]], 8, 8, none8),
        "1x1": (QUAD, 1, 1, [[0]]),
        # the diagonal y = 9 x meets the column of centres x = 0.5 at y = 4.5, the centre of texel 4: triangle 0 up to there
        "1x9": (QUAD, 1, 9, [[0]] * 5 + [[1]] * 4),
        "9x1": (QUAD, 9, 1, [[1] * 4 + [0] * 5]),
    }


def hand_uv(bridge, inst, tri_uvs):
    """an override layout that gives the first triangles of the instance the uvs of a hand-worked case and every other
    vertex (-1, -1): those triangles have no area and cover nothing.  For meshes whose triangles share no vertices."""
    first, count = instance_triangles(bridge, inst)
    topo = np.asarray(bridge.mesh_topology, np.uint32).reshape(-1, 20)
    tri_uvs = np.asarray(tri_uvs, np.float32)
    assert len(tri_uvs) <= count
    uv = np.full((np.asarray(bridge.uvs).size // 2, 2), -1.0, np.float32)
    for j, t in enumerate(tri_uvs):
        uv[topo[first + j, 0:3]] = t
    return uv
