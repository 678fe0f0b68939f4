"""Shared pieces of the reflection-sampler tests (rt_sample_reflection): the stand-alone reference model
(tests/model/reflection_sample_model.cpp, built with the flags the other models use), an independent float64 restatement of
the rule in numpy, a numpy fold, and the chains, probes, boxes and queries of the tests."""
import ctypes
import functools
import os

import numpy as np

import model_build
import radiance_util as ru
import reflection_util as rf

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "model", "reflection_sample_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libreflection_sample_model.so")


def _R():
    from webgpu_raytracer_amd import renderer
    return renderer


@functools.lru_cache(maxsize=None)
def model_lib():
    L = ctypes.CDLL(model_build.build(SRC, LIB, ru.FLAGS + ["-I", os.path.join(REPO, "include"), "-shared"]))
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.reflection_sample_model.argtypes = [vp, vp, u32, vp, vp, vp, u32, i32, vp]
    L.reflection_sample_model.restype = None
    L.reflection_sample_model_direction.argtypes = [vp, vp, vp, vp, u32, vp]
    L.reflection_sample_model_direction.restype = None
    L.reflection_sample_model_fold.argtypes = [u32, i32, i32]
    L.reflection_sample_model_fold.restype = u32
    L.reflection_sample_model_taps.argtypes = [u32, vp, u32, vp, vp]
    L.reflection_sample_model_taps.restype = None
    return L


def _words(a, dtype):
    """records of `dtype` or (n, 8) float32 -> (n, 8) float32, C-contiguous; None stays None"""
    if a is None:
        return None
    r = np.ascontiguousarray(a)
    if r.dtype == dtype:
        r = r.reshape(-1).view(np.float32)
    return np.ascontiguousarray(r, np.float32).reshape(-1, 8)


def _ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data


def chains_of(desc, chains):
    """-> (n_probes, chain_texels, 4) f32"""
    d = np.ascontiguousarray(desc).reshape(())
    texels = int(rf.level_offsets(int(d["size"]), int(d["levels"]))[-1])
    return np.ascontiguousarray(chains, np.float32).reshape(-1, texels, 4)


def model_sample(desc, chains, queries, probes=None, boxes=None, n_probes=None, clamp=False):
    """-> (n, 4) f32 by the model.  n_probes: how many of the chains the call may use (default: all).  clamp: the clamp-to-edge
    form of the fetch, which is not the rule."""
    R = _R()
    d = np.ascontiguousarray(desc).reshape(())
    c = chains_of(d, chains)
    q = _words(queries, R.REFLECTION_QUERY_DTYPE)
    p, b = _words(probes, R.PROBE_DTYPE), _words(boxes, R.REFLECTION_BOX_DTYPE)
    out = np.full((q.shape[0], 4), -7.0, np.float32)
    model_lib().reflection_sample_model(d.ctypes.data, _ptr(c), c.shape[0] if n_probes is None else n_probes, _ptr(p), _ptr(b),
                                        _ptr(q), q.shape[0], int(clamp), _ptr(out))
    return out


def model_direction(desc, queries, probes=None, boxes=None):
    """-> (n, 3) f32: the direction the fetch packs, d'"""
    R = _R()
    d = np.ascontiguousarray(desc).reshape(())
    q = _words(queries, R.REFLECTION_QUERY_DTYPE)
    p, b = _words(probes, R.PROBE_DTYPE), _words(boxes, R.REFLECTION_BOX_DTYPE)
    out = np.empty((q.shape[0], 3), np.float32)
    model_lib().reflection_sample_model_direction(d.ctypes.data, _ptr(p), _ptr(b), _ptr(q), q.shape[0], _ptr(out))
    return out


def model_fold(S, i, j):
    return int(model_lib().reflection_sample_model_fold(int(S), int(i), int(j)))


def model_taps(S, dirs):
    """-> (index (n, 4) u32, weight (n, 4) f32) of a level of side S, in the order t00, t10, t01, t11"""
    v = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    index, weight = np.empty((v.shape[0], 4), np.uint32), np.empty((v.shape[0], 4), np.float32)
    model_lib().reflection_sample_model_taps(int(S), _ptr(v), v.shape[0], _ptr(index), _ptr(weight))
    return index, weight


# ---- numpy: the fold, and the whole rule in float64
def np_fold(S, i, j):
    """integer arrays i, j in -1 .. S -> (i, j) inside the map, by the rule's two steps"""
    i, j = np.array(i, np.int64), np.array(j, np.int64)
    out = (i < 0) | (i >= S)
    i, j = np.where(out, np.where(i < 0, -1 - i, 2 * S - 1 - i), i), np.where(out, S - 1 - j, j)
    out = (j < 0) | (j >= S)
    j, i = np.where(out, np.where(j < 0, -1 - j, 2 * S - 1 - j), j), np.where(out, S - 1 - i, i)
    return i, j


def direction_f64(desc, queries, probes, boxes):
    R = _R()
    d = np.ascontiguousarray(desc).reshape(())
    q = _words(queries, R.REFLECTION_QUERY_DTYPE)
    dirs = q[:, 4:7].astype(np.float64)
    if not int(d["flags"]) & R.RT_REFLECTION_SAMPLE_PARALLAX:
        return dirs
    pr = q.view(np.uint32)[:, 3].astype(np.int64)
    x = q[:, 0:3].astype(np.float64)
    c = _words(probes, R.PROBE_DTYPE)[pr, 0:3].astype(np.float64)
    bx = _words(boxes, R.REFLECTION_BOX_DTYPE)[pr].astype(np.float64)
    lo, hi = bx[:, 0:3], bx[:, 4:7]
    with np.errstate(all="ignore"):
        inside = ((lo <= x) & (x <= hi)).all(axis=1)
        t = np.where(dirs > 0, (hi - x) / dirs, np.where(dirs < 0, (lo - x) / dirs, np.inf)).min(axis=1)
        use = inside & (t < np.inf)
        bent = x + dirs * t[:, None] - c
    return np.where(use[:, None], bent, dirs)


def sample_f64(desc, chains, queries, probes=None, boxes=None):
    """The rule in float64, vectorised over the queries, written from the header and sharing nothing with the model: (n, 4)
    float64.  For finite chains and probe indices inside the array (a weight of zero is multiplied here, not skipped)."""
    R = _R()
    d = np.ascontiguousarray(desc).reshape(())
    size, levels = int(d["size"]), int(d["levels"])
    c = chains_of(d, chains).astype(np.float64)
    q = _words(queries, R.REFLECTION_QUERY_DTYPE)
    pr = q.view(np.uint32)[:, 3].astype(np.int64)
    v = direction_f64(d, q, probes, boxes)
    s = 1.0 / np.abs(v).sum(axis=1)
    px, py = v[:, 0] * s, v[:, 1] * s
    ox, oy = (1.0 - np.abs(py)) * np.where(px >= 0, 1.0, -1.0), (1.0 - np.abs(px)) * np.where(py >= 0, 1.0, -1.0)
    qx, qy = np.where(v[:, 2] < 0, ox, px), np.where(v[:, 2] < 0, oy, py)
    r = np.clip(np.nan_to_num(q[:, 7].astype(np.float64), nan=0.0), 0.0, 1.0)
    xl = r * (levels - 1)
    m0 = np.minimum(np.floor(xl).astype(np.int64), levels - 2)
    g = xl - m0
    off = rf.level_offsets(size, levels)
    out = np.zeros((q.shape[0], 4))
    for lv, wl in ((m0, 1.0 - g), (m0 + 1, g)):
        S = size >> lv
        u = np.clip((qx * 0.5 + 0.5) * S - 0.5, -0.5, S - 0.5)
        w = np.clip((qy * 0.5 + 0.5) * S - 0.5, -0.5, S - 0.5)
        i0, j0 = np.floor(u).astype(np.int64), np.floor(w).astype(np.int64)
        fx, fy = u - i0, w - j0
        val = np.zeros((q.shape[0], 4))
        for a, b, wt in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
            i, j = np_fold(S, i0 + a, j0 + b)
            val += wt[:, None] * c[pr, off[lv] + j * S + i]
        out += wl[:, None] * val
    return out


# ---- inputs
def make_boxes(lo, hi):
    R = _R()
    lo = np.asarray(lo, np.float32).reshape(-1, 3)
    b = np.zeros(lo.shape[0], R.REFLECTION_BOX_DTYPE)
    b["lo"], b["hi"] = lo, np.asarray(hi, np.float32).reshape(-1, 3)
    return b


def make_probes(positions):
    R = _R()
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    p = np.zeros(pos.shape[0], R.PROBE_DTYPE)
    p["position"], p["t_max"] = pos, 1e30
    return p


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_queries(rng, n, n_probes, lo=-1.0, hi=1.0):
    """n queries with directions uniform on the sphere and of lengths 0.25 .. 4, positions in and a little around [lo, hi]^3,
    roughness over a little more than [0, 1]"""
    R = _R()
    dirs = unit(rng.normal(size=(n, 3))) * rng.uniform(0.25, 4.0, size=(n, 1))
    pos = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), size=(n, 3))
    return R.reflection_queries(pos, rng.integers(0, n_probes, size=n), dirs, rng.uniform(-0.1, 1.1, size=n))


def affine_map(size, coeff=(1.0, 0.5, 0.3, -0.2)):
    """level 0 of a chain: f(d) = c0 + c1 d.x + c2 d.y + c3 d.z of the unit direction of each texel centre, in all four
    channels; (size, size, 4) f32"""
    d = _R().octa_directions(size)
    f = coeff[0] + d @ np.asarray(coeff[1:], np.float64)
    return np.repeat(f[..., None], 4, axis=-1).astype(np.float32)


def chain_from_levels(desc, level0, fill=0.0):
    """one chain whose level 0 is the map and whose other levels hold `fill`; (1, chain_texels, 4) f32"""
    d = np.ascontiguousarray(desc).reshape(())
    size, levels = int(d["size"]), int(d["levels"])
    out = np.full((1, int(rf.level_offsets(size, levels)[-1]), 4), fill, np.float32)
    out[0, :size * size] = np.asarray(level0, np.float32).reshape(size * size, 4)
    return out


def hostile_chains(size, levels, n_probes):
    """chains of rf.special_maps (NaN, infinities, denormals, -0) filtered by the reflection model: (n_probes, chain_texels, 4).
    Of the three maps drawn the second comes first: at size 8 it is the one that holds NaNs."""
    return rf.model_filter(rf.desc(size, levels, 1, 64), rf.special_maps(3, size)[[1, 0, 2][:n_probes]])


def hostile_boxes(n_probes):
    """(probes, boxes): probe 0 in a unit-ish box around it; the last probe's box is degenerate (lo == hi on one axis); with
    three probes the middle one has a box off its centre"""
    pos = np.array([[0.0, 0.0, 0.0], [0.5, 0.25, -0.25], [2.0, 2.0, 2.0]], np.float32)[:n_probes]
    lo = np.array([[-1.0, -1.0, -1.0], [-1.0, -0.5, -2.0], [1.5, 1.5, 2.0]], np.float32)[:n_probes]
    hi = np.array([[1.0, 1.0, 1.0], [3.0, 1.5, 0.5], [2.5, 2.5, 2.0]], np.float32)[:n_probes]
    return make_probes(pos), make_boxes(lo, hi)


def hostile_queries(size, levels, n_probes):
    """The hostile set, three queries per direction, shuffled once (a fixed permutation) so that a prefix of any length is a
    mix of every kind: texel-centre directions of every level, directions on each seam edge, at the four corners and at both
    poles, zero, NaN and infinite directions; roughness in {-1, 0, 0.5, 1, 2, NaN} and two in between; probe indices n_probes
    - 1, 0, n_probes and 0xffffffff; positions inside, outside, on a face of the boxes of hostile_boxes, and NaN."""
    R = _R()
    nan, inf = np.nan, np.inf
    dirs = [R.octa_directions(size >> m).reshape(-1, 3) for m in range(levels)]
    e = 1e-3
    # the four edges of the square are the images of the half planes x = 0 and y = 0 of the lower hemisphere, the corners of -z,
    # the middle of the map of +z, the middles of the edges of -+x and -+y at z = 0 seen from below
    seams = [[0.0, 0.7, -0.7], [0.0, -0.7, -0.7], [0.7, 0.0, -0.7], [-0.7, 0.0, -0.7], [e, 0.7, -0.7], [-e, -0.7, -0.7],
             [0.7, e, -0.7], [-0.7, -e, -0.7], [0.0, 0.0, -1.0], [e, e, -1.0], [-e, e, -1.0], [e, -e, -1.0], [-e, -e, -1.0],
             [0.0, 0.0, 1.0], [e, -e, 1.0], [0.0, 1.0, -0.0], [0.0, -1.0, -e], [1.0, 0.0, -e], [-1.0, 0.0, -0.0],
             [0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [nan, 1.0, 0.0], [1.0, nan, nan], [nan, nan, nan], [inf, 0.0, 0.0],
             [1.0, -inf, 0.5], [inf, inf, -inf], [0.0, 3.0, 0.0], [1e-30, 0.0, -1e-30], [3e38, 3e38, 3e38]]
    dirs = np.concatenate(dirs + [np.array(seams, np.float64)])
    rng = np.random.default_rng(3)
    n = 3 * len(dirs)
    rough = np.array([0.0, 0.5, 1.0, -1.0, 2.0, nan, 0.25, 0.75], np.float32)
    probe = np.array([n_probes - 1] * 4 + [0] * 3 + [n_probes // 2] * 2 + [n_probes, 0xffffffff], np.uint32)
    pos = np.array([[0.5, 0.0, 0.0], [0.25, -0.5, 0.75], [5.0, 0.0, 0.0], [1.0, 0.25, 0.0], [nan, 0.0, 0.0], [0.0, 0.0, 0.0],
                    [2.0, 2.0, 2.0], [2.25, 1.75, 2.0], [-1.0, -1.0, -1.0], [0.0, inf, 0.0]], np.float32)
    # every direction three times, in a shuffled order; position, probe and roughness drawn independently for each query, so
    # that the three meet different ones whatever the number of directions is
    return R.reflection_queries(pos[rng.integers(len(pos), size=n)], probe[rng.integers(len(probe), size=n)],
                                dirs[rng.permutation(n) % len(dirs)], rough[rng.integers(len(rough), size=n)])


def check_words(got, want, tag):
    """bit for bit; where the model has a NaN, a NaN of any payload is equal"""
    rf.check_words(got, want, tag, nan_as_class=True)
