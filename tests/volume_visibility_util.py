"""Shared pieces of the probe-visibility tests (rt_bake_volume_visibility / rt_sample_volume_visible /
rt_encode_volume_visibility): the stand-alone reference model (tests/model/volume_visibility_model.cpp, built with the flags the
other models use), a float64 restatement of the fetch and of the sampler, the maps the known answers are made of, and the maps
and points of the parity tests.

Figures measured on the development host by tests/test_volume_visibility_model.py (it prints them):
  seam continuity (c), size 16, f(d) = 1 + 0.5 d.x + 0.3 d.y - 0.2 d.z against its bilinear fetch from texel centres:
    float64 fetch  worst error with a wrapped tap 0.0303, without 0.0290
    model          worst error with a wrapped tap 0.0303, without 0.0290
  f32 error (d): the largest |model - f64| / max(1, |f64|) over the sampler cases of that test: 4.68e-06"""
import ctypes
import functools
import os

import numpy as np

import model_build
import radiance_util as ru
import volume_util as vu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "model", "volume_visibility_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libvolume_visibility_model.so")
# the largest |f32 - f64| / max(1, |f64|) of the MODEL's visible sampler on the inputs of tests/test_volume_visibility_model.py,
# measured on the development host (the docstring above has the figure), times four: the margin is for other libm / compiler
# versions
FLOAT_TOLERANCE = 4 * 4.68e-6


def _R():
    from webgpu_raytracer_amd import renderer
    return renderer


@functools.lru_cache(maxsize=None)
def model_lib():
    L = ctypes.CDLL(model_build.build(SRC, LIB, ru.FLAGS + ["-I", os.path.join(REPO, "include"), "-shared"]))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.vvis_model_rays.argtypes = [vp, vp, u32, vp]
    L.vvis_model_texels.argtypes = [vp, vp, u32, vp]
    L.vvis_model_wrap.argtypes = [u32, ctypes.c_int, ctypes.c_int]
    L.vvis_model_wrap.restype = u32
    L.vvis_model_fetch.argtypes = [u32, vp, vp, u32, vp, vp]
    L.vvis_model_weights.argtypes = [vp, vp, vp, vp, u32, vp]
    L.vvis_model_sample.argtypes = [vp, vp, vp, vp, vp, u32, vp]
    L.vvis_model_tiles.argtypes = [vp, vp, vp, ctypes.c_int, vp]
    for f in (L.vvis_model_rays, L.vvis_model_texels, L.vvis_model_fetch, L.vvis_model_weights, L.vvis_model_sample,
              L.vvis_model_tiles):
        f.restype = None
    return L


def _descs(desc, vis):
    return np.ascontiguousarray(desc).reshape(()), np.ascontiguousarray(vis).reshape(())


def _maps(desc, vis, maps):
    size = int(np.asarray(vis).reshape(())["size"])
    return np.ascontiguousarray(maps, np.float32).reshape(vu.probe_count(desc), size, size, 2)


def model_rays(desc, vis, seed):
    """-> (n * size * size * spt, 8) f32 in the rt_ray layout, (probe, texel, sample) order"""
    d, v = _descs(desc, vis)
    out = np.empty((vu.probe_count(d) * int(v["size"]) ** 2 * int(v["spt"]), 8), np.float32)
    model_lib().vvis_model_rays(d.ctypes.data, v.ctypes.data, int(seed), out.ctypes.data)
    return out


def model_texels(vis, hits):
    """hits: a RAY_HIT_DTYPE array or (m, 4) words in (texel, sample) order -> (m / spt, 2) f32"""
    v = np.ascontiguousarray(vis).reshape(())
    h = np.ascontiguousarray(hits)
    n = h.size * h.dtype.itemsize // 16 // int(v["spt"])
    out = np.empty((n, 2), np.float32)
    model_lib().vvis_model_texels(v.ctypes.data, h.ctypes.data, n, out.ctypes.data)
    return out


def model_wrap(size, i, j):
    return int(model_lib().vvis_model_wrap(int(size), int(i), int(j)))


def model_fetch(map_, dirs):
    """map_: (size, size, 2) f32; dirs: (n, 3) -> ((n, 2) f32, (n,) bool: a tap was wrapped)"""
    m = np.ascontiguousarray(map_, np.float32)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    out, wrapped = np.empty((d.shape[0], 2), np.float32), np.empty(d.shape[0], np.uint8)
    model_lib().vvis_model_fetch(m.shape[0], m.ctypes.data, d.ctypes.data, d.shape[0], out.ctypes.data, wrapped.ctypes.data)
    return out, wrapped.astype(bool)


def model_weights(desc, vis, maps, points):
    """-> (m, 8) f32: vis_c of every corner, before the product with the trilinear weight"""
    d, v = _descs(desc, vis)
    m = _maps(d, v, maps)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 8)
    out = np.empty((p.shape[0], 8), np.float32)
    model_lib().vvis_model_weights(d.ctypes.data, v.ctypes.data, m.ctypes.data, p.ctypes.data, p.shape[0], out.ctypes.data)
    return out


def model_sample(desc, vis, volume, maps, points):
    """-> (m, 4) f32 {rgb, W}, by the model"""
    d, v = _descs(desc, vis)
    vol = np.ascontiguousarray(volume, np.float32).reshape(vu.probe_count(d), 28)
    m = _maps(d, v, maps)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 8)
    out = np.empty((p.shape[0], 4), np.float32)
    model_lib().vvis_model_sample(d.ctypes.data, v.ctypes.data, vol.ctypes.data, m.ctypes.data, p.ctypes.data, p.shape[0],
                                  out.ctypes.data)
    return out


def model_tiles(desc, vis, maps, f16):
    """-> (ny * nz * (size + 2), nx * (size + 2), 2) f32, or uint16 half bit patterns"""
    d, v = _descs(desc, vis)
    m = _maps(d, v, maps)
    tile = int(v["size"]) + 2
    out = np.empty((int(d["ny"]) * int(d["nz"]) * tile, int(d["nx"]) * tile, 2), np.uint16 if f16 else np.float32)
    model_lib().vvis_model_tiles(d.ctypes.data, v.ctypes.data, m.ctypes.data, int(bool(f16)), out.ctypes.data)
    return out


# ---- float64 restatements
def unpack_f64(px, py):
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    z = 1.0 - np.abs(px) - np.abs(py)
    t = np.clip(-z, 0.0, 1.0)
    x = px + np.where(px >= 0, -t, t)
    y = py + np.where(py >= 0, -t, t)
    v = np.stack([x, y, z], axis=-1)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def pack_f64(v):
    v = np.asarray(v, np.float64)
    p = v[..., :2] / np.abs(v).sum(axis=-1, keepdims=True)
    sx, sy = np.where(p[..., 0] >= 0, 1.0, -1.0), np.where(p[..., 1] >= 0, 1.0, -1.0)
    folded = np.stack([(1.0 - np.abs(p[..., 1])) * sx, (1.0 - np.abs(p[..., 0])) * sy], axis=-1)
    return np.where((v[..., 2] < 0)[..., None], folded, p)


def texel_directions(size):
    """(size, size, 3) float64: the direction of every texel centre, [j, i]"""
    c = (np.arange(size) + 0.5) / size * 2.0 - 1.0
    px, py = np.meshgrid(c, c, indexing="xy")
    return unpack_f64(px, py)


def wrap_f64(i, j, size):
    """the wrap rule on integer arrays: -> (i, j) inside the map, and whether the tap was outside"""
    i, j = np.array(i, np.int64), np.array(j, np.int64)
    outside = (i < 0) | (i >= size) | (j < 0) | (j >= size)
    lo, hi = i < 0, i >= size
    i2 = np.where(lo, -1 - i, np.where(hi, 2 * size - 1 - i, i))
    j2 = np.where(lo | hi, size - 1 - j, j)
    lo, hi = j2 < 0, j2 >= size
    j3 = np.where(lo, -1 - j2, np.where(hi, 2 * size - 1 - j2, j2))
    i3 = np.where(lo | hi, size - 1 - i2, i2)
    return i3, j3, outside


def fetch_f64(maps, dirs):
    """maps: (m, size, size, 2) one map per direction, or (size, size, 2) for all; dirs (m, 3) -> ((m, 2) float64, wrapped)"""
    maps = np.asarray(maps, np.float64)
    size = maps.shape[-2]
    q = pack_f64(dirs)
    u = (q * 0.5 + 0.5) * size - 0.5
    fl = np.clip(np.floor(u), -1, size - 1)
    f = u - fl
    i0, j0 = fl[:, 0].astype(np.int64), fl[:, 1].astype(np.int64)
    rows = np.arange(len(dirs))
    wrapped = np.zeros(len(dirs), bool)
    taps = {}
    for di in (0, 1):
        for dj in (0, 1):
            i, j, out = wrap_f64(i0 + di, j0 + dj, size)
            wrapped |= out
            taps[di, dj] = maps[rows, j, i] if maps.ndim == 4 else maps[j, i]
    a = taps[0, 0] + f[:, 0:1] * (taps[1, 0] - taps[0, 0])
    b = taps[0, 1] + f[:, 0:1] * (taps[1, 1] - taps[0, 1])
    return a + f[:, 1:2] * (b - a), wrapped


def sample_f64(desc, vis, volume, maps, points):
    """The visible sampler in float64 for volumes whose probes are all valid and points that lie on no probe: -> (m, 3)"""
    R = _R()
    desc, vis = np.asarray(desc).reshape(()), np.asarray(vis).reshape(())
    dims = np.array([int(desc["nx"]), int(desc["ny"]), int(desc["nz"])])
    size = int(vis["size"])
    origin, step = np.asarray(desc["origin"], np.float64), np.asarray(desc["step"], np.float64)
    v = np.asarray(volume, np.float64).reshape(dims[2], dims[1], dims[0], 28)[..., :27].reshape(dims[2], dims[1], dims[0], 9, 3)
    m = np.asarray(maps, np.float64).reshape(dims[2], dims[1], dims[0], size, size, 2)
    p = np.asarray(points, np.float64).reshape(-1, 8)
    g = np.clip((p[:, 0:3] - origin) / step, 0.0, dims - 1.0)
    i0 = np.minimum(np.floor(g).astype(np.int64), np.maximum(dims - 2, 0))
    i1 = np.minimum(i0 + 1, dims - 1)
    f = g - i0
    nrm = p[:, 4:7] / np.linalg.norm(p[:, 4:7], axis=1)[:, None]
    Y = R.sh9_basis(nrm)
    B = p[:, 0:3] + nrm * float(vis["normal_bias"])
    E, W = np.zeros((p.shape[0], 3)), np.zeros(p.shape[0])
    for c in range(8):
        d = np.array([c & 1, (c >> 1) & 1, c >> 2])
        at = np.where(d, i1, i0)
        tri = np.prod(np.where(d, f, 1.0 - f), axis=1)
        P = origin + at * step
        e = B - P
        length = np.linalg.norm(e, axis=1)
        safe = np.where(length > 0, length, 1.0)
        mom, _ = fetch_f64(m[at[:, 2], at[:, 1], at[:, 0]], np.where((length > 0)[:, None], e / safe[:, None], [0.0, 0.0, 1.0]))
        var = np.abs(mom[:, 0] ** 2 - mom[:, 1])
        gap = length - mom[:, 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            ch = var / (var + gap * gap)
        ch = np.where(ch > 0, ch, 0.0) ** 3
        w = np.where((length > 0) & ~(length <= mom[:, 0]), np.maximum(ch, float(vis["min_visibility"])), 1.0)
        if int(vis["flags"]) & 1:
            h = P - p[:, 0:3]
            h = h / np.linalg.norm(h, axis=1)[:, None]
            b = ((h * nrm).sum(axis=1) + 1.0) * 0.5
            w = w * (b * b + 0.2)
        crush = float(vis["crush_threshold"])
        if crush > 0:
            w = np.where(w < crush, w ** 3 / crush ** 2, w)
        w = w * tri
        W += w
        E += w[:, None] * np.einsum("mk,mkc->mc", Y, v[at[:, 2], at[:, 1], at[:, 0]])
    return np.maximum(E / W[:, None], 0.0), W


# ---- maps
def constant_maps(desc, vis, D):
    """every texel {D, D * D} in float32"""
    size = int(np.asarray(vis).reshape(())["size"])
    m = np.empty((vu.probe_count(desc), size, size, 2), np.float32)
    m[..., 0] = np.float32(D)
    m[..., 1] = np.float32(D) * np.float32(D)
    return m


def plane_maps(desc, vis, x_w):
    """Zero-variance maps of a scene that is the plane x = x_w alone: per texel the distance from the probe to the plane along
    the texel centre's direction, clamped at max_distance (a direction that never reaches the plane holds max_distance), and
    its square in float32."""
    vis = np.asarray(vis).reshape(())
    size, far = int(vis["size"]), float(vis["max_distance"])
    dirs = texel_directions(size)                                        # (size, size, 3)
    px = vu.numpy_probes(desc)[:, 0].astype(np.float64)                  # (n,)
    gap = (x_w - px)[:, None, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(gap * dirs[None, :, :, 0] > 0, gap / dirs[None, :, :, 0], far)
    t = np.minimum(t, far).astype(np.float32)
    m = np.empty(t.shape + (2,), np.float32)
    m[..., 0] = t
    m[..., 1] = t * t
    assert m.dtype == np.float32
    return m


def random_maps(desc, vis, seed, hostile=True):
    """(n, size, size, 2) f32: mean distances uniform in [0.2, 2) times the smallest step's length scale, second moments m1^2 +
    a variance in [0.01, 0.25).  hostile: a tenth of the texels get zero variance (m2 == m1 * m1 exactly), and a few a NaN, an
    infinite, a negative or a zero word."""
    rng = np.random.default_rng(seed)
    size = int(np.asarray(vis).reshape(())["size"])
    n = vu.probe_count(desc)
    scale = float(np.linalg.norm(np.asarray(np.asarray(desc).reshape(())["step"], np.float64)))
    m1 = rng.uniform(0.2, 2.0, (n, size, size)).astype(np.float32) * np.float32(scale)
    var = rng.uniform(0.01, 0.25, (n, size, size)).astype(np.float32) * np.float32(scale * scale)
    m = np.empty((n, size, size, 2), np.float32)
    m[..., 0] = m1
    m[..., 1] = m1 * m1 + var
    if hostile:
        flat = m.reshape(-1, 2)
        zero = rng.random(len(flat)) < 0.1
        flat[zero, 1] = flat[zero, 0] * flat[zero, 0]
        odd = rng.permutation(len(flat))[:max(10, len(flat) // 40)]        # every value at least once in either word
        vals = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0], np.float32)
        flat[odd, (np.arange(len(odd)) // len(vals)) % 2] = vals[np.arange(len(odd)) % len(vals)]
    return m


def parity_points(desc, n, seed):
    """vu.parity_points - every grid node exactly (len == 0 at one corner), cell centres, points outside on every side,
    non-finite positions, a zero normal - with a NaN normal and an infinite one among them where there is room."""
    p = np.array(vu.parity_points(desc, n, seed))
    if n > 8:
        p[n // 3, 4] = np.nan
        p[n // 3 + 1, 5] = np.inf
    return p
