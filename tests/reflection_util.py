"""Shared pieces of the reflection-probe tests (rt_capture_reflection / rt_filter_reflection / rt_bake_reflection): the reference
model (tests/model/reflection_model.cpp: the radiance model's translation unit plus the capture stated once on its first-hit
and bounce functions, and the filter stated on the two public headers alone), built with the flags of oracle/Makefile and
driven through a ModelRenderer that loads the reflection library instead; the numpy restatement of the texel side of the filter
(octahedral mapping, frame, lookup, fixed summation tree) on the model's exported lobe; a float64 evaluation of the lobe; and
the descriptors, probes and rays of the tests."""
import ctypes
import functools
import os

import numpy as np

import model_build
import probe_util as prb
import radiance_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "model", "reflection_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libreflection_model.so")
SEED = ru.SEED
DESC_DTYPE = np.dtype([("size", np.uint32), ("levels", np.uint32), ("spt", np.uint32), ("filter_samples", np.uint32),
                       ("reserved", np.uint32, (4,))])

def desc(size, levels, spt=1, filter_samples=64):
    d = np.zeros((), DESC_DTYPE)
    d["size"], d["levels"], d["spt"], d["filter_samples"] = size, levels, spt, filter_samples
    return d


def level_offsets(size, levels):
    sides = np.array([size >> m for m in range(levels)], np.int64)
    return np.concatenate([[0], np.cumsum(sides * sides)])


@functools.lru_cache(maxsize=None)
def model_lib():
    """the reflection library: every oracle_* and radiance_model_* entry declared as radiance_util declares it, plus the
    reflection_model_* ones"""
    L = ru.bind_model(model_build.build(SRC, LIB, ru.FLAGS + ["-shared"]))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.reflection_model_directions.argtypes = [vp, u32, u32, u32, u32, vp]
    L.reflection_model_directions.restype = None
    L.reflection_model_capture.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp]
    L.reflection_model_capture.restype = None
    L.reflection_model_filter.argtypes = [vp, vp, u32, vp]
    L.reflection_model_filter.restype = None
    L.reflection_model_lobe.argtypes = [u32, u32, u32, vp, vp]
    L.reflection_model_lobe.restype = None
    L.reflection_model_centres.argtypes = [u32, vp]
    L.reflection_model_centres.restype = None
    return L


def model_filter(d, maps):
    """maps (n, size, size, 4) f32 -> chains (n, chain_texels, 4) f32 by the model; no scene"""
    L = model_lib()
    m = np.ascontiguousarray(maps, np.float32)
    n = m.shape[0]
    out = np.empty((n, int(level_offsets(int(d["size"]), int(d["levels"]))[-1]), 4), np.float32)
    L.reflection_model_filter(d.ctypes.data, m.ctypes.data, n, out.ctypes.data)
    return out


def model_lobe(level, levels, K):
    """-> (l_t (K, 3) f32, sum_w f32) of a level as the model's filter forms them"""
    lt = np.empty((K, 3), np.float32)
    sw = np.empty(1, np.float32)
    model_lib().reflection_model_lobe(level, levels, K, lt.ctypes.data, sw.ctypes.data)
    return lt, sw[0]


def model_centres(size):
    out = np.empty((size, size, 3), np.float32)
    model_lib().reflection_model_centres(size, out.ctypes.data)
    return out


class ReflectionModel(ru.ModelRenderer):
    """ModelRenderer on the reflection library: the oracle, traceRadiance, plus the capture"""
    _library = staticmethod(model_lib)

    def reflectionDirections(self, probes, size, spt, seed):
        """-> (n, size * size, spt, 3) f32: the direction of every sample of every texel"""
        p = np.ascontiguousarray(probes, dtype=np.float32)
        out = np.empty((p.shape[0], size * size, spt, 3), np.float32)
        self.L.reflection_model_directions(p.ctypes.data, p.shape[0], size, spt, seed & 0xffffffff, out.ctypes.data)
        return out

    def captureReflection(self, d, probes, max_depth, seed):
        """-> (maps (n, size, size, 4) f32, counts (5,) u64 COUNT_NAMES, the sums over the call)"""
        p = np.ascontiguousarray(probes, dtype=np.float32)
        n, size = p.shape[0], int(d["size"])
        out = np.empty((n, size, size, 4), np.float32)
        counts = np.empty(5, np.uint64)
        self.L.reflection_model_capture(self.ctx, d.ctypes.data, p.ctypes.data, n, max_depth, seed & 0xffffffff, out.ctypes.data,
                                        counts.ctypes.data)
        return out, counts


model_for = functools.partial(ru.model_for, cls=ReflectionModel)


def texel_rays(probes, dirs, s):
    """the plain rays {position, t_max, direction of sample s, pad + t} of every texel of every probe, (n * size^2, 8) f32"""
    p = np.ascontiguousarray(probes, np.float32)
    n, texels = dirs.shape[:2]
    r = np.repeat(p, texels, axis=0)
    r[:, 4:7] = dirs[:, :, s, :].reshape(n * texels, 3)
    pads = np.repeat(p.view(np.uint32)[:, 7].astype(np.uint64), texels) + np.tile(np.arange(texels, dtype=np.uint64), n)
    r.view(np.uint32)[:, 7] = pads.astype(np.uint32)
    return r


def compose_capture(trace, probes, dirs, max_depth, spt, seed):
    """The capture as the composition of radiance queries on the plain rays: trace(rays, max_depth, 1, f) -> (m, 4) f32 {r, g,
    b, t} for every sample; then the rule's mean in numpy float32.  -> (n, size, size, 4) f32"""
    p = np.ascontiguousarray(probes, np.float32)
    n, texels = dirs.shape[:2]
    size = int(round(texels ** 0.5))
    t_max = np.repeat(p[:, 3], texels)
    col = np.zeros((n * texels, 3), np.float32)
    hits = np.zeros(n * texels, np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s, f in enumerate(prb.sample_frames(spt, seed)):
            res = np.ascontiguousarray(trace(texel_rays(p, dirs, s), max_depth, 1, int(f)), np.float32).reshape(-1, 4)
            col = col + res[:, :3]
            hits += (res[:, 3] < t_max)
        if spt != 1:
            col = col / np.float32(spt)
        out = np.empty((n * texels, 4), np.float32)
        out[:, :3] = col
        out[:, 3] = hits.astype(np.float32) / np.float32(spt)
    assert col.dtype == np.float32
    return out.reshape(n, size, size, 4)


# ---- the texel side of the filter in numpy float32, every operation in the order of the rule
F = np.float32


def _normalize(x, y, z):
    inv = F(1.0) / np.sqrt(x * x + y * y + z * z)      # rt_rsqrt: two roundings
    return x * inv, y * inv, z * inv


def np_unpack(px, py):
    px, py = np.asarray(px, F), np.asarray(py, F)
    nz = F(1.0) - np.abs(px) - np.abs(py)
    t = np.minimum(np.maximum(-nz, F(0.0)), F(1.0))
    nx = px + np.where(px >= 0, -t, t)
    ny = py + np.where(py >= 0, -t, t)
    return _normalize(nx, ny, nz)


def np_pack(x, y, z):
    s = F(1.0) / (np.abs(x) + np.abs(y) + np.abs(z))
    px, py = x * s, y * s
    ox = (F(1.0) - np.abs(py)) * np.where(px >= 0, F(1.0), F(-1.0))
    oy = (F(1.0) - np.abs(px)) * np.where(py >= 0, F(1.0), F(-1.0))
    return np.where(z < 0, ox, px), np.where(z < 0, oy, py)


def np_filter(d, maps):
    """The filter in numpy: the lobe (l_t per level and sample) from the model's export, everything that depends on the texel
    restated here.  maps (n, size, size, 4) f32 -> chains (n, chain_texels, 4) f32"""
    size, levels, K = int(d["size"]), int(d["levels"]), int(d["filter_samples"])
    m = np.ascontiguousarray(maps, np.float32)
    n = m.shape[0]
    off = level_offsets(size, levels)
    out = np.empty((n, int(off[-1]), 4), np.float32)
    out[:, :size * size] = m.reshape(n, size * size, 4)
    lanes = np.arange(64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for lv in range(1, levels):
            S = size >> lv
            lt, _ = model_lobe(lv, levels, K)
            c = (np.arange(S, dtype=F) + F(0.5)) / F(S) * F(2.0) - F(1.0)
            cx, cy = np.meshgrid(c, c, indexing="xy")                  # [j, i]
            nx, ny, nz = (a.reshape(-1) for a in np_unpack(cx, cy))
            sign = np.where(nz >= 0, F(1.0), F(-1.0))
            a = -(F(1.0) / (sign + nz))
            b = nx * ny * a
            u = (F(1.0) + sign * nx * nx * a, sign * b, -sign * nx)
            v = (b, sign + ny * ny * a, -ny)
            w = (nx, ny, nz)
            P = np.zeros((n, S * S, 64, 5), np.float32)
            for s in range(K):
                tx, ty, tz = lt[s]
                if not tz > 0:
                    continue                                           # five terms +0: the partial stays as it is
                l = [(tx * u[k] + ty * v[k]) + tz * w[k] for k in range(3)]
                qx, qy = np_pack(*l)
                idx = []
                for q in (qx, qy):
                    uu = (q * F(0.5) + F(0.5)) * F(size)
                    uu = np.where(uu > 0, uu, F(0.0))
                    idx.append(np.minimum(np.floor(uu).astype(np.int64), size - 1))
                texel = m[:, idx[1], idx[0], :]                        # (n, S*S, 4)
                term = np.concatenate([tz * texel, np.full((n, S * S, 1), tz, F)], axis=2)
                assert term.dtype == np.float32
                P[:, :, s % 64, :] = P[:, :, s % 64, :] + term
            for mm in (32, 16, 8, 4, 2, 1):
                P = P + P[:, :, lanes ^ mm, :]
            tot = P[:, :, 0, :]
            res = np.where(tot[:, :, 4:5] > 0, tot[:, :, :4] / tot[:, :, 4:5], F(0.0))
            out[:, off[lv]:off[lv + 1]] = res.astype(np.float32)
    return out


def lobe_f64(level, levels, K):
    """l_t (K, 3) and sum_w of a level by the same formulas in float64 with numpy's sin / cos / sqrt"""
    a = level / (levels - 1.0)
    s = np.arange(K, dtype=np.uint32)
    rev = np.zeros(K, np.uint32)
    for b in range(32):
        rev |= ((s >> np.uint32(b)) & np.uint32(1)) << np.uint32(31 - b)
    ux = (s.astype(np.float64) + 0.5) / K
    uy = (rev >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    phi = 2.0 * np.pi * ux
    cos_t = np.sqrt(np.maximum(0.0, (1.0 - uy) / (1.0 + (a * a - 1.0) * uy)))
    sin_t = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
    h = np.stack([sin_t * np.cos(phi), sin_t * np.sin(phi), cos_t], axis=1)
    lt = np.stack([2.0 * h[:, 2] * h[:, 0], 2.0 * h[:, 2] * h[:, 1], 2.0 * h[:, 2] * h[:, 2] - 1.0], axis=1)
    return lt, float(np.where(lt[:, 2] > 0, lt[:, 2], 0.0).sum())


def special_maps(n, size, seed=11):
    """n maps of positive radiance with NaN, +-inf, denormals, -0 and large values scattered over them"""
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.0, 4.0, size=(n, size, size, 4)).astype(np.float32)
    m[..., 3] = rng.uniform(0.0, 1.0, size=(n, size, size)).astype(np.float32)
    flat = m.reshape(-1)
    specials = np.array([np.nan, np.inf, -np.inf, 1e-45, -1e-42, -0.0, 3e38, -3e38], np.float32)
    where = rng.choice(flat.size, size=max(8, flat.size // 40), replace=False)
    flat[where] = specials[np.arange(where.size) % specials.size]
    return m


def check_words(got, want, tag, nan_as_class=False):
    """(..., 4) f32 against (..., 4) f32, bit for bit, texel by texel.  nan_as_class: where the REFERENCE has a NaN, a NaN of
    any payload is equal; every other word stays bit-exact."""
    g = np.ascontiguousarray(got, np.float32).reshape(-1, 4)
    w = np.ascontiguousarray(want, np.float32).reshape(-1, 4)
    assert g.shape == w.shape, (tag, g.shape, w.shape)
    bad = g.view(np.uint32) != w.view(np.uint32)
    if nan_as_class:
        bad &= ~(np.isnan(g) & np.isnan(w))
    rows = np.nonzero(bad.any(axis=1))[0]
    assert rows.size == 0, (tag, "texels that differ", int(rows.size), rows[:8].tolist(), g[rows[:3]].tolist(), w[rows[:3]].tolist())
