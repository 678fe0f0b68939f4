"""Shared pieces of the encode tests (rt_encode_atlas, the last stage of rt_bake_atlas_lightmap): the encoding rule of
include/mi355rt.h "lightmaps" restated in numpy, in float64 and integer arithmetic and without a look at float bit patterns
(the exponent comes from frexp, the scale from ldexp, the bytes from floor: every product of a float32 and a power of two is
exact in float64); the atlas of special values the GPU tests encode; and the host build of the two per-texel functions the
kernel applies (tests/model/encode_model.cpp), built with the flags of oracle/Makefile as the other models are."""
import ctypes
import functools
import os

import numpy as np

import model_build
import radiance_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "model", "encode_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libencode_model.so")
TOP = float(np.float32(2.0 ** 127 - 2.0 ** 103))      # 0x1.fffffep+126f, the largest colour the rule keeps
NAN, INF = float("nan"), float("inf")
F32, F16, RGBE8 = 0, 1, 2


def as_f32(atlas):
    """an (..., 4) f32 array or an array of 16-byte records -> (n, 4) f32, the same bytes"""
    a = np.ascontiguousarray(atlas)
    if a.dtype != np.float32:
        a = a.view(np.float32)
    return a.reshape(-1, 4)


def sanitise(atlas):
    """(n, 3) float64: c' = (c > 0) ? min(c, TOP) : 0; a NaN, a negative value and either zero give 0"""
    with np.errstate(invalid="ignore"):
        c = as_f32(atlas)[:, 0:3].astype(np.float64)
        return np.where(c > 0.0, np.minimum(c, TOP), 0.0)


def biased_exponent(v):
    """the biased exponent field of non-negative float32 values held in float64: 0 for zero and the denormals"""
    m, e = np.frexp(v)                                 # v = m * 2^e, 0.5 <= m < 1: v lies in [2^(e - 1), 2^e)
    return np.where(v >= 2.0 ** -126, e + 126, 0).astype(np.int64)


def encode_rgbe(atlas):
    """-> (n,) uint32 words R | G << 8 | B << 16 | E << 24"""
    a = as_f32(atlas)
    c = sanitise(a)
    b = biased_exponent(c.max(axis=1))
    keep = (a[:, 3] != np.float32(-1.0)) & (b >= 32)   # a NaN w is not -1: encoded
    bytes_ = np.floor(np.ldexp(c, (134 - b)[:, None])).astype(np.int64)
    assert (bytes_[keep] >= 0).all() and (bytes_[keep] <= 255).all()
    word = bytes_[:, 0] | (bytes_[:, 1] << 8) | (bytes_[:, 2] << 16) | ((b + 2) << 24)
    return np.where(keep, word, 0).astype(np.uint32)


def encode_f16(atlas):
    """-> (n, 4) uint16 half bit patterns, numpy's conversion: round to nearest even, overflow to infinity"""
    with np.errstate(over="ignore"):
        return as_f32(atlas).astype(np.float16).view(np.uint16)


def decode_rgbe(words):
    """(n,) words -> (n, 3) float64, (byte + 0.5) * 2^(E - 136); the word 0 is black.  The tests' own decoder, beside the
    package's."""
    w = np.asarray(words, np.uint32).astype(np.int64)
    e = w >> 24
    rgb = np.stack([(w >> s) & 0xff for s in (0, 8, 16)], axis=-1).astype(np.float64)
    return np.where((w != 0)[:, None], (rgb + 0.5) * np.exp2((e - 136).astype(np.float64))[:, None], 0.0)


def f16_is_nan(h):
    h = np.asarray(h, np.uint16)
    return ((h & 0x7c00) == 0x7c00) & ((h & 0x03ff) != 0)


def same_f16(got, want):
    """bit for bit, except that where the model has a NaN any NaN will do"""
    got, want = np.asarray(got, np.uint16).reshape(-1), np.asarray(want, np.uint16).reshape(-1)
    return bool(np.all((got == want) | (f16_is_nan(want) & f16_is_nan(got))))


def ulp(x, k):
    """the float32 k ulps from x"""
    u = np.array([x], np.float32).view(np.uint32).astype(np.int64) + k
    return float(u.astype(np.uint32).view(np.float32)[0])


SPECIAL = [NAN, INF, -INF, -0.0, 0.0, -1.5, 1e-40, -1e-40, ulp(2.0 ** -95, -1), 2.0 ** -95, ulp(2.0 ** -95, 1), TOP, 3.0e38,
           2.0 ** -126, ulp(2.0 ** -126, -1), 1.0, 0.5, 65504.0, 65520.0, 65519.99, 1e5, 2.0 ** -24, 2.0 ** -25, ulp(2.0 ** -25, 1),
           2.0 ** -14, ulp(2.0 ** -14, -1), 255.99998, 2.0 ** 127]


def random_colours(n, seed, binades=60):
    """(n, 3) f32 colours whose magnitudes spread over `binades` binades around 1"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 1.0, (n, 3)) * np.exp2(rng.integers(-binades // 2, binades // 2, (n, 3)))).astype(np.float32)


def special_atlas(width, height, seed):
    """(height, width, 4) f32: random colours over 60 binades with w drawn from {-1, -2, 0.3}; then every special value once
    in each channel of a texel of its own with w = 0.3 (as far as the atlas has room), once as a whole texel, and once
    alone beside two tiny neighbours, so that it is the largest channel where it can be"""
    rng = np.random.default_rng(seed)
    n = width * height
    a = np.empty((n, 4), np.float32)
    a[:, 0:3] = random_colours(n, seed + 1)
    a[:, 3] = rng.choice(np.array([-1.0, -2.0, 0.3], np.float32), n)
    rows = []
    for s in SPECIAL:
        for ch in range(3):
            row = [1e-30, 1e-30, 1e-30, 0.3]
            row[ch] = s
            rows.append(row)
        rows.append([s, s, s, -2.0])
        rows.append([s, 1.0, 0.25, s])
    rows = np.array(rows, np.float32)
    where = rng.permutation(n)[:min(n, len(rows))]
    a[where] = rows[:len(where)]
    return a.reshape(height, width, 4)


@functools.lru_cache(maxsize=None)
def host_lib():
    L = ctypes.CDLL(model_build.build(SRC, LIB, ru.FLAGS + ["-I", os.path.join(REPO, "include"), "-shared"]))
    for f in (L.encode_host_rgbe8, L.encode_host_f16):
        f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        f.restype = None
    return L


def host_rgbe(atlas):
    a = np.ascontiguousarray(as_f32(atlas))
    out = np.empty(len(a), np.uint32)
    host_lib().encode_host_rgbe8(a.ctypes.data, len(a), out.ctypes.data)
    return out


def host_f16(values):
    v = np.ascontiguousarray(values, np.float32).reshape(-1)
    out = np.empty(len(v), np.uint16)
    host_lib().encode_host_f16(v.ctypes.data, len(v), out.ctypes.data)
    return out
