"""Shared pieces of the frame-denoise tests (rt_denoise_frame): the reference model (tests/model/frame_denoise_model.cpp: prepare,
one pass, finish and a call in plain loops), built with the flags of oracle/Makefile as the other models are; the synthetic
G-buffer generator (surfaces facing a pinhole camera at the origin); a numpy restatement of the h-only pass; the "specials"
accumulator; and the cornell renders of the oracle the quality gate uses."""
import ctypes
import functools
import os

import numpy as np

import model_build
import radiance_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "model", "frame_denoise_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libframe_denoise_model.so")
DEMODULATE, SAME_INSTANCE = 1, 2
U = 2.0 ** -24   # unit roundoff of f32
F = np.float32
DESC_DTYPE = np.dtype([("passes", "<u4"), ("step", "<u4"), ("flags", "<u4"), ("normal_cos", "<f4"), ("plane_eps", "<f4"),
                       ("sigma_lum", "<f4"), ("reserved", "<u4", (2,))])
# the documented parameters of the cornell quality gate and of the GPU tests on cornell
CORNELL = dict(passes=4, step=1, flags=DEMODULATE, normal_cos=0.9, plane_eps=0.02, sigma_lum=4.0)


@functools.lru_cache(maxsize=None)
def model_lib():
    L = ctypes.CDLL(model_build.build(SRC, LIB, ru.FLAGS + ["-I", os.path.join(REPO, "include"), "-shared"]))
    vp, u32, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
    L.fd_model_prepare.argtypes = [vp, vp, vp, vp, vp, u32, vp, vp, vp]
    L.fd_model_prepare.restype = None
    L.fd_model_pass.argtypes = [vp, vp, u32, u32, u32, u32, f32, f32, f32, vp, vp, vp, vp]
    L.fd_model_pass.restype = None
    L.fd_model_finish.argtypes = [vp, vp, ctypes.c_uint64, vp]
    L.fd_model_finish.restype = None
    L.fd_model_call.argtypes = [vp] * 7
    L.fd_model_call.restype = ctypes.c_int
    return L


def desc(**kw):
    d = np.zeros(1, DESC_DTYPE)
    for k, v in kw.items():
        d[k] = v
    return d


def uniforms(width, height, jitter=(0.0, 0.0), eye=(0.0, 0.0, 0.0)):
    """a 256-byte uniform block: pinhole at `eye` looking down -z, the image plane z = -1 spanning [-1, 1]^2 (focal length 1,
    so z_view is the distance along -z)"""
    u = np.zeros(64, np.float32)
    e = np.asarray(eye, np.float32)
    u[0:3] = e
    u[4:7] = e + np.array([-1, -1, -1], np.float32)
    u[8:11] = (2, 0, 0)
    u[12:15] = (0, 2, 0)
    w = u.view(np.uint32)
    w[53], w[54] = width, height        # @212, @216
    u[56], u[57] = jitter               # @224
    return u.view(np.uint8)


def depth_of(z_view):
    """the clip depth k_primary_visibility stores for z_view, in its f32 arithmetic"""
    z = np.asarray(z_view, F)
    zn, zf = F(0.001), F(10000.0)
    zc = z * (zf / (zf - zn)) - (zf * zn) / (zf - zn)
    return (zc / z).astype(F)


class Frame:
    """the inputs of a call: accum (H, W, 4) f32, albedo (H, W) u32, normal_id (H, W, 4) f32, depth (H, W) f32, uniforms"""

    def __init__(self, width, height, *, z=2.0, oct_normal=(0.0, 0.0), inst=0, albedo=0xff808080, rgb=1.0, weight=1.0,
                 jitter=(0.0, 0.0)):
        self.W, self.H = width, height
        self.accum = np.empty((height, width, 4), F)
        self.accum[..., 0:3] = rgb
        self.accum[..., 3] = weight
        self.albedo = np.full((height, width), albedo, np.uint32)
        self.normal_id = np.zeros((height, width, 4), F)
        self.normal_id[..., 0:2] = oct_normal
        self.normal_id[..., 3] = np.full((height, width), inst, np.uint32).view(F)
        self.depth = np.broadcast_to(depth_of(z), (height, width)).astype(F).copy()
        self.uniforms = uniforms(width, height, jitter)

    def background(self, mask):
        """turn the pixels of `mask` into misses, with the G-buffer's miss values"""
        self.albedo[mask] = 0
        self.normal_id[mask] = 0.0
        self.depth[mask] = 1.0
        return self

    def args(self):
        for a in ("accum", "albedo", "normal_id", "depth", "uniforms"):
            setattr(self, a, np.ascontiguousarray(getattr(self, a)))
        return [a.ctypes.data for a in (self.accum, self.albedo, self.normal_id, self.depth, self.uniforms)]

    def radiance(self):
        """get_radiance of every pixel in f32"""
        a = self.accum
        with np.errstate(all="ignore"):
            return np.where((a[..., 3] <= 0)[..., None], F(0), a[..., 0:3] / a[..., 3:4]).astype(F)


def prepare(fr, flags):
    """-> col (H, W, 4), guide (H, W, 8), mod (H, W, 4), all f32"""
    col = np.empty((fr.H, fr.W, 4), F)
    guide = np.empty((fr.H, fr.W, 8), F)
    mod = np.empty((fr.H, fr.W, 4), F)
    model_lib().fd_model_prepare(*fr.args(), int(flags), col.ctypes.data, guide.ctypes.data, mod.ctypes.data)
    return col, guide, mod


def one_pass(col, guide, step, *, flags=0, normal_cos=0.9, plane_eps=0.02, sigma_lum=0.0, extremes=False):
    """-> out (H, W, 4) f32 [, lo (H, W, 3), hi (H, W, 3), accepted (H, W) u32]"""
    col, guide = np.ascontiguousarray(col, F), np.ascontiguousarray(guide, F)
    H, W = col.shape[:2]
    out = np.empty_like(col)
    lo, hi, acc = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F), np.zeros((H, W), np.uint32)
    model_lib().fd_model_pass(col.ctypes.data, guide.ctypes.data, W, H, int(step), int(flags), float(normal_cos), float(plane_eps),
                              float(sigma_lum), out.ctypes.data, lo.ctypes.data if extremes else None,
                              hi.ctypes.data if extremes else None, acc.ctypes.data if extremes else None)
    return (out, lo, hi, acc) if extremes else out


def finish(col, mod):
    col, mod = np.ascontiguousarray(col, F), np.ascontiguousarray(mod, F)
    out = np.empty_like(col)
    model_lib().fd_model_finish(col.ctypes.data, mod.ctypes.data, col.shape[0] * col.shape[1], out.ctypes.data)
    return out


def call(fr, d):
    """a whole call by the model -> (H, W, 4) f32; d: a DESC_DTYPE record or a dict of its fields"""
    d = desc(**d) if isinstance(d, dict) else np.ascontiguousarray(d, DESC_DTYPE)
    out = np.empty((fr.H, fr.W, 4), F)
    assert model_lib().fd_model_call(*fr.args(), d.ctypes.data, out.ctypes.data) == 0, "the model refuses this descriptor"
    return out


def words(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def differing(got, want):
    """(H, W) bool: the pixels in which some word differs - where the model's word is a NaN the other's need only be a NaN"""
    g, w = words(got), words(want)
    with np.errstate(invalid="ignore"):
        both_nan = np.isnan(np.asarray(got, F)) & np.isnan(np.asarray(want, F))
    return ((g != w) & ~both_nan).any(axis=-1)


KW = (0.375, 0.25, 0.0625)


def numpy_pass(col, ok_of_tap, step):
    """The h-only pass in numpy, f32, sums in visiting order: one masked accumulation per tap.  ok_of_tap(dx, dy, inside) ->
    (H, W) bool of the pixels that accept the tap (dx, dy) beyond `inside`.  -> (H, W, 4) f32 for surface pixels everywhere."""
    col = np.asarray(col, F)
    H, W = col.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    acc = np.zeros((H, W, 4), F)
    wsum = np.zeros((H, W), F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            h = F(KW[abs(dx)]) * F(KW[abs(dy)])
            qx, qy = xs + dx * step, ys + dy * step
            inside = (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
            ok = ok_of_tap(dx, dy, inside) & inside
            c = col[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
            with np.errstate(all="ignore"):
                t = acc.copy()
                t[..., 0:3] = acc[..., 0:3] + h * c[..., 0:3]
                t[..., 3] = acc[..., 3] + (h * h) * c[..., 3]
                acc = np.where(ok[..., None], t, acc)
                wsum = np.where(ok, wsum + h, wsum)
    with np.errstate(all="ignore"):
        out = np.empty_like(acc)
        out[..., 0:3] = acc[..., 0:3] / wsum[..., None]
        out[..., 3] = acc[..., 3] / (wsum * wsum)
    return out


SPECIALS = np.array([0x7fc00000, 0x7f800001, 0xffc12345, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x00400000, 0x0,
                     0x80000000, 0xbf800000], np.uint32)


def specials(accum):
    """a copy of the accumulator with special values - NaNs, infinities, denormals, both zeros, -1, in colours and in weights -
    at the corners, on the 32- and 8-pixel tile seams and on the last row and column"""
    a = np.array(accum, F)
    H, W = a.shape[:2]
    w = a.view(np.uint32)
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    spots += [(y, x) for y in range(H) for x in (31, 32, 63, 64) if x < W and y % 3 == 0]
    spots += [(y, x) for x in range(W) for y in (7, 8, 15, 16) if y < H and x % 5 == 0]
    spots += [(H - 1, x) for x in range(0, W, 4)] + [(y, W - 1) for y in range(0, H, 4)]
    for k, (y, x) in enumerate(spots):
        w[y, x, k % 4] = SPECIALS[k % len(SPECIALS)]
        w[y, x, 3 if k % 3 == 0 else (k + 1) % 4] = SPECIALS[(k * 7 + 3) % len(SPECIALS)]
    return a


_cornell = {}


def cornell_oracle(W, oracle_lib, size=64, depth=4):
    """cornell at size x size by the CPU oracle: {"noisy": 4 spp, "clean": 512 spp} accumulators as read back, the G-buffer
    and the uniform block of the 4-spp frame.  Rendered once per process."""
    key = (size, depth)
    if key in _cornell:
        return _cornell[key]
    import parity_util as pu
    b = pu.bridge_for(W, "cornell")
    out = {}
    for name, spp, frames in (("noisy", 4, 1), ("clean", 64, 8)):
        o = oracle_lib.OracleRenderer()
        o.buildPipeline(depth, spp)
        W.upload_scene(o, b, size, size)
        for f in range(1, frames + 1):
            o.compute(f)
        out[name] = o.readAccum()
        if name == "noisy":
            out["gbuffer"] = o.readGBuffer()
            out["uniforms"] = o.readUniforms()
    _cornell[key] = out
    return out


def frame_of(accum, gbuffer, uniforms_block):
    """a Frame from read-backs: accum (H, W, 4), (albedo (H, W, 4) u8, normal_id, depth), the 256-byte block"""
    alb, nid, dep = gbuffer
    H, W = dep.shape
    fr = Frame(W, H)
    fr.accum = np.array(accum, F)
    fr.albedo = np.ascontiguousarray(alb).view(np.uint32).reshape(H, W).copy()
    fr.normal_id = np.array(nid, F)
    fr.depth = np.array(dep, F)
    fr.uniforms = np.array(uniforms_block, np.uint8)
    return fr


def rmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)))
