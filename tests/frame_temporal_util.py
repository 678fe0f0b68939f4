"""Shared pieces of the frame-temporal tests (rt_set_frame_temporal): the reference model of the stage
(tests/model/frame_temporal_model.cpp), built with the flags of oracle/Makefile as the other models are; the history a context
keeps, as a small class; a whole call as frame_denoise_util.prepare -> stage -> one_pass x passes -> finish; a pinhole that can
be moved and rolled, for frame_denoise_util.Frame scenes; and the cornell sequences of the oracle the quality gate uses."""
import ctypes
import functools
import os

import numpy as np

import frame_denoise_util as fu
import model_build
import radiance_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "model", "frame_temporal_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libframe_temporal_model.so")
SAME_INSTANCE = 1
MAX_HISTORY = 256
F = np.float32
U = fu.U
DESC_DTYPE = np.dtype([("flags", "<u4"), ("max_history", "<u4"), ("var_history", "<u4"), ("normal_cos", "<f4"),
                       ("plane_eps", "<f4"), ("reserved", "<u4", (3,))])
# the documented parameters of the cornell quality gate and of the GPU tests on cornell
CORNELL = dict(flags=0, max_history=32, var_history=4, normal_cos=0.9, plane_eps=0.02)


@functools.lru_cache(maxsize=None)
def model_lib():
    L = ctypes.CDLL(model_build.build(SRC, LIB, ru.FLAGS + ["-I", os.path.join(REPO, "include"), "-shared"]))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.ft_model_stage.argtypes = [vp] * 7 + [u32, u32] + [vp] * 4
    L.ft_model_stage.restype = ctypes.c_int
    return L


def desc(**kw):
    d = np.zeros(1, DESC_DTYPE)
    for k, v in kw.items():
        d[k] = v
    return d


class History:
    """what a context keeps between frames: the history colour (H, W, 4) {q.rgb, n}, the moments (H, W, 2), the guide (H, W, 8)
    and the 256-byte uniform block of the frame they were made from; `frames` integrated since the last drop"""

    def __init__(self):
        self.hist = self.mom = self.guide = self.uniforms = None
        self.frames = 0

    def n(self):
        return self.hist[..., 3]


def stage(col, guide, uniforms, d, state):
    """One run of the stage by the model.  state: a History, advanced IN PLACE.  -> integ (H, W, 4), accepted (H, W) u32"""
    d = desc(**d) if isinstance(d, dict) else np.ascontiguousarray(d, DESC_DTYPE)
    col, guide = np.ascontiguousarray(col, F), np.ascontiguousarray(guide, F)
    H, W = col.shape[:2]
    integ, hist, mom = np.empty((H, W, 4), F), np.empty((H, W, 4), F), np.empty((H, W, 2), F)
    acc = np.zeros((H, W), np.uint32)
    have = state.hist is not None
    if have:
        ph, pm, pg = (np.ascontiguousarray(a, F) for a in (state.hist, state.mom, state.guide))
        pu = np.ascontiguousarray(state.uniforms, np.uint8)
    r = model_lib().ft_model_stage(col.ctypes.data, guide.ctypes.data, ph.ctypes.data if have else None,
                                   pm.ctypes.data if have else None, pg.ctypes.data if have else None,
                                   pu.ctypes.data if have else None, d.ctypes.data, W, H, integ.ctypes.data, hist.ctypes.data,
                                   mom.ctypes.data, acc.ctypes.data)
    assert r == 0, "the model refuses this descriptor"
    state.hist, state.mom, state.guide = hist, mom, guide.copy()
    state.uniforms = np.array(uniforms, np.uint8)
    state.frames += 1
    return integ, acc


def filter_from(col, guide, mod, d):
    """the passes and the finish of a call on a colour image"""
    d = fu.desc(**d) if isinstance(d, dict) else d
    for p in range(int(d["passes"][0])):
        col = fu.one_pass(col, guide, int(d["step"][0]) << p, flags=int(d["flags"][0]), normal_cos=float(d["normal_cos"][0]),
                          plane_eps=float(d["plane_eps"][0]), sigma_lum=float(d["sigma_lum"][0]))
    return fu.finish(col, mod)


def call(fr, d, t, state):
    """A whole call with the stage on, composed of its stages: prepare -> stage -> passes -> finish.  fr: a
    frame_denoise_util.Frame; d: the denoise descriptor, t: the temporal one (dicts or records); state: a History, advanced in
    place - dropped first when the DEMODULATE bit differs from the one it was made under.  -> out (H, W, 4), integ, accepted"""
    dd = fu.desc(**d) if isinstance(d, dict) else np.ascontiguousarray(d, fu.DESC_DTYPE)
    demod = int(dd["flags"][0]) & fu.DEMODULATE
    if state.hist is not None and getattr(state, "demod", demod) != demod:
        state.__init__()
    state.demod = demod
    col, guide, mod = fu.prepare(fr, int(dd["flags"][0]))
    integ, acc = stage(col, guide, fr.uniforms, t, state)
    return filter_from(integ, guide, mod, dd), integ, acc


def camera(width, height, eye=(0.0, 0.0, 0.0), roll=0.0, jitter=(0.0, 0.0)):
    """frame_denoise_util.uniforms with the pinhole at `eye`, rolled by `roll` radians about its axis (-z): the image plane is
    one unit ahead and spans 2 x 2, hor and ver orthogonal and NOT axis-aligned when roll != 0"""
    u = fu.uniforms(width, height, jitter).view(np.float32).copy()
    e = np.asarray(eye, np.float64)
    hor = 2.0 * np.array([np.cos(roll), np.sin(roll), 0.0])
    ver = 2.0 * np.array([-np.sin(roll), np.cos(roll), 0.0])
    u[0:3] = e
    u[4:7] = e + np.array([0.0, 0.0, -1.0]) - hor / 2 - ver / 2
    u[8:11] = hor
    u[12:15] = ver
    return u.view(np.uint8)


def wall(width, height, eye=(0.0, 0.0, 0.0), roll=0.0, jitter=(0.0, 0.0), plane_z=-2.0, **kw):
    """a Frame that sees the plane z = plane_z (normal +z) from camera(...): the view depth is eye.z - plane_z everywhere"""
    fr = fu.Frame(width, height, z=float(eye[2]) - plane_z, jitter=jitter, **kw)
    fr.uniforms = camera(width, height, eye, roll, jitter)
    return fr


def moved_camera(bridge, k, step):
    """the bridge's cameraData (24 floats: origin, lower_left, horizontal, vertical, u, v) with the pinhole translated by
    k * step world units"""
    cam = np.array(bridge.cameraData, dtype=np.float32).reshape(6, 4).copy()
    s = (np.asarray(step, np.float64) * k).astype(np.float32)
    cam[0, :3] += s
    cam[1, :3] += s
    return cam.reshape(-1)


def render_frame(r, bridge, k, step, frame_count):
    """one frame of a sequence on any renderer (the oracle binding too): the camera at k * step, a fresh accumulation, one
    compute(frame_count)"""
    r.updateSceneUniforms(moved_camera(bridge, k, step), 0, bridge.lightCount)
    r.resetAccumulation()
    r.compute(frame_count)


_sequences = {}
# the camera step of the quality gate, world units per frame (cornell's box is about 2 units wide; at 64 x 64 a pixel of the
# back wall is about 0.03 units): a third of a pixel per frame, sideways and up
GATE_STEP = (0.01, 0.005, 0.0)


def cornell_sequence(W, oracle_lib, frames=8, step=GATE_STEP, size=64, depth=4, clean_spp=512):
    """cornell by the CPU oracle at size x size: `frames` frames of 1 spp, the accumulation reset every frame and the camera
    translated by `step` per frame through updateSceneUniforms; and the clean image, clean_spp samples at the last camera.
    -> {"frames": [Frame, ...], "clean": (H, W, 3) radiance}.  Rendered once per process."""
    key = (frames, tuple(step), size, depth, clean_spp)
    if key in _sequences:
        return _sequences[key]
    import parity_util as pu
    b = pu.bridge_for(W, "cornell")
    o = oracle_lib.OracleRenderer()
    o.buildPipeline(depth, 1)
    W.upload_scene(o, b, size, size)
    out = {"frames": []}
    for f in range(frames):
        render_frame(o, b, f, step, f + 1)
        out["frames"].append(fu.frame_of(o.readAccum(), o.readGBuffer(), o.readUniforms()))
    c = oracle_lib.OracleRenderer()
    c.buildPipeline(depth, 64)
    W.upload_scene(c, b, size, size)
    c.updateSceneUniforms(moved_camera(b, frames - 1, step), 0, b.lightCount)
    c.resetAccumulation()
    for f in range(clean_spp // 64):
        c.compute(f + 1)
    a = c.readAccum()
    out["clean"] = a[..., :3] / a[..., 3:4]
    _sequences[key] = out
    return out


def footprint(guide, prev_uniforms):
    """Where the surface points of `guide` (H, W, 8) fall in the previous frame, in float64 - a restatement for the tests, not the
    rule's arithmetic: -> fx, fy (H, W) pixel coordinates (pixel centres at whole numbers), s (H, W) the sign test's quantity"""
    u = np.asarray(prev_uniforms, np.uint8).view(np.float32).astype(np.float64)
    eye, ll, hor, ver = u[0:3], u[4:7], u[8:11], u[12:15]
    Wd, Hd = (float(v) for v in np.asarray(prev_uniforms, np.uint8).view(np.uint32)[53:55])
    jx, jy = u[56], u[57]
    P = np.asarray(guide, np.float64)[..., 0:3]
    nrm = np.cross(hor, ver)
    with np.errstate(all="ignore"):
        s = np.dot(ll - eye, nrm) / ((P - eye) @ nrm)
        r = (P - eye) * s[..., None] - (ll - eye)
        uu, vv = (r @ hor) / np.dot(hor, hor), (r @ ver) / np.dot(ver, ver)
    return uu * Wd - 0.5 - jx * Wd, (1.0 - vv) * Hd - 0.5 - jy * Hd, s
