"""Shared pieces of the irradiance-volume tests (rt_bake_volume / rt_sample_volume / rt_encode_volume): the stand-alone reference
model (tests/model/volume_model.cpp, built with the flags the other models use), the numpy float32 restatement of the grid
probes and of the finish that the composition tests put around probe gathers, the float64 restatement of the sampler, and the
volumes and points of the parity tests."""
import ctypes
import functools
import os

import numpy as np

import model_build
import radiance_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "model", "volume_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libvolume_model.so")
BAND_A = np.array([3.141592654] + [2.094395102] * 3 + [0.785398163] * 5, np.float32)
BAND_OF = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])
# the largest |f32 - f64| / max(1, |f64|) of the MODEL's sampler on the inputs of tests/test_volume_model.py, measured on the
# development host (its docstring has the figure), times four: the margin is for other libm / compiler versions
FLOAT_TOLERANCE = 4 * 1.16e-6


def _renderer_module():
    from webgpu_raytracer_amd import renderer
    return renderer


@functools.lru_cache(maxsize=None)
def model_lib():
    L = ctypes.CDLL(model_build.build(SRC, LIB, ru.FLAGS + ["-I", os.path.join(REPO, "include"), "-shared"]))
    vp = ctypes.c_void_p
    L.volume_model_probes.argtypes = [vp, vp]
    L.volume_model_finish.argtypes = [vp, vp]
    L.volume_model_sample.argtypes = [vp, vp, vp, ctypes.c_uint32, vp]
    L.volume_model_layers.argtypes = [vp, vp, ctypes.c_int, vp]
    for f in (L.volume_model_probes, L.volume_model_finish, L.volume_model_sample, L.volume_model_layers):
        f.restype = None
    return L


def probe_count(desc):
    d = np.asarray(desc).reshape(())
    return int(d["nx"]) * int(d["ny"]) * int(d["nz"])


def model_probes(desc):
    """-> (n, 8) f32 in the rt_probe layout: the probes of the grid, by the model"""
    d = np.ascontiguousarray(desc)
    out = np.empty((probe_count(d), 8), np.float32)
    model_lib().volume_model_probes(d.ctypes.data, out.ctypes.data)
    return out


def model_finish(desc, sh9):
    """(n, 28) f32 radiance records -> a NEW (n, 28) f32 of irradiance coefficients, by the model"""
    d = np.ascontiguousarray(desc)
    v = np.array(sh9, np.float32).reshape(probe_count(d), 28)
    model_lib().volume_model_finish(d.ctypes.data, v.ctypes.data)
    return v


def model_sample(desc, volume, points):
    """volume (n, 28) f32, points (m, 8) f32 -> (m, 4) f32 {rgb, W}, by the model"""
    d = np.ascontiguousarray(desc)
    v = np.ascontiguousarray(volume, np.float32).reshape(probe_count(d), 28)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 8)
    out = np.empty((p.shape[0], 4), np.float32)
    model_lib().volume_model_sample(d.ctypes.data, v.ctypes.data, p.ctypes.data, p.shape[0], out.ctypes.data)
    return out


def model_layers(desc, volume, f16):
    """-> (7, n, 4) f32, or uint16 half bit patterns"""
    d = np.ascontiguousarray(desc)
    v = np.ascontiguousarray(volume, np.float32).reshape(probe_count(d), 28)
    out = np.empty((7, probe_count(d), 4), np.uint16 if f16 else np.float32)
    model_lib().volume_model_layers(d.ctypes.data, v.ctypes.data, int(bool(f16)), out.ctypes.data)
    return out


def numpy_probes(desc):
    """the probes of the grid in numpy float32: position = origin + f32(idx) * step with the product rounded first, t_max of
    the desc, unused words 0, pad = pad_first + p; -> (n, 8) f32"""
    desc = np.asarray(desc).reshape(())
    nx, ny, nz = int(desc["nx"]), int(desc["ny"]), int(desc["nz"])
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    idx = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32)
    step, origin = np.asarray(desc["step"], np.float32), np.asarray(desc["origin"], np.float32)
    prod = idx * step
    assert prod.dtype == np.float32
    p = np.zeros((nx * ny * nz, 8), np.float32)
    p[:, 0:3] = origin + prod
    p[:, 3] = desc["t_max"]
    p.view(np.uint32)[:, 7] = int(desc["pad_first"]) + np.arange(nx * ny * nz, dtype=np.uint32)
    return p


def numpy_finish(desc, sh9):
    """the finish in numpy float32: (sh * A_band) * window[band], hit_fraction's bits kept; (n, 28) f32 -> a new (n, 28) f32"""
    v = np.array(sh9, np.float32).reshape(-1, 28)
    window = np.asarray(np.asarray(desc).reshape(())["window"], np.float32)[BAND_OF]
    with np.errstate(invalid="ignore", over="ignore"):
        sh = (v[:, :27].reshape(-1, 9, 3) * BAND_A[None, :, None]) * window[None, :, None]
    assert sh.dtype == np.float32
    v[:, :27] = sh.reshape(-1, 27)
    return v


def sample_f64(desc, volume, points):
    """The sampler in float64 for volumes whose probes are all valid: the trilinear blend of the eight surrounding probes'
    sh9_basis evaluations at the normalised normal, clamped at 0.  -> (m, 3) float64"""
    R = _renderer_module()
    desc = np.asarray(desc).reshape(())
    dims = np.array([int(desc["nx"]), int(desc["ny"]), int(desc["nz"])])
    v = np.asarray(volume, np.float64).reshape(dims[2], dims[1], dims[0], 28)[..., :27].reshape(dims[2], dims[1], dims[0], 9, 3)
    p = np.asarray(points, np.float64).reshape(-1, 8)
    g = (p[:, 0:3] - np.asarray(desc["origin"], np.float64)) / np.asarray(desc["step"], np.float64)
    g = np.clip(g, 0.0, dims - 1.0)
    i0 = np.minimum(np.floor(g).astype(np.int64), np.maximum(dims - 2, 0))
    i1 = np.minimum(i0 + 1, dims - 1)
    f = g - i0
    nrm = p[:, 4:7] / np.linalg.norm(p[:, 4:7], axis=1)[:, None]
    Y = R.sh9_basis(nrm)                                                  # (m, 9)
    E = np.zeros((p.shape[0], 3))
    for c in range(8):
        d = np.array([c & 1, (c >> 1) & 1, c >> 2])
        at = np.where(d, i1, i0)
        w = np.prod(np.where(d, f, 1.0 - f), axis=1)
        E += w[:, None] * np.einsum("mk,mkc->mc", Y, v[at[:, 2], at[:, 1], at[:, 0]])
    return np.maximum(E, 0.0)


def make_points(positions, normals):
    """-> (n, 8) f32 in the rt_gather_point layout; t_max and pad, which the sampler does not read, hold junk on purpose"""
    pos, nrm = np.asarray(positions, np.float32), np.asarray(normals, np.float32)
    p = np.empty((pos.shape[0], 8), np.float32)
    p[:, 0:3], p[:, 4:7] = pos, nrm
    p[:, 3] = np.nan
    p.view(np.uint32)[:, 7] = 0xdeadbeef
    return p


def random_volume(desc, seed, invalid=True):
    """(n, 28) f32: coefficients uniform in [-1, 2) (irradiance-like: mostly positive band 0).  invalid: hit_fraction spread
    over [0, 1] (some exactly 0, 0.5 and 1, one NaN where there is room), and a fifth of the probes with hit_fraction above 0.5
    get a NaN or an infinite coefficient - an invalid probe at max_hit_fraction = 0.5 may hold anything; a few valid probes
    get one too.  Else every hit_fraction is 0."""
    rng = np.random.default_rng(seed)
    n = probe_count(desc)
    v = np.zeros((n, 28), np.float32)
    v[:, :27] = rng.uniform(-1.0, 2.0, (n, 27))
    v[:, 0:3] += 2.0
    if invalid:
        hf = rng.uniform(0.0, 1.0, n).astype(np.float32)
        hf[rng.random(n) < 0.45] *= 0.5                                   # more than half valid at 0.5
        if n == 1:
            hf[0] = 0.25                                                  # a one-probe grid with its probe invalid samples nothing
        for k, val in enumerate((0.0, 0.5, 1.0, np.nan)):
            if n > 2 * k + 2:
                hf[2 * k + 1] = val
        v[:, 27] = hf
        bad = np.nonzero(~(hf <= 0.5))[0]
        for p in bad[::2]:
            v[p, rng.integers(27)] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32))
        good = np.nonzero(hf <= 0.5)[0]
        for p in good[5::17]:
            v[p, rng.integers(27)] = rng.choice(np.array([np.nan, np.inf], np.float32))
    return v


def parity_points(desc, n, seed):
    """n points for the sampler parity: every grid node exactly, cell centres, the last node of each axis, points outside on
    every side, a NaN, a +inf and a -inf position, a zero normal - then random points in and around the grid up to n (a short
    n keeps the head of that list, in an order mixed by the seed so that every kind comes early)."""
    rng = np.random.default_rng(seed)
    desc = np.asarray(desc).reshape(())
    dims = np.array([int(desc["nx"]), int(desc["ny"]), int(desc["nz"])])
    origin, step = np.asarray(desc["origin"], np.float32), np.asarray(desc["step"], np.float32)
    nodes = numpy_probes(desc)[:, 0:3]
    hi = origin + (dims - 1).astype(np.float32) * step
    centres = nodes + np.float32(0.5) * step
    outside = []
    for a in range(3):
        for side in (-1.0, 1.0):
            q = (origin + hi) * np.float32(0.5)
            q[a] = (origin[a] - 3.0 * step[a]) if side < 0 else (hi[a] + 3.0 * step[a])
            outside.append(q)
    last = []
    for a in range(3):
        q = origin + np.float32(0.25) * step
        q[a] = hi[a]
        last.append(q)
    odd = np.tile((origin + hi) * np.float32(0.5), (3, 1))
    odd[0, 0], odd[1, 1], odd[2, 2] = np.nan, np.inf, -np.inf
    special = np.concatenate([np.array(outside, np.float32), np.array(last, np.float32), odd, [hi], [origin]])
    pos = np.concatenate([special, nodes, centres]).astype(np.float32)
    order = rng.permutation(len(pos))
    pos = pos[order]
    if len(pos) < n:
        extra = rng.uniform(origin - step, hi + step, (n - len(pos), 3)).astype(np.float32)
        pos = np.concatenate([pos, extra])
    pos = pos[:n]
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm[::5] *= np.float32(7.5)                                           # need not be normalised
    if n > 2:
        nrm[n // 2] = 0.0                                                 # a zero normal
    return make_points(pos, nrm)


def words(a):
    """any array of 4-byte items or records -> its uint32 words, flat"""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def check_samples(got, want, tag):
    """got: IRRADIANCE_DTYPE (n,) or (n, 4) f32; want: the model's (n, 4) f32.  Bit for bit, point by point; NaNs compare as a
    class only in rows where the model has one."""
    g, w = words(got).reshape(-1, 4), words(want).reshape(-1, 4)
    bad = g != w
    gf, wf = g.view(np.float32), w.view(np.float32)
    model_nan_row = np.isnan(wf).any(axis=1)
    bad &= ~(np.isnan(gf) & np.isnan(wf) & model_nan_row[:, None])
    rows = np.nonzero(bad.any(axis=1))[0]
    assert rows.size == 0, (tag, "points that differ", int(rows.size), rows[:8].tolist(), gf[rows[:3]].tolist(),
                            wf[rows[:3]].tolist())
