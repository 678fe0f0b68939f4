"""Shared pieces of the probe-gather tests (rt_gather_probes): the reference model (tests/model/probe_model.cpp: the radiance
model's translation unit plus the probe gather stated once on its first-hit and bounce functions), built with the flags of
oracle/Makefile and driven through a ModelRenderer that loads the probe library instead; the numpy restatement of the
projection (basis, fixed summation tree) that the composition tests put behind radiance queries; and the probe set of the GPU
tests."""
import ctypes
import functools
import os

import numpy as np

import model_build
import radiance_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "model", "probe_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libprobe_model.so")
COUNT_NAMES = ru.COUNT_NAMES
SEED = ru.SEED
RNG_STEP = 719393                 # init_rng(a, b) hashes a + b * RNG_STEP
FOUR_PI = np.float32(12.566370614)
Y0 = np.float32(0.282094792)


@functools.lru_cache(maxsize=None)
def model_lib():
    """the probe library: every oracle_* and radiance_model_* entry declared as radiance_util declares it, plus the two
    probe_model_* ones"""
    L = ru.bind_model(model_build.build(SRC, LIB, ru.FLAGS + ["-shared"]))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.probe_model_directions.argtypes = [vp, u32, u32, u32, vp]
    L.probe_model_directions.restype = None
    L.probe_model_gather.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, vp]
    L.probe_model_gather.restype = None
    return L


class ProbeModel(ru.ModelRenderer):
    """ModelRenderer on the probe library: the oracle, traceRadiance / cameraRays, plus probeDirections / gatherProbes"""
    _library = staticmethod(model_lib)

    def probeDirections(self, probes, spp, seed):
        """probes (n, 8) f32 in the rt_probe layout -> (n, spp, 3) f32: the direction of every sample"""
        p = np.ascontiguousarray(probes, dtype=np.float32)
        out = np.empty((p.shape[0], spp, 3), np.float32)
        self.L.probe_model_directions(p.ctypes.data, p.shape[0], spp, seed & 0xffffffff, out.ctypes.data)
        return out

    def gatherProbes(self, probes, max_depth, spp, seed):
        """-> (out (n, 28) f32 {sh[9][3], hit_fraction}, hits (n,) u32, counts (n, 5) u64 COUNT_NAMES)"""
        p = np.ascontiguousarray(probes, dtype=np.float32)
        n = p.shape[0]
        out = np.empty((n, 28), np.float32)
        hits = np.empty(n, np.uint32)
        counts = np.empty((n, 5), np.uint64)
        self.L.probe_model_gather(self.ctx, p.ctypes.data, n, max_depth, spp, seed & 0xffffffff, out.ctypes.data,
                                  hits.ctypes.data, counts.ctypes.data)
        return out, hits, counts


model_for = functools.partial(ru.model_for, cls=ProbeModel)


def make_probes(positions, t_max=1e30, pad_step=ru.PAD_STEP, pad_first=ru.PAD_0):
    """(n, 3) positions -> (n, 8) f32 in the rt_probe layout: unused words 0, pads pad_step * i + pad_first"""
    pos = np.asarray(positions, np.float32)
    p = np.zeros((pos.shape[0], 8), np.float32)
    p[:, 0:3] = pos
    p[:, 3] = np.float32(t_max)
    return ru.with_pads(p, pad_step, pad_first)


def sample_frames(spp, seed):
    """f = seed * spp + s in u32 arithmetic, s = 0 .. spp-1"""
    return ((np.uint64(seed & 0xffffffff) * np.uint64(spp) + np.arange(spp, dtype=np.uint64)) & np.uint64(0xffffffff)).astype(np.uint32)


def plain_rays(probes, dirs, s):
    """the rays {position, t_max, direction of sample s, pad} of every probe, in the rt_ray layout"""
    r = np.ascontiguousarray(probes, np.float32).copy()
    r[:, 4:7] = dirs[:, s, :]
    return r


def pad_prime_rays(probes, dirs, spp, seed):
    """the n * spp rays k_probe_rays makes, probe-major: {position, t_max, direction, pad' = pad + f * 719393 (u32)}"""
    p = np.ascontiguousarray(probes, np.float32)
    n = p.shape[0]
    r = np.repeat(p, spp, axis=0)
    r[:, 4:7] = dirs.reshape(n * spp, 3)
    f = np.tile(sample_frames(spp, seed), n).astype(np.uint64)
    pads = np.repeat(p.view(np.uint32)[:, 7].astype(np.uint64), spp)
    r.view(np.uint32)[:, 7] = ((pads + f * np.uint64(RNG_STEP)) & np.uint64(0xffffffff)).astype(np.uint32)
    return r


def sh9_basis_f32(d):
    """(..., 3) f32 -> (..., 9) f32: the basis of the probe rule, every operation a float32 one in the order written"""
    d = np.asarray(d, np.float32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    c = np.float32
    Y = np.empty(d.shape[:-1] + (9,), np.float32)
    Y[..., 0] = c(0.282094792)
    Y[..., 1] = c(0.488602512) * y
    Y[..., 2] = c(0.488602512) * z
    Y[..., 3] = c(0.488602512) * x
    Y[..., 4] = c(1.092548431) * (x * y)
    Y[..., 5] = c(1.092548431) * (y * z)
    Y[..., 6] = c(0.315391565) * (c(3.0) * (z * z) - c(1.0))
    Y[..., 7] = c(1.092548431) * (x * z)
    Y[..., 8] = c(0.546274215) * (x * x - y * y)
    return Y


def project(radiance, dirs, t_max):
    """The projection of the probe rule in numpy float32: radiance (n, spp, 4) f32 {r, g, b, t}, dirs (n, spp, 3) f32, t_max
    (n,) f32 -> (out (n, 28) f32, hits (n,) u32).  Lane partials in ascending sample order from +0, the six butterfly steps,
    lane 0, rt_div by spp, times 4 pi."""
    rad = np.ascontiguousarray(radiance, np.float32)
    n, spp = rad.shape[:2]
    with np.errstate(invalid="ignore", over="ignore"):
        terms = (rad[:, :, None, :3] * sh9_basis_f32(dirs)[:, :, :, None]).reshape(n, spp, 27)
        assert terms.dtype == np.float32
        P = np.zeros((n, 64, 27), np.float32)
        for s in range(spp):
            P[:, s % 64, :] = P[:, s % 64, :] + terms[:, s, :]
        lanes = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            P = P + P[:, lanes ^ m, :]
        assert P.dtype == np.float32
        hits = (rad[:, :, 3] < np.asarray(t_max, np.float32)[:, None]).sum(axis=1).astype(np.uint32)
        out = np.empty((n, 28), np.float32)
        out[:, :27] = (P[:, 0, :] / np.float32(spp)) * FOUR_PI
        out[:, 27] = hits.astype(np.float32) / np.float32(spp)
    return out, hits


def compose(trace, probes, dirs, max_depth, spp, seed):
    """The probe gather as the composition of radiance queries on the PLAIN rays: trace(rays, max_depth, 1, f) -> ((n, 4)
    f32 {r, g, b, t}, extra) for every sample, then project().  Returns (out, hits, [extra of every call])."""
    probes = np.ascontiguousarray(probes, np.float32)
    n = probes.shape[0]
    rad = np.empty((n, spp, 4), np.float32)
    extras = []
    for s, f in enumerate(sample_frames(spp, seed)):
        res, extra = trace(plain_rays(probes, dirs, s), max_depth, 1, int(f))
        rad[:, s, :] = res
        extras.append(extra)
    out, hits = project(rad, dirs, probes[:, 3])
    return out, hits, extras


def compose_pad_prime(trace, probes, dirs, max_depth, spp, seed):
    """The same through ONE radiance query on the pad' rays at seed = 0, spp = 1.  Returns (out, hits, extra)."""
    probes = np.ascontiguousarray(probes, np.float32)
    n = probes.shape[0]
    res, extra = trace(pad_prime_rays(probes, dirs, spp, seed), max_depth, 1, 0)
    out, hits = project(np.ascontiguousarray(res, np.float32).reshape(n, spp, 4), dirs, probes[:, 3])
    return out, hits, extra


def scene_bounds(bridge):
    """(lo, hi) of the world box: the TLAS root"""
    root = np.asarray(bridge.tlas, np.float32).reshape(-1, 8)[0]
    return root[0:3].astype(np.float64), root[4:7].astype(np.float64)


def grid_positions(bridge, k):
    """k^3 cell centres of a grid in the scene's bounds"""
    lo, hi = scene_bounds(bridge)
    g = (np.arange(k) + 0.5) / k
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * (hi - lo) + lo


def scene_probes(model, bridge):
    """96 probes of a scene, pads 7 i + 3: a 4 x 4 x 4 grid in the bounds of the scene, 16 ON its surfaces (the first hits of
    rays from the middle of the scene) and 16 outside every box (beyond the bounds)"""
    lo, hi = scene_bounds(bridge)
    mid = 0.5 * (lo + hi)
    rng = np.random.default_rng(77)
    unit = rng.normal(size=(528, 3))
    unit /= np.linalg.norm(unit, axis=1)[:, None]
    rays = np.zeros((512, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = mid, 1e30, unit[:512]
    t = model.traceRadiance(rays, 0, 1, 0)[0][:, 3]
    hit = np.nonzero(t < rays[:, 3])[0][:16]
    assert hit.size == 16, "the scene is too open for 16 surface probes"
    surf = rays[hit, 0:3] + rays[hit, 4:7] * t[hit, None]
    outside = mid + unit[512:] * (1.5 * np.linalg.norm(hi - lo))
    return make_probes(np.concatenate([grid_positions(bridge, 4), surf, outside]))


result_words = functools.partial(ru.result_words, width=28)   # PROBE_SH9_DTYPE (n,) -> (n, 28) u32
# res: PROBE_SH9_DTYPE (n,); ref: (n, 28) f32; the rule of the gathers
check_against_model = functools.partial(ru.check_records_against_model, width=28, what="probes", shown=2)
check_counts = ru.check_counts
