"""Rates of reflection probes (rt_bake_reflection, rt_filter_reflection_device) beside the route that existed before them, from
one process, on the Cornell box.

(a) bake: N_PROBES probes on a line through the box, size 64, 5 levels, spt 16, 256 lobe samples, depth 4:
      bake       one rt_bake_reflection call: the wall time of the call (32 B per probe up, a chain per probe down) and the summed
                 kernel_ms of its radiance launches (rt_reflection_stats).  rays + texels + filter: the same bake through
                 rt_bake_reflection_device between two device events on the context's stream, minus that call's kernel_ms.
      composed   the route it replaces: the size^2 * spt rays per probe made in numpy by the rule (wall), one rt_trace_radiance
                 call on them at spp = 1 through the pad identity (wall, kernel_ms; 16 B per sample come back), the mean per
                 texel and the filter restated in numpy float32 (wall).  The two routes give the same words, which is reported.
(b) filter alone: N_FILTER chains of size 128, 6 levels, in place on the device through rt_filter_reflection_device between two
    device events, at 256, 1024 and 4096 lobe samples (the three builds of k_reflection_filter): output texels/s, lookups/s
    (contributing samples only) and the gather rate at 16 B per lookup, to hold against tools/gather_peak.hip's figure in
    profiles/r03_gather_peak.txt.
Device events for the kernel times; one warm-up pass; 5 rounds that alternate the routes; every figure is the median of the
rounds with (min .. max) beside it.  Nothing is gated on these numbers.  What to hold the first run against: DESIGN.md 4.1o.

usage: python tools/reflection_time.py [--out profiles/reflection_rate.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from webgpu_raytracer_amd import renderer as R  # noqa: E402
from timing_util import fmt, init_rng, rand_pcg  # noqa: E402

N_PROBES, SIZE, LEVELS, SPT, K, DEPTH, ROUNDS, SEED = 4, 64, 5, 16, 256, 4, 5, 5
N_FILTER, F_SIZE, F_LEVELS, F_KS = 8, 128, 6, (256, 1024, 4096)
F = np.float32
U = np.uint32


# ---- the rule in numpy: uint32 / float32 arithmetic in the order of mi355rt.h
def sincos(x):
    kf = np.floor(x * F(0.636619746685028076171875) + F(0.5))
    k = kf.astype(np.int32)
    r = x - kf * F(1.5703125)
    r = r - kf * F(4.837512969970703125e-4)
    r = r - kf * F(7.54978995489188216e-8)
    z = r * r
    sp = F(-1.9515295891e-4) * z + F(8.3321608736e-3)
    sp = sp * z - F(1.6666654611e-1)
    s = sp * z * r + r
    cp = F(2.443315711809948e-5) * z - F(1.388731625493765e-3)
    cp = cp * z + F(4.166664568298827e-2)
    c = cp * z * z - F(0.5) * z + F(1.0)
    q = k & 3
    ss, cc = np.where(q & 1, c, s), np.where(q & 1, s, c)
    cc = np.where((q == 1) | (q == 2), -cc, cc)
    ss = np.where(q >= 2, -ss, ss)
    return ss.astype(F), cc.astype(F)


def unpack(px, py):
    nz = F(1.0) - np.abs(px) - np.abs(py)
    t = np.minimum(np.maximum(-nz, F(0.0)), F(1.0))
    nx = px + np.where(px >= 0, -t, t)
    ny = py + np.where(py >= 0, -t, t)
    inv = F(1.0) / np.sqrt(nx * nx + ny * ny + nz * nz)
    return nx * inv, ny * inv, nz * inv


def pack(x, y, z):
    s = F(1.0) / (np.abs(x) + np.abs(y) + np.abs(z))
    px, py = x * s, y * s
    ox = (F(1.0) - np.abs(py)) * np.where(px >= 0, F(1.0), F(-1.0))
    oy = (F(1.0) - np.abs(px)) * np.where(py >= 0, F(1.0), F(-1.0))
    return np.where(z < 0, ox, px), np.where(z < 0, oy, py)


def host_rays(probes, size, spt, seed):
    """the pad' rays of every (probe, texel, sample), probe-major, texel, then sample: (n * size^2 * spt, 8) f32"""
    n = probes.shape[0]
    t = np.arange(size * size, dtype=U)
    s = np.arange(spt, dtype=U)
    pad_t = (probes.view(U)[:, 7][:, None] + t[None, :])[:, :, None].repeat(spt, axis=2)            # (n, T, spt)
    with np.errstate(over="ignore"):
        f = np.broadcast_to((U(seed) * U(spt) + s)[None, None, :], pad_t.shape).astype(U)
    rng = init_rng(pad_t ^ U(0x80000000), f)
    jx = rand_pcg(rng)
    jy = rand_pcg(rng)
    i = (t % U(size)).astype(F)[None, :, None]
    j = (t // U(size)).astype(F)[None, :, None]
    px = (i + jx) / F(size) * F(2.0) - F(1.0)
    py = (j + jy) / F(size) * F(2.0) - F(1.0)
    dx, dy, dz = unpack(px, py)
    rays = np.empty((n, size * size, spt, 8), F)
    rays[..., 0:4] = probes[:, None, None, 0:4]
    rays[..., 4], rays[..., 5], rays[..., 6] = dx, dy, dz
    with np.errstate(over="ignore"):
        rays.view(U)[..., 7] = pad_t + f * U(719393)
    return rays.reshape(-1, 8)


def host_mean(rad, probes, size, spt):
    """(n * size^2 * spt, 4) f32 {r, g, b, t} -> maps (n, size, size, 4) f32"""
    n = probes.shape[0]
    rad = rad.reshape(n, size * size, spt, 4)
    col = np.zeros((n, size * size, 3), F)
    for s in range(spt):
        col = col + rad[:, :, s, :3]
    if spt != 1:
        col = col / F(spt)
    hits = (rad[..., 3] < probes[:, 3][:, None, None]).sum(axis=2).astype(F) / F(spt)
    return np.concatenate([col, hits[..., None]], axis=2).reshape(n, size, size, 4).astype(F)


def lobe(level, levels, K):
    a = F(level) / F(levels - 1)
    s = np.arange(K, dtype=U)
    rev = np.zeros(K, U)
    for b in range(32):
        rev |= ((s >> U(b)) & U(1)) << U(31 - b)
    ux = (s.astype(F) + F(0.5)) / F(K)
    uy = (rev >> U(8)).astype(F) * F(2.0 ** -24)
    cos_t = np.sqrt(np.maximum(F(0.0), (F(1.0) - uy) / (F(1.0) + (a * a - F(1.0)) * uy)))
    sin_t = np.sqrt(np.maximum(F(0.0), F(1.0) - cos_t * cos_t))
    sp, cp = sincos(F(6.28318548202514648438) * ux)
    hx, hy, hz = sin_t * cp, sin_t * sp, cos_t
    return F(2.0) * (hz * hx), F(2.0) * (hz * hy), F(2.0) * (hz * hz) - F(1.0)


def host_filter(maps, levels, K):
    n, size = maps.shape[0], maps.shape[1]
    off = R.reflection_level_offsets(size, levels)
    out = np.empty((n, int(off[-1]), 4), F)
    out[:, :size * size] = maps.reshape(n, size * size, 4)
    lanes = np.arange(64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for lv in range(1, levels):
            S = size >> lv
            tx, ty, tz = lobe(lv, levels, K)
            c = (np.arange(S, dtype=F) + F(0.5)) / F(S) * F(2.0) - F(1.0)
            cx, cy = np.meshgrid(c, c, indexing="xy")
            nx, ny, nz = (a.reshape(-1) for a in unpack(cx, cy))
            sign = np.where(nz >= 0, F(1.0), F(-1.0))
            a = -(F(1.0) / (sign + nz))
            b = nx * ny * a
            u = (F(1.0) + sign * nx * nx * a, sign * b, -sign * nx)
            v = (b, sign + ny * ny * a, -ny)
            w = (nx, ny, nz)
            P = np.zeros((n, S * S, 64, 5), F)
            for s in range(K):
                if not tz[s] > 0:
                    continue
                l = [(tx[s] * u[k] + ty[s] * v[k]) + tz[s] * w[k] for k in range(3)]
                idx = []
                for q in pack(*l):
                    uu = (q * F(0.5) + F(0.5)) * F(size)
                    uu = np.where(uu > 0, uu, F(0.0))
                    idx.append(np.minimum(np.floor(uu).astype(np.int64), size - 1))
                texel = maps[:, idx[1], idx[0], :]
                term = np.concatenate([tz[s] * texel, np.full((n, S * S, 1), tz[s], F)], axis=2)
                P[:, :, s % 64, :] = P[:, :, s % 64, :] + term
            for m in (32, 16, 8, 4, 2, 1):
                P = P + P[:, :, lanes ^ m, :]
            tot = P[:, :, 0, :]
            out[:, off[lv]:off[lv + 1]] = np.where(tot[:, :, 4:5] > 0, tot[:, :, :4] / tot[:, :, 4:5], F(0.0))
    return out


def contributing(levels, K):
    """per level >= 1: lobe samples with w > 0"""
    return [int((lobe(lv, levels, K)[2] > 0).sum()) for lv in range(1, levels)]


def bake_part(lines):
    import torch
    b = W.WorldBridge()
    b.loadScene("cornell")
    r = W.WebGPURenderer(0)
    W.upload_scene(r, b, 16, 16)
    r.setKernelTiming(True)
    root = np.asarray(b.tlas, np.float32).reshape(-1, 8)[0]
    lo, hi = root[0:3].astype(np.float64), root[4:7].astype(np.float64)
    probes = np.zeros((N_PROBES, 8), F)
    for k in range(N_PROBES):
        probes[k, 0:3] = lo + (hi - lo) * (0.25 + 0.5 * (k + 0.5) / N_PROBES)
    probes[:, 3] = 1e30
    probes.view(U)[:, 7] = 1000003 * np.arange(N_PROBES, dtype=U) + 17
    d = R.reflection_desc(SIZE, LEVELS, SPT, K)
    chain = int(R.reflection_level_offsets(SIZE, LEVELS)[-1])
    stream = torch.cuda.Stream()
    d_probes = torch.from_numpy(probes).cuda()
    d_out = torch.empty((N_PROBES, chain, 4), dtype=torch.float32, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def bake_route():
        t0 = time.perf_counter()
        chains = r.bakeReflection(d, probes, DEPTH, SEED)
        wall = (time.perf_counter() - t0) * 1e3
        st = r.reflectionStats()
        r.setStream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            ev[0].record(stream)
            r.bakeReflectionDevice(d, d_probes.data_ptr(), N_PROBES, d_out.data_ptr(), DEPTH, SEED)
            ev[1].record(stream)
        stream.synchronize()
        around = ev[0].elapsed_time(ev[1]) - r.reflectionStats()["kernel_ms"]
        r.setStream(None)
        return chains, st, wall, around

    def composed_route():
        t0 = time.perf_counter()
        rays = host_rays(probes, SIZE, SPT, SEED)
        make = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        rad = r.traceRadiance(rays, DEPTH, 1, 0)
        wall = (time.perf_counter() - t0) * 1e3
        st = r.radianceQueryStats()
        t0 = time.perf_counter()
        maps = host_mean(np.ascontiguousarray(rad).view(F).reshape(-1, 4), probes, SIZE, SPT)
        chains = host_filter(maps, LEVELS, K)
        return chains, st, wall, make, (time.perf_counter() - t0) * 1e3

    chains, st, _, _ = bake_route()
    chains_c, st_c, _, _, _ = composed_route()
    same = bool(np.array_equal(chains.view(U), chains_c.view(U)))
    same0 = bool(np.array_equal(chains[:, :SIZE * SIZE].view(U), chains_c[:, :SIZE * SIZE].view(U)))
    names = ("bake radiance kernel", "composed radiance kernel", "bake kernels around", "bake wall", "composed rays numpy wall",
             "composed query wall", "composed mean + filter wall")
    ms = {k: [] for k in names}
    for _ in range(ROUNDS):
        _, st, wall, around = bake_route()
        ms["bake radiance kernel"].append(st["kernel_ms"])
        ms["bake kernels around"].append(around)
        ms["bake wall"].append(wall)
        _, st_c, wall, make, host = composed_route()
        ms["composed radiance kernel"].append(st_c["kernel_ms"])
        ms["composed rays numpy wall"].append(make)
        ms["composed query wall"].append(wall)
        ms["composed mean + filter wall"].append(host)
    samples = N_PROBES * SIZE * SIZE * SPT
    lines.append("cornell: %s form; mean hit fraction %.3f; the two routes give the same words: %s (level 0: %s)"
                 % ("LDS" if st["lds"] else "global-memory", float(chains[:, :SIZE * SIZE, 3].mean()), same, same0))
    for name in names[:2]:
        lines.append("  %-28s %s; %s" % (name, fmt([samples / (v * 1e-3) * 1e-6 for v in ms[name]], "Msamples/s"), fmt(ms[name], "ms")))
    for name in names[2:]:
        lines.append("  %-28s %s" % (name, fmt(ms[name], "ms")))
    r.destroy()


def filter_part(lines):
    import torch
    r = W.WebGPURenderer(0)                                           # nothing uploaded: the filter needs no scene
    stream = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    off = R.reflection_level_offsets(F_SIZE, F_LEVELS)
    chain = int(off[-1])
    rng = np.random.default_rng(3)
    host = rng.uniform(0.0, 4.0, size=(N_FILTER, chain, 4)).astype(F)
    d_chain = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    r.setStream(stream.cuda_stream)

    def timed(d):
        with torch.cuda.stream(stream):
            ev[0].record(stream)
            r.filterReflectionDevice(d, d_chain.data_ptr(), N_FILTER, d_chain.data_ptr())
            ev[1].record(stream)
        stream.synchronize()
        return ev[0].elapsed_time(ev[1])

    descs = {k: R.reflection_desc(F_SIZE, F_LEVELS, 1, k) for k in F_KS}
    for k in F_KS:
        timed(descs[k])
    ms = {k: [] for k in F_KS}
    for _ in range(ROUNDS):
        for k in F_KS:
            ms[k].append(timed(descs[k]))
    r.setStream(None)
    lines.append("filter alone: %d chains of size %d, %d levels, in place (%d output texels per chain, level 0 is %d KiB); "
                 "GB/s = 1e-9 * 16 B * lookups / seconds" % (N_FILTER, F_SIZE, F_LEVELS, chain - F_SIZE * F_SIZE, F_SIZE * F_SIZE * 16 // 1024))
    for k in F_KS:
        sides = [F_SIZE >> lv for lv in range(1, F_LEVELS)]
        texels = N_FILTER * sum(s * s for s in sides)
        lookups = N_FILTER * sum(s * s * c for s, c in zip(sides, contributing(F_LEVELS, k)))
        lines.append("  K = %-4d (%2d per lane)      %s; %s; %s; gather %s" % (
            k, k // 64, fmt(ms[k], "ms"), fmt([texels / (v * 1e-3) * 1e-6 for v in ms[k]], "Mtexels/s"),
            fmt([lookups / (v * 1e-3) * 1e-9 for v in ms[k]], "Glookups/s"),
            fmt([16.0 * lookups / (v * 1e-3) * 1e-9 for v in ms[k]], "GB/s")))
    r.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["reflection probes, %d probes, size %d, %d levels, spt %d, %d lobe samples, depth %d; Msamples/s = 1e-6 * probes * "
             "size^2 * spt / radiance kernel seconds" % (N_PROBES, SIZE, LEVELS, SPT, K, DEPTH)]
    bake_part(lines)
    filter_part(lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
