"""Rates of the irradiance volume (rt_bake_volume, rt_sample_volume_device) beside the routes that existed before it, from one
process.

(a) bake, per scene (cornell, sponza_like): a 16 x 16 x 16 grid in the scene's bounds (the TLAS root), the outer probes half a
    cell inside them, spp = 1024, depth 4, Hanning window of width 3 - 2^22 samples, one batch:
      volume     one rt_bake_volume call: the wall time of the call (64 B up, 112 B per probe down) and the summed kernel_ms
                 of its radiance launches (rt_probe_gather_stats).  probes + rays + project + finish: the same bake through
                 rt_bake_volume_device between two device events on the context's stream, minus that call's kernel_ms.
      composed   the existing route: the probes made in numpy, one rt_gather_probes call (wall, kernel_ms), the band factors
                 and the window applied in numpy (wall).
(b) sample: the cornell volume of (a) on the device, 2^22 points through rt_sample_volume_device between two device events:
      coherent   a 2048 x 2048 sheet through the middle of the volume, row-major: neighbours share their eight probes
      random     uniformly random in the scene's bounds
    points/s, and bytes/s at the 48 B per point that a point must move (32 B in, 16 B out) - the 896 B per point gathered from
    the 448 KiB volume are cache hits, reported apart as the gather rate.  Beside it, in the same run: a plain device-to-device
    copy that moves the same 48 B per point (24 B per point read and 24 written), as the achieved HBM rate; and the numpy
    float32 restatement of the sampler on the same points (wall time, once per point set, not alternated: it takes seconds).
Device events for the kernel times; one warm-up pass; 5 rounds that alternate the routes; every figure is the median of the
rounds with (min .. max) beside it.  Nothing is gated on these numbers.  What to hold the first run against:
the bake's radiance kernel_ms within the spread of the composed route's (the same rays); the coherent sampler bound by its 48 B
per point, that is, near the copy's rate.

usage: python tools/volume_time.py [--out profiles/volume_rate.txt] [--scenes cornell,sponza_like]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from webgpu_raytracer_amd import renderer as R  # noqa: E402
from timing_util import fmt  # noqa: E402

GRID, DEPTH, SPP, ROUNDS, SEED = 16, 4, 1024, 5, 5
N_POINTS, SHEET = 1 << 22, 2048
BAND_A = np.array([3.141592654] + [2.094395102] * 3 + [0.785398163] * 5, np.float32)
BAND_OF = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])


def bounds(bridge):
    root = np.asarray(bridge.tlas, np.float32).reshape(-1, 8)[0]
    return root[0:3].astype(np.float64), root[4:7].astype(np.float64)


def grid_desc(bridge):
    lo, hi = bounds(bridge)
    step = (hi - lo) / GRID
    return R.volume_desc(lo + 0.5 * step, step, (GRID, GRID, GRID), window=R.sh_hanning_window(3))


def host_probes(d):
    """the grid's probes in numpy float32, as the volume rule makes them"""
    z, y, x = np.meshgrid(np.arange(GRID), np.arange(GRID), np.arange(GRID), indexing="ij")
    idx = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32)
    p = np.zeros((idx.shape[0], 8), np.float32)
    p[:, 0:3] = np.asarray(d["origin"], np.float32) + idx * np.asarray(d["step"], np.float32)
    p[:, 3] = d["t_max"]
    p.view(np.uint32)[:, 7] = int(d["pad_first"]) + np.arange(idx.shape[0], dtype=np.uint32)
    return p


def host_finish(d, sh9):
    out = sh9.copy()
    out["sh"] = (sh9["sh"] * BAND_A[None, :, None]) * np.asarray(d["window"], np.float32)[BAND_OF][None, :, None]
    return out


def host_sample(d, volume, points, chunk=1 << 18):
    """the sampler restated in numpy float32 for a volume whose probes are all valid (plain summation order): (n, 4) f32"""
    dims = np.array([GRID, GRID, GRID])
    sh = np.ascontiguousarray(volume["sh"]).reshape(GRID, GRID, GRID, 27)
    origin, step = np.asarray(d["origin"], np.float32), np.asarray(d["step"], np.float32)
    out = np.empty((points.shape[0], 4), np.float32)
    for first in range(0, points.shape[0], chunk):
        p = points[first:first + chunk]
        g = np.clip((p[:, 0:3] - origin) / step, np.float32(0), (dims - 1).astype(np.float32))
        i0 = np.minimum(g.astype(np.int64), dims - 2)
        f = g - i0.astype(np.float32)
        S = np.zeros((p.shape[0], 27), np.float32)
        Wt = np.zeros(p.shape[0], np.float32)
        for c in range(8):
            dd = np.array([c & 1, (c >> 1) & 1, c >> 2])
            at = i0 + dd
            w = np.prod(np.where(dd, f, np.float32(1) - f), axis=1, dtype=np.float32)
            S += w[:, None] * sh[at[:, 2], at[:, 1], at[:, 0]]
            Wt += w
        nrm = p[:, 4:7] / np.sqrt((p[:, 4:7] * p[:, 4:7]).sum(axis=1, dtype=np.float32))[:, None]
        Y = R.sh9_basis(nrm).astype(np.float32)
        E = np.einsum("mk,mkc->mc", Y, (S / Wt[:, None]).reshape(-1, 9, 3))
        out[first:first + chunk, :3] = np.maximum(E, np.float32(0))
        out[first:first + chunk, 3] = Wt
    return out


def sample_points(bridge, coherent):
    lo, hi = bounds(bridge)
    p = np.zeros((N_POINTS, 8), np.float32)
    if coherent:
        u = (np.arange(SHEET) + 0.5) / SHEET
        yy, xx = np.meshgrid(u, u, indexing="ij")
        p[:, 0] = (lo[0] + xx * (hi[0] - lo[0])).reshape(-1)
        p[:, 1] = (lo[1] + yy * (hi[1] - lo[1])).reshape(-1)
        p[:, 2] = 0.5 * (lo[2] + hi[2])
    else:
        p[:, 0:3] = np.random.default_rng(1).uniform(lo, hi, (N_POINTS, 3))
    p[:, 4:7] = np.random.default_rng(2).normal(size=(N_POINTS, 3))
    return p


def bake_part(scene, lines, keep):
    import torch
    b = W.WorldBridge()
    b.loadScene(scene)
    r = W.WebGPURenderer(0)
    W.upload_scene(r, b, 16, 16)
    r.setKernelTiming(True)
    d = grid_desc(b)
    n = GRID ** 3
    stream = torch.cuda.Stream()
    d_out = torch.empty((n, 28), dtype=torch.float32, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def volume_route():
        t0 = time.perf_counter()
        vol = r.bakeVolume(d, DEPTH, SPP, SEED)
        wall = (time.perf_counter() - t0) * 1e3
        st = r.probeGatherStats()
        r.setStream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            ev[0].record(stream)
            r.bakeVolumeDevice(d, d_out.data_ptr(), DEPTH, SPP, SEED)
            ev[1].record(stream)
        stream.synchronize()
        around = ev[0].elapsed_time(ev[1]) - r.probeGatherStats()["kernel_ms"]
        r.setStream(None)
        return vol, st, wall, around

    def composed_route():
        t0 = time.perf_counter()
        probes = host_probes(d)
        make = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        sh9 = r.gatherProbes(probes, DEPTH, SPP, SEED)
        wall = (time.perf_counter() - t0) * 1e3
        st = r.probeGatherStats()
        t0 = time.perf_counter()
        vol = host_finish(d, sh9)
        return vol, st, wall, make + (time.perf_counter() - t0) * 1e3

    vol, st, _, _ = volume_route()
    vol_c, st_c, _, _ = composed_route()
    same = bool(np.array_equal(vol.reshape(-1).view(np.uint32), vol_c.reshape(-1).view(np.uint32)))
    ms = {"volume radiance kernel": [], "composed radiance kernel": [], "volume kernels around": [], "volume wall": [],
          "composed gather wall": [], "composed numpy wall": []}
    for _ in range(ROUNDS):
        _, st, wall, around = volume_route()
        ms["volume radiance kernel"].append(st["kernel_ms"])
        ms["volume kernels around"].append(around)
        ms["volume wall"].append(wall)
        _, st_c, wall, host = composed_route()
        ms["composed radiance kernel"].append(st_c["kernel_ms"])
        ms["composed gather wall"].append(wall)
        ms["composed numpy wall"].append(host)
    lines.append("%s: %s form, %d workgroups; mean hit fraction %.3f; the two routes give the same words: %s"
                 % (scene, "LDS" if st["lds"] else "global-memory", st["workgroups"], float(vol["hit_fraction"].mean()), same))
    for name in ("volume radiance kernel", "composed radiance kernel"):
        lines.append("  %-25s %s; %s" % (name, fmt([n * SPP / (v * 1e-3) * 1e-6 for v in ms[name]], "Msamples/s"), fmt(ms[name], "ms")))
    for name in ("volume kernels around", "volume wall", "composed gather wall", "composed numpy wall"):
        lines.append("  %-25s %s" % (name, fmt(ms[name], "ms")))
    if keep:
        return r, b, d, vol
    r.destroy()
    return None


def sample_part(r, b, d, vol, lines):
    import torch
    stream = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    d_vol = torch.from_numpy(np.ascontiguousarray(vol).reshape(-1).view(np.float32).copy()).cuda()
    d_res = torch.empty((N_POINTS, 4), dtype=torch.float32, device="cuda")
    copy_src = torch.empty(N_POINTS * 6, dtype=torch.float32, device="cuda")      # 24 B per point read, 24 B written
    copy_dst = torch.empty_like(copy_src)
    sets = {}
    for name, coherent in (("coherent", True), ("random", False)):
        pts = sample_points(b, coherent)
        sets[name] = (pts, torch.from_numpy(pts).cuda())
    torch.cuda.synchronize()
    r.setStream(stream.cuda_stream)

    def timed(fn):
        with torch.cuda.stream(stream):
            ev[0].record(stream)
            fn()
            ev[1].record(stream)
        stream.synchronize()
        return ev[0].elapsed_time(ev[1])

    def sampler(name):
        return timed(lambda: r.sampleVolumeDevice(d, d_vol.data_ptr(), sets[name][1].data_ptr(), N_POINTS, d_res.data_ptr()))

    def copy():
        return timed(lambda: copy_dst.copy_(copy_src))

    for name in sets:
        sampler(name)
    copy()
    ms = {"coherent": [], "random": [], "copy": []}
    for _ in range(ROUNDS):
        for name in ("coherent", "random"):
            ms[name].append(sampler(name))
        ms["copy"].append(copy())
    r.setStream(None)
    lines.append("sampler: %d points from the %d^3 cornell volume (%d KiB); GB/s = 1e-9 * 48 B * points / seconds; the gather rate "
                 "counts the 896 B per point read from the volume instead" % (N_POINTS, GRID, GRID ** 3 * 112 // 1024))
    for name in ("coherent", "random"):
        lines.append("  %-25s %s; %s; %s; gather %s" % (
            name, fmt(ms[name], "ms"), fmt([N_POINTS / (v * 1e-3) * 1e-9 for v in ms[name]], "Gpoints/s"),
            fmt([48.0 * N_POINTS / (v * 1e-3) * 1e-9 for v in ms[name]], "GB/s"),
            fmt([896.0 * N_POINTS / (v * 1e-3) * 1e-9 for v in ms[name]], "GB/s")))
    lines.append("  %-25s %s; %s" % ("device-to-device copy", fmt(ms["copy"], "ms"),
                                       fmt([48.0 * N_POINTS / (v * 1e-3) * 1e-9 for v in ms["copy"]], "GB/s")))
    for name in ("coherent", "random"):
        pts = sets[name][0]
        r.sampleVolumeDevice(d, d_vol.data_ptr(), sets[name][1].data_ptr(), N_POINTS, d_res.data_ptr())
        r.sync()
        got = d_res.cpu().numpy()
        t0 = time.perf_counter()
        want = host_sample(d, vol, pts)
        wall = time.perf_counter() - t0
        diff = float(np.abs(got[:, :3] - want[:, :3]).max())
        lines.append("  numpy sampler, %-10s %.1f ms wall (once); largest |device - numpy| %.3g; mean E %.4f; all W > 0.999: %s"
                     % (name, wall * 1e3, diff, float(got[:, :3].mean()), bool((got[:, 3] > 0.999).all())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", default="cornell,sponza_like")
    args = ap.parse_args()
    lines = ["irradiance volume, %d^3 probes, spp %d, depth %d, Hanning window of width 3; Msamples/s = 1e-6 * probes * spp / "
             "radiance kernel seconds" % (GRID, SPP, DEPTH)]
    kept = None
    for scene in args.scenes.split(","):
        res = bake_part(scene, lines, keep=(scene == "cornell"))
        if res:
            kept = res
    if kept:
        sample_part(*kept, lines)
        kept[0].destroy()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
