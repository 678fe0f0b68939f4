"""Rate of the irradiance gather (rt_gather_irradiance) beside the route it replaces, from one process.

Per scene (cornell, sponza_like): 2^18 points made from the first hits of a 512 x 512 grid of the scene camera's rays (a hit
gives the point o + d (0.999 t) with normal -d / |d|, a miss the point o with normal d / |d|), spp = 16, depth 4:
  gather     one rt_gather_irradiance call on the points: kernel_ms of rt_irradiance_gather_stats, and the wall time of the
             call (points up, results down)
  composed   the same samples as 16 rt_trace_radiance calls (spp = 1, seed = seed * 16 + s) on 2^18 host-made rays each, summed
             and divided on the host: the summed kernel_ms of rt_radiance_query_stats, and the wall time of the 16 calls with
             the sum (rays up, results down).  The directions are the gather's rule restated in numpy (equal up to the rounding
             of sin / cos); making them is timed apart and is not part of the wall time.
Device events for the kernel times; one warm-up pass; 5 rounds that alternate the two routes; every figure is the median of
the rounds with (min .. max) beside it.  Nothing is gated on these numbers.  What to hold the first run against: the
gather's kernel time within the spread of the composed kernels' (the same rays), its wall time lower by the transfers.

usage: python tools/irradiance_gather_time.py [--out profiles/irradiance_gather_rate.txt] [--scenes cornell,sponza_like]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from timing_util import camera_rays, fmt, init_rng, rand_pcg  # noqa: E402

GRID, DEPTH, SPP, ROUNDS, SEED = 512, 4, 16, 5, 5


def points_from_hits(rays, t, hit):
    o, d = rays[:, 0:3], rays[:, 4:7]
    unit = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    p = rays.copy()
    p[:, 0:3] = np.where(hit[:, None], o + d * (np.float32(0.999) * t)[:, None], o)
    p[:, 4:7] = np.where(hit[:, None], -unit, unit)
    return np.ascontiguousarray(p, np.float32)


def directions(points, f):
    """sample f of every point: the Lambert sampler's direction (Raytracer.wgsl:228-233, 191-199, 207-214) in float32"""
    rng = init_rng(points.view(np.uint32)[:, 7] ^ np.uint32(0x80000000), np.uint32(f))
    r1, r2 = rand_pcg(rng), rand_pcg(rng)
    n = points[:, 4:7]
    n = n / np.sqrt((n * n).sum(axis=1, dtype=np.float32))[:, None]
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    sign = np.where(z >= 0, np.float32(1), np.float32(-1))
    a = -np.float32(1) / (sign + z)
    b = x * y * a
    u = np.stack([1 + sign * x * x * a, sign * b, -sign * x], axis=1)
    v = np.stack([b, sign + y * y * a, -y], axis=1)
    phi = np.float32(2 * np.pi) * r1
    cos_t, sin_t = np.sqrt(1 - r2), np.sqrt(r2)
    d = (np.cos(phi) * sin_t)[:, None] * u + (np.sin(phi) * sin_t)[:, None] * v + cos_t[:, None] * n
    return d.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", default="cornell,sponza_like")
    args = ap.parse_args()
    n = GRID * GRID
    lines = ["irradiance gather rate, %d points, spp %d, depth %d; Msamples/s = 1e-6 * points * spp / kernel seconds" % (n, SPP, DEPTH)]
    for scene in args.scenes.split(","):
        b = W.WorldBridge()
        b.loadScene(scene)
        r = W.WebGPURenderer(0)
        W.upload_scene(r, b, GRID, GRID)
        r.setKernelTiming(True)
        rays = camera_rays(b, GRID, GRID, pads=True)
        first = r.traceRays(rays)
        hit = first["hit"] != 0
        points = points_from_hits(rays, first["t"], hit)
        t0 = time.perf_counter()
        sample_rays = []
        for s in range(SPP):
            q = points.copy()
            q[:, 4:7] = directions(points, (SEED * SPP + s) & 0xffffffff)
            sample_rays.append(q)
        make_s = time.perf_counter() - t0

        def gather():
            t0 = time.perf_counter()
            res = r.gatherIrradiance(points, DEPTH, SPP, SEED)
            wall = time.perf_counter() - t0
            return res, r.irradianceGatherStats(), wall * 1e3

        def composed():
            col = np.zeros((n, 3), np.float32)
            kernel, wall, traced = 0.0, 0.0, 0
            for s in range(SPP):
                t0 = time.perf_counter()
                res = r.traceRadiance(sample_rays[s], DEPTH, 1, (SEED * SPP + s) & 0xffffffff)
                col = col + res["rgb"]
                wall += time.perf_counter() - t0
                st = r.radianceQueryStats()
                kernel += st["kernel_ms"]
                traced += st["extension_rays"] + st["shadow_rays"]
            t0 = time.perf_counter()
            col = col / np.float32(SPP)
            wall += time.perf_counter() - t0
            return col, kernel, wall * 1e3, traced

        res, st, _ = gather()
        col, _, _, traced = composed()
        form = "%s form, %d workgroups" % ("LDS" if st["lds"] else "global-memory", st["workgroups"])
        means = (res["rgb"].astype(np.float64).mean(), col.astype(np.float64).mean())
        per_sample = (st["extension_rays"] + st["shadow_rays"]) / (n * SPP)
        ms = {"gather kernel": [], "composed kernels": [], "gather wall": [], "composed wall": []}
        for _ in range(ROUNDS):
            _, st, wall = gather()
            ms["gather kernel"].append(st["kernel_ms"])
            ms["gather wall"].append(wall)
            _, kernel, wall, _ = composed()
            ms["composed kernels"].append(kernel)
            ms["composed wall"].append(wall)
        lines.append("%s: %s; %d of %d camera rays hit; %.2f rays traced per sample (composed route: %.2f); mean rgb "
                     "%.5f (composed route: %.5f); host directions %.1f ms, not in the wall times"
                     % (scene, form, int(hit.sum()), n, per_sample, traced / (n * SPP), means[0], means[1], make_s * 1e3))
        for name in ("gather kernel", "composed kernels"):
            lines.append("  %-17s %s; %s" % (name, fmt([n * SPP / (v * 1e-3) * 1e-6 for v in ms[name]], "Msamples/s"), fmt(ms[name], "ms")))
        for name in ("gather wall", "composed wall"):
            lines.append("  %-17s %s" % (name, fmt(ms[name], "ms")))
        r.destroy()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
