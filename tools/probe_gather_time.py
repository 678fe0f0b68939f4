"""Rate of the probe gather (rt_gather_probes) beside the route that existed before it, from one process.

Per scene (cornell, sponza_like): 4096 probes, the cell centres of a 16 x 16 x 16 grid in the scene's bounds (the TLAS root),
spp = 1024, depth 4 - 2^22 samples, one batch:
  probes     one rt_gather_probes call: the wall time of the call (probes up, 112 B per probe down) and the summed kernel_ms of
             its radiance launches (rt_probe_gather_stats).  k_probe_rays + k_probe_project: the same gather through
             rt_gather_probes_device between two device events on the context's stream, minus that call's kernel_ms (the two
             small counter memsets of the launch are in this figure too).
  composed   the same samples as ONE rt_trace_radiance call (spp = 1, seed = 0) on n * spp host-made rays with pad' = pad + f *
             719393 (32 B per sample up, 16 B per sample down), then the SH9 projection in numpy: wall time and kernel_ms of the
             query, wall time of the projection.  The directions are the probe rule restated in numpy (equal up to the rounding
             of sin / cos); making the rays is timed apart and is not part of the wall time.
Device events for the kernel times; one warm-up pass; 5 rounds that alternate the two routes; every figure is the median of
the rounds with (min .. max) beside it.  Nothing is gated on these numbers.  What to hold the first run against: radiance
kernel time within the spread of the composed route's (the same rays), wall time lower by the transfers and the host
projection.

usage: python tools/probe_gather_time.py [--out profiles/probe_gather_rate.txt] [--scenes cornell,sponza_like]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from webgpu_raytracer_amd import renderer as R  # noqa: E402
from timing_util import fmt, init_rng, rand_pcg  # noqa: E402

GRID, DEPTH, SPP, ROUNDS, SEED = 16, 4, 1024, 5, 5
RNG_STEP = np.uint32(719393)


def grid_probes(bridge):
    root = np.asarray(bridge.tlas, np.float32).reshape(-1, 8)[0]
    lo, hi = root[0:3].astype(np.float64), root[4:7].astype(np.float64)
    g = (np.arange(GRID) + 0.5) / GRID
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * (hi - lo) + lo
    p = np.zeros((pos.shape[0], 8), np.float32)
    p[:, 0:3] = pos
    p[:, 3] = 1e30
    p.view(np.uint32)[:, 7] = np.arange(pos.shape[0], dtype=np.uint32)
    return p


def host_rays(probes):
    """(rays (n * spp, 8) with pad', directions (n * spp, 3)): the probe rule's uniform-sphere directions in float32 numpy"""
    n = probes.shape[0]
    pads = np.repeat(probes.view(np.uint32)[:, 7], SPP)
    f = np.tile(((SEED * SPP + np.arange(SPP, dtype=np.uint64)) & 0xffffffff).astype(np.uint32), n)
    rng = init_rng(pads ^ np.uint32(0x80000000), f)
    u1, u2 = rand_pcg(rng), rand_pcg(rng)
    with np.errstate(over="ignore"):
        pad_prime = pads + f * RNG_STEP
    z = np.float32(1) - np.float32(2) * u1
    rad = np.sqrt(np.maximum(np.float32(0), np.float32(1) - z * z))
    phi = np.float32(2 * np.pi) * u2
    d = np.stack([rad * np.cos(phi), rad * np.sin(phi), z], axis=1).astype(np.float32)
    rays = np.repeat(probes, SPP, axis=0)
    rays[:, 4:7] = d
    rays.view(np.uint32)[:, 7] = pad_prime
    return rays, d


def host_projection(res, dirs, n):
    """the numpy projection of n * spp radiance results: (n, 9, 3) float32 (plain summation order)"""
    Y = R.sh9_basis(dirs).astype(np.float32)
    terms = Y[:, :, None] * res["rgb"][:, None, :]
    return terms.reshape(n, SPP, 9, 3).sum(axis=1, dtype=np.float32) * np.float32(4 * np.pi / SPP)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", default="cornell,sponza_like")
    args = ap.parse_args()
    n = GRID ** 3
    lines = ["probe gather rate, %d probes, spp %d, depth %d; Msamples/s = 1e-6 * probes * spp / radiance kernel seconds" % (n, SPP, DEPTH)]
    for scene in args.scenes.split(","):
        b = W.WorldBridge()
        b.loadScene(scene)
        r = W.WebGPURenderer(0)
        W.upload_scene(r, b, 16, 16)
        r.setKernelTiming(True)
        probes = grid_probes(b)
        t0 = time.perf_counter()
        rays, dirs = host_rays(probes)
        make_s = time.perf_counter() - t0
        stream = torch.cuda.Stream()
        d_probes = torch.from_numpy(probes).cuda()
        d_out = torch.empty((n, 28), dtype=torch.float32, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def probe_route():
            t0 = time.perf_counter()
            res = r.gatherProbes(probes, DEPTH, SPP, SEED)
            wall = (time.perf_counter() - t0) * 1e3
            st = r.probeGatherStats()
            r.setStream(stream.cuda_stream)
            with torch.cuda.stream(stream):
                ev[0].record(stream)
                r.gatherProbesDevice(d_probes.data_ptr(), n, d_out.data_ptr(), DEPTH, SPP, SEED)
                ev[1].record(stream)
            stream.synchronize()
            around = ev[0].elapsed_time(ev[1]) - r.probeGatherStats()["kernel_ms"]
            r.setStream(None)
            return res, st, wall, around

        def composed_route():
            t0 = time.perf_counter()
            res = r.traceRadiance(rays, DEPTH, 1, 0)
            wall = (time.perf_counter() - t0) * 1e3
            st = r.radianceQueryStats()
            t0 = time.perf_counter()
            sh = host_projection(res, dirs, n)
            return sh, st, wall, (time.perf_counter() - t0) * 1e3

        res, st, _, _ = probe_route()
        sh, st_c, _, _ = composed_route()
        form = "%s form, %d workgroups" % ("LDS" if st["lds"] else "global-memory", st["workgroups"])
        per_sample = (st["extension_rays"] + st["shadow_rays"]) / (n * SPP)
        per_sample_c = (st_c["extension_rays"] + st_c["shadow_rays"]) / (n * SPP)
        ms = {"probes radiance kernel": [], "composed radiance kernel": [], "probes rays + project": [], "probes wall": [],
              "composed query wall": [], "composed projection wall": []}
        for _ in range(ROUNDS):
            _, st, wall, around = probe_route()
            ms["probes radiance kernel"].append(st["kernel_ms"])
            ms["probes rays + project"].append(around)
            ms["probes wall"].append(wall)
            _, st_c, wall, proj = composed_route()
            ms["composed radiance kernel"].append(st_c["kernel_ms"])
            ms["composed query wall"].append(wall)
            ms["composed projection wall"].append(proj)
        lines.append("%s: %s; mean hit fraction %.3f; %.2f rays traced per sample (composed route: %.2f); mean sh[0] %.5f "
                     "(composed route: %.5f); host rays %.1f ms, not in the wall times"
                     % (scene, form, float(res["hit_fraction"].mean()), per_sample, per_sample_c,
                        float(res["sh"][:, 0, :].astype(np.float64).mean()), float(sh[:, 0, :].astype(np.float64).mean()), make_s * 1e3))
        for name in ("probes radiance kernel", "composed radiance kernel"):
            lines.append("  %-25s %s; %s" % (name, fmt([n * SPP / (v * 1e-3) * 1e-6 for v in ms[name]], "Msamples/s"), fmt(ms[name], "ms")))
        for name in ("probes rays + project", "probes wall", "composed query wall", "composed projection wall"):
            lines.append("  %-25s %s" % (name, fmt(ms[name], "ms")))
        r.destroy()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
