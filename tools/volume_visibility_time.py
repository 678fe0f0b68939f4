"""Rates of probe visibility maps (rt_bake_volume_visibility, rt_sample_volume_visible_device) beside what existed before
them, from one process, on the 16 x 16 x 16 cornell volume of tools/volume_time.py.

(a) sample: 2^22 points through rt_sample_volume_visible_device between two device events, against rt_sample_volume_device -
    the parent commit's sampler, whose code this feature leaves as it was - on the same points (the coherent sheet and the
    random set of tools/volume_time.py), at map sizes 8 and 16, with flags = 0 and no crush ("plain") and with the backface
    weight and a crush threshold ("full").  points/s and the ratio to the plain sampler's median.  The visible sampler reads
    32 more 8-byte taps per point, from maps of 512 B (size 8) or 2 KiB (size 16) per probe: 2 MiB or 8 MiB for the volume.
(b) bake: the maps at 4 samples per texel - 2^20 rays at size 8, 2^22 at size 16, one batch each - the summed kernel_ms of the
    bake's ray launches (rt_volume_visibility_stats) against one rt_trace_rays_device call on the rule's own rays, restated
    in numpy float32 (rt_ray_query_stats); the bake's other two kernels from a device-event pair around the whole call.
Device events for the kernel times; one warm-up pass; 5 rounds that alternate the routes; every figure is the median of the
rounds with (min .. max) beside it.  Nothing is gated on these numbers.  What to hold the first run against:
the visible sampler between 1.5 and 2.5 times the plain sampler's time, the arithmetic rather than the taps being the cost; the
bake's ray time within the spread of the ray query's.

usage: python tools/volume_visibility_time.py [--out profiles/volume_visibility_rate.txt]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from webgpu_raytracer_amd import renderer as R  # noqa: E402
from timing_util import fmt  # noqa: E402
from volume_time import GRID, N_POINTS, grid_desc, host_probes, sample_points  # noqa: E402

ROUNDS, SEED, SPT = 5, 5, 4
SIZES = (8, 16)


def vis_desc(d, size, full):
    cell = float(np.linalg.norm(np.asarray(d["step"], np.float64)))
    return R.volume_visibility_desc(size, 1.5 * cell, spt=SPT, normal_bias=0.01 * cell, crush_threshold=0.2 if full else 0.0,
                                    backface=full)


def rule_rays(d, v, seed):
    """the rays of THE VISIBILITY RULE in numpy float32 (to rounding; a timing needs no more): (n * size^2 * spt, 8) f32"""
    size, spt = int(v["size"]), int(v["spt"])
    probes = host_probes(d)
    n = probes.shape[0]
    T = np.arange(n * size * size, dtype=np.uint32)
    s = np.arange(spt, dtype=np.uint32)
    pad_t = (np.uint32(int(d["pad_first"])) + T)[:, None]
    f = (np.uint32(seed * spt) + s)[None, :]
    with np.errstate(over="ignore"):
        st = (pad_t ^ np.uint32(0x80000000)) + f * np.uint32(719393)
        st ^= np.uint32(2747636419)
        st *= np.uint32(2654435769)
        st ^= st >> np.uint32(16)
        st *= np.uint32(2654435769)
        st ^= st >> np.uint32(16)
        st *= np.uint32(2654435769)
        jit = []
        for _ in range(2):
            old = st
            st = old * np.uint32(747796405) + np.uint32(2891336453)
            word = (st >> ((old >> np.uint32(28)) + np.uint32(4))) ^ st
            jit.append(((word >> np.uint32(22)) ^ word).astype(np.float32) * np.float32(2.3283064365386962890625e-10))
    t = T % np.uint32(size * size)
    px = ((t % np.uint32(size)).astype(np.float32)[:, None] + jit[0]) / np.float32(size) * np.float32(2) - np.float32(1)
    py = ((t // np.uint32(size)).astype(np.float32)[:, None] + jit[1]) / np.float32(size) * np.float32(2) - np.float32(1)
    z = np.float32(1) - np.abs(px) - np.abs(py)
    fold = np.clip(-z, np.float32(0), np.float32(1))
    x = px + np.where(px >= 0, -fold, fold)
    y = py + np.where(py >= 0, -fold, fold)
    inv = np.float32(1) / np.sqrt(x * x + y * y + z * z)
    rays = np.zeros((n * size * size, spt, 8), np.float32)
    rays[:, :, 0:3] = np.repeat(probes[:, 0:3], size * size, axis=0)[:, None, :]
    rays[:, :, 3] = v["max_distance"]
    rays[:, :, 4], rays[:, :, 5], rays[:, :, 6] = x * inv, y * inv, z * inv
    rays.view(np.uint32)[:, :, 7] = pad_t
    return rays.reshape(-1, 8)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    b = W.WorldBridge()
    b.loadScene("cornell")
    r = W.WebGPURenderer(0)
    W.upload_scene(r, b, 16, 16)
    r.setKernelTiming(True)
    d = grid_desc(b)
    n = GRID ** 3
    vol = r.bakeVolume(d, 4, 64, SEED)
    stream = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    lines = ["probe visibility maps on the %d^3 cornell volume; every figure the median of %d alternated rounds" % (GRID, ROUNDS)]

    def timed(fn):
        with torch.cuda.stream(stream):
            ev[0].record(stream)
            fn()
            ev[1].record(stream)
        stream.synchronize()
        return ev[0].elapsed_time(ev[1])

    # ---- (b) the bake
    maps = {}
    for size in SIZES:
        v = vis_desc(d, size, False)
        n_rays = n * size * size * SPT
        d_maps = torch.empty((n * size * size, 2), dtype=torch.float32, device="cuda")
        d_rays = torch.from_numpy(rule_rays(d, v, SEED)).cuda()
        d_hits = torch.empty((n_rays, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.setStream(stream.cuda_stream)

        def bake():
            whole = timed(lambda: r.bakeVolumeVisibilityDevice(d, v, d_maps.data_ptr(), SEED))
            st = r.volumeVisibilityStats()
            return st, whole - st["kernel_ms"]

        def query():
            timed(lambda: r.traceRaysDevice(d_rays.data_ptr(), n_rays, d_hits.data_ptr()))
            return r.rayQueryStats()

        st, _ = bake()
        st_q = query()
        ms = {"bake ray kernel": [], "ray query kernel": [], "bake kernels around": []}
        for _ in range(ROUNDS):
            st, around = bake()
            ms["bake ray kernel"].append(st["kernel_ms"])
            ms["bake kernels around"].append(around)
            ms["ray query kernel"].append(query()["kernel_ms"])
        r.setStream(None)
        maps[size] = d_maps
        m = d_maps.cpu().numpy()
        lines.append("bake, size %d, spt %d: %d rays, %s form, %d workgroups (the query: %d); mean distance %.3f of max_distance %.3f"
                     % (size, SPT, n_rays, "LDS" if st["lds"] else "global-memory", st["workgroups"], st_q["workgroups"],
                        float(m[:, 0].mean()), float(v["max_distance"])))
        for name in ("bake ray kernel", "ray query kernel"):
            lines.append("  %-25s %s; %s" % (name, fmt([n_rays / (x * 1e-3) * 1e-6 for x in ms[name]], "Mrays/s"), fmt(ms[name], "ms")))
        lines.append("  %-25s %s" % ("bake kernels around", fmt(ms["bake kernels around"], "ms")))
        del d_rays, d_hits

    # ---- (a) the sampler
    d_vol = torch.from_numpy(np.ascontiguousarray(vol).reshape(-1).view(np.float32).copy()).cuda()
    d_res = torch.empty((N_POINTS, 4), dtype=torch.float32, device="cuda")
    sets = {name: torch.from_numpy(sample_points(b, coherent)).cuda() for name, coherent in (("coherent", True), ("random", False))}
    torch.cuda.synchronize()
    r.setStream(stream.cuda_stream)
    routes = {"plain sampler": lambda pts: r.sampleVolumeDevice(d, d_vol.data_ptr(), pts.data_ptr(), N_POINTS, d_res.data_ptr())}
    for size in SIZES:
        for full in (False, True):
            v = vis_desc(d, size, full)
            routes["visible, size %d, %s" % (size, "full" if full else "plain")] = (
                lambda pts, v=v, size=size: r.sampleVolumeVisibleDevice(d, v, d_vol.data_ptr(), maps[size].data_ptr(), pts.data_ptr(),
                                                                        N_POINTS, d_res.data_ptr()))
    for name, pts in sets.items():
        ms = {route: [] for route in routes}
        for route, fn in routes.items():
            timed(lambda: fn(pts))
        for _ in range(ROUNDS):
            for route, fn in routes.items():
                ms[route].append(timed(lambda: fn(pts)))
        base = float(np.median(ms["plain sampler"]))
        lines.append("sampler, %d %s points" % (N_POINTS, name))
        for route in routes:
            lines.append("  %-25s %s; %s; %.2f x the plain sampler" % (
                route, fmt(ms[route], "ms"), fmt([N_POINTS / (x * 1e-3) * 1e-9 for x in ms[route]], "Gpoints/s"),
                float(np.median(ms[route])) / base))
        got = d_res.cpu().numpy()
        lines.append("  the last route's results: mean E %.4f, mean W %.4f" % (float(got[:, :3].mean()), float(got[:, 3].mean())))
    r.setStream(None)
    r.destroy()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
