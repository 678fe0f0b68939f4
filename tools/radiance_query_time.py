"""Rate of the radiance query (rt_trace_radiance_device) beside the render's own path for the same work, from one process.

Per scene (cornell, instanced1000, sponza_like), at spp = 1 and depth 8:
  ordered    1920 x 1080 pinhole rays of the scene camera, in row order, pad = pixel index  } rays as a torch tensor on the
  shuffled   the same rays in a random order                                                 } device, kernel_ms of
                                                                                               rt_radiance_query_stats
  frame      one rt_compute frame of the same camera with the persistent kernel: RT_TIMER_PRIMARY + RT_TIMER_PATHTRACE of
             rt_kernel_times (the G-buffer pass is the render's first segment)
Device events only; one warm-up pass; 5 rounds that alternate the three measurements; every figure is the median of the
rounds with (min .. max) beside it, and each round repeats its measurement until it has >= 0.1 s of kernel time.  Nothing is
gated on these numbers.  What to hold the first run against: ordered rays on a scene in the global-memory form within the
spread of a frame of the persistent kernel's global form; cornell slower than the render, which uses the one-leaf form this
kernel lacks.

usage: python tools/radiance_query_time.py [--out profiles/radiance_query_rate.txt] [--scenes cornell,instanced1000,sponza_like]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ray_query_time import WIDTH, HEIGHT  # noqa: E402
from timing_util import camera_rays, fmt  # noqa: E402

DEPTH, SPP, ROUNDS = 8, 1, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", default="cornell,instanced1000,sponza_like")
    args = ap.parse_args()
    import torch
    lines = ["radiance query rate, %d x %d rays, spp %d, depth %d; Mrays/s = 1e-6 * rays / kernel seconds" % (WIDTH, HEIGHT, SPP, DEPTH)]
    for scene in args.scenes.split(","):
        b = W.WorldBridge()
        b.loadScene(scene)
        r = W.WebGPURenderer(0)
        r.buildPipeline(DEPTH, SPP)
        W.upload_scene(r, b, WIDTH, HEIGHT)
        r.setKernelVariant(1)
        r.setKernelTiming(True)
        rays = camera_rays(b, WIDTH, HEIGHT)
        n = rays.shape[0]
        rays.view(np.uint32)[:, 7] = np.arange(n, dtype=np.uint32)
        sets = {"ordered": torch.from_numpy(rays).cuda(),
                "shuffled": torch.from_numpy(rays[np.random.default_rng(1).permutation(n)]).cuda()}
        out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def query(t, seed):
            r.traceRadianceDevice(t.data_ptr(), n, out.data_ptr(), DEPTH, SPP, seed)
            return r.radianceQueryStats()

        def frame(f):
            r.kernelTimes()
            r.compute(f)
            r.sync()
            kt = r.kernelTimes()
            return kt["primary"]["ms"] + kt["pathtrace"]["ms"]

        st = query(sets["ordered"], 1)
        form = "%s form, %d workgroups" % ("LDS" if st["lds"] else "global-memory", st["workgroups"])
        n_hit = int((out[:, 3] < 1e30).sum())
        per_ray = (st["extension_rays"] + st["shadow_rays"]) / n
        query(sets["shuffled"], 1)
        frame(1)
        ms = {"ordered": [], "shuffled": [], "frame": []}   # per round: mean kernel time of one query / one frame
        next_frame = 2
        for k in range(ROUNDS):
            for name, t in sets.items():
                total, reps = 0.0, 0
                while total < 100.0:
                    total += query(t, 2 + k)["kernel_ms"]
                    reps += 1
                ms[name].append(total / reps)
            total, reps = 0.0, 0
            while total < 100.0:
                total += frame(next_frame)
                next_frame += 1
                reps += 1
            ms["frame"].append(total / reps)
        lines.append("%s: %s; %d of %d camera rays hit; %.2f rays traced per query ray" % (scene, form, n_hit, n, per_ray))
        for name in ("ordered", "shuffled", "frame"):
            lines.append("  %-10s %s; %s" % (name, fmt([n / (v * 1e-3) * 1e-6 for v in ms[name]], "Mrays/s"), fmt(ms[name], "ms")))
        r.destroy()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
