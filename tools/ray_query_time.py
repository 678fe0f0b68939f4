"""Rate of the ray query (rt_trace_rays_device) beside the product's own closest-hit trace rate, from one process.

Per scene (cornell, instanced1000, sponza_like):
  ordered    1920 x 1080 pinhole rays of the scene camera, in row order       } closest hit, rays as a torch tensor on the
  shuffled   the same rays in a random order                                  } device, kernel_ms of rt_ray_query_stats
  wavefront  extension rays of rt_get_counters over RT_TIMER_WF_TRACE_EXT of rt_kernel_times: wavefront form, depth 8,
             1920 x 1080, batches of 4 frames
Device events only; one warm-up pass; 5 rounds that alternate the three measurements; every figure is the median of the
rounds with (min .. max) beside it, and each round of a query set repeats until it has >= 0.1 s of kernel time (>= 0.5 s
over the rounds).  Nothing is gated on these numbers.

usage: python tools/ray_query_time.py [--out profiles/ray_query_rate.txt] [--scenes cornell,instanced1000,sponza_like]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from timing_util import camera_rays, fmt  # noqa: E402

WIDTH, HEIGHT, DEPTH, BATCH, ROUNDS = 1920, 1080, 8, 4, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", default="cornell,instanced1000,sponza_like")
    args = ap.parse_args()
    import torch
    lines = ["ray query rate, %d x %d rays, closest hit; Grays/s = 1e-9 * rays / kernel seconds" % (WIDTH, HEIGHT)]
    for scene in args.scenes.split(","):
        b = W.WorldBridge()
        b.loadScene(scene)
        r = W.WebGPURenderer(0)
        r.buildPipeline(DEPTH, 1)
        W.upload_scene(r, b, WIDTH, HEIGHT)
        r.setKernelVariant(2)
        r.setKernelTiming(True)
        rays = camera_rays(b, WIDTH, HEIGHT)
        n = rays.shape[0]
        sets = {"ordered": torch.from_numpy(rays).cuda(),
                "shuffled": torch.from_numpy(rays[np.random.default_rng(1).permutation(n)]).cuda()}
        hits = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def query(t):
            r.traceRaysDevice(t.data_ptr(), n, hits.data_ptr())
            return r.rayQueryStats()

        def wavefront(first):
            c0 = r.getCounters()["extension_rays"]
            r.kernelTimes()
            r.computeBatch(list(range(first, first + BATCH)))
            r.sync()
            ms = r.kernelTimes()["wf_trace_ext"]["ms"]
            return (r.getCounters()["extension_rays"] - c0) / (ms * 1e-3) * 1e-9

        st = query(sets["ordered"])
        form = "%s walk, %s%s, %d workgroups" % ("pair" if st["walk"] else "node", "LDS" if st["lds"] else "mixed / global",
                                                  ", RAYREG" if st["rayreg"] else "", st["workgroups"])
        n_hit = int((hits[:, 3] != 0).sum())
        query(sets["shuffled"])
        wavefront(1)
        rate = {"ordered": [], "shuffled": [], "wavefront": []}
        for k in range(ROUNDS):
            for name, t in sets.items():
                ms, reps = 0.0, 0
                while ms < 100.0:
                    ms += query(t)["kernel_ms"]
                    reps += 1
                rate[name].append(reps * n / (ms * 1e-3) * 1e-9)
            rate["wavefront"].append(wavefront(1 + BATCH * (k + 1)))
        lines.append("%s: %s; %d of %d camera rays hit" % (scene, form, n_hit, n))
        for name in ("ordered", "shuffled", "wavefront"):
            lines.append("  %-10s %s" % (name, fmt(rate[name], "Grays/s")))
        r.destroy()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
