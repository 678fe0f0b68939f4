"""Rate of the directional gather (rt_gather_directional) beside the irradiance gather on the same points, from one process.

Per scene (cornell, sponza_like): the covered texels of a 1024 x 1024 atlas - the first instances of the scene (at most 64), one
square rectangle each, the chart layout of atlas_bake_time.py - as bakeAtlasPoints gives them; depth 4; spp 16 and 64:
  directional  one rt_gather_directional call: the wall time of the call (32 B per point up, 64 B per point down) and the summed
               kernel_ms of its radiance launches (rt_directional_gather_stats).  k_dir_rays + k_dir_project: the same gather
               through rt_gather_directional_device between two device events on the context's stream, minus that call's
               kernel_ms (the small counter memsets of the launches are in this figure too).
  irradiance   one rt_gather_irradiance call on the same points: wall time (16 B per point down) and kernel_ms of its one
               launch, k_irradiance_gather, in which a lane keeps its point for all spp samples.
The two gathers draw different directions (uniform on the hemisphere / cosine-distributed), so their paths differ: the rays
traced per sample are printed beside the rates.  Device events for the kernel times; one warm-up pass; 5 rounds that alternate
the two routes; every figure is the median of the rounds with (min .. max) beside it.  Nothing is gated on these numbers.

usage: python tools/directional_gather_time.py [--out profiles/directional_gather_rate.txt] [--scenes cornell,sponza_like]"""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from atlas_bake_time import merged_grid_uv  # noqa: E402
from timing_util import fmt  # noqa: E402

ATLAS, MAX_ENTRIES, DEPTH, SPPS, ROUNDS, SEED = 1024, 64, 4, (16, 64), 5, 5


def atlas_points(r, b):
    n_inst = np.asarray(b.draw_commands).size // 4
    n = min(n_inst, MAX_ENTRIES)
    side = math.ceil(math.sqrt(n))
    cell = ATLAS // side
    insts = list(range(n))
    entries = [(e, (e % side) * cell, (e // side) * cell, cell, cell) for e in insts]
    uv = merged_grid_uv(b, insts)[0]
    points, texels = r.bakeAtlasPoints(entries, ATLAS, ATLAS, atlas_uv=uv)
    return np.ascontiguousarray(points), n, cell


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", default="cornell,sponza_like")
    args = ap.parse_args()
    lines = ["directional gather rate beside the irradiance gather on the same points, depth %d; Msamples/s = 1e-6 * points * spp / "
             "radiance kernel seconds" % DEPTH]
    for scene in args.scenes.split(","):
        b = W.WorldBridge()
        b.loadScene(scene)
        r = W.WebGPURenderer(0)
        W.upload_scene(r, b, 16, 16)
        r.setKernelTiming(True)
        points, n_entries, cell = atlas_points(r, b)
        n = points.shape[0]
        stream = torch.cuda.Stream()
        d_points = torch.from_numpy(points).cuda()
        d_out = torch.empty((n, 16), dtype=torch.float32, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        lines.append("%s: %d points, the covered texels of a %d x %d atlas of %d entries of %d x %d texels"
                     % (scene, n, ATLAS, ATLAS, n_entries, cell, cell))
        for spp in SPPS:
            def directional_route():
                t0 = time.perf_counter()
                res = r.gatherDirectional(points, DEPTH, spp, SEED)
                wall = (time.perf_counter() - t0) * 1e3
                st = r.directionalGatherStats()
                r.setStream(stream.cuda_stream)
                with torch.cuda.stream(stream):
                    ev[0].record(stream)
                    r.gatherDirectionalDevice(d_points.data_ptr(), n, d_out.data_ptr(), DEPTH, spp, SEED)
                    ev[1].record(stream)
                stream.synchronize()
                around = ev[0].elapsed_time(ev[1]) - r.directionalGatherStats()["kernel_ms"]
                r.setStream(None)
                return res, st, wall, around

            def irradiance_route():
                t0 = time.perf_counter()
                res = r.gatherIrradiance(points, DEPTH, spp, SEED)
                wall = (time.perf_counter() - t0) * 1e3
                return res, r.irradianceGatherStats(), wall

            res, st, _, _ = directional_route()          # the warm-up
            res_i, st_i, _ = irradiance_route()
            ms = {"directional radiance kernel": [], "irradiance gather kernel": [], "directional rays + project": [],
                  "directional wall": [], "irradiance wall": []}
            for _ in range(ROUNDS):
                _, st, wall, around = directional_route()
                ms["directional radiance kernel"].append(st["kernel_ms"])
                ms["directional rays + project"].append(around)
                ms["directional wall"].append(wall)
                _, st_i, wall = irradiance_route()
                ms["irradiance gather kernel"].append(st_i["kernel_ms"])
                ms["irradiance wall"].append(wall)
            batches = -(-n // ((1 << 22) // spp))
            lines.append("  spp %d: %s form, %d radiance launch(es) of %d workgroups in all (irradiance gather: %d); hit fraction %.3f "
                         "(irradiance: %.3f); %.2f rays traced per sample (irradiance: %.2f); mean layer 0 %.5f, mean |band 1| %.5f"
                         % (spp, "LDS" if st["lds"] else "global-memory", batches, st["workgroups"], st_i["workgroups"],
                            float(res["layer"][:, 0, 3].mean()), float(res_i["hit_fraction"].mean()),
                            (st["extension_rays"] + st["shadow_rays"]) / (n * spp),
                            (st_i["extension_rays"] + st_i["shadow_rays"]) / (n * spp),
                            float(res["layer"][:, 0, :3].astype(np.float64).mean()),
                            float(np.abs(res["layer"][:, 1:, :3].astype(np.float64)).mean())))
            for name in ("directional radiance kernel", "irradiance gather kernel"):
                lines.append("    %-27s %s; %s" % (name, fmt([n * spp / (v * 1e-3) * 1e-6 for v in ms[name]], "Msamples/s"), fmt(ms[name], "ms")))
            for name in ("directional rays + project", "directional wall", "irradiance wall"):
                lines.append("    %-27s %s" % (name, fmt(ms[name], "ms")))
        r.destroy()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
