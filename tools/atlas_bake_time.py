"""Wall time of a whole-scene lightmap bake in ONE call (rt_bake_atlas_irradiance) beside the route that existed before it:
one rt_bake_irradiance call per instance, from one process.

Scene instanced1000 (1001 instances over four geometries).  1024 entries - instances 0 .. 1000 and 23 repeats (instances
0 .. 22 again) - as a 32 x 32 grid of 32 x 32 rectangles in a 1024 x 1024 atlas; the chart layout is one triangle per cell
of a ceil(sqrt(n)) grid of the unit square per distinct geometry, merged into one override array (the layout of the
atlas-bake tests); depth 4, spp 16.
  atlas   one bakeAtlasIrradiance: one point pass, one gather, one scatter, one copy back
  loop    1024 bakeIrradiance calls on 32 x 32 atlases, one per entry: each a memset, four launches, a blocking read of the
          count, a gather, a scatter and a copy back (the host-side blit of the results into one atlas is NOT included)
Per route: the wall time around the call(s) and the summed kernel_ms of the gather stats.  One warm-up of each, then five
rounds, the two routes alternated; every figure the median with (min .. max).  Nothing is gated on these numbers.

usage: python tools/atlas_bake_time.py [--out profiles/atlas_bake_rate.txt]"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from timing_util import fmt2 as fmt  # noqa: E402,F401  (dilate_time, denoise_time and lightmap_time take it from here)

SCENE, CELL, SIDE, DEPTH, SPP, ROUNDS, SEED = "instanced1000", 32, 32, 4, 16, 5, 5


def merged_grid_uv(bridge, insts):
    """one triangle per grid cell for every distinct geometry among insts; vertices no such triangle uses at (-1, -1)"""
    dc = np.asarray(bridge.draw_commands, np.uint32).reshape(-1, 4)
    topo = np.asarray(bridge.mesh_topology, np.uint32).reshape(-1, 20)
    uv = np.full((np.asarray(bridge.uvs).size // 2, 2), -1.0, np.float32)
    corner = np.array([[0.11, 0.13], [0.89, 0.12], [0.12, 0.87]])
    seen = set()
    for inst in insts:
        first, count = int(dc[inst, 2]) // 3, int(dc[inst, 0]) // 3
        if (first, count) in seen:
            continue
        seen.add((first, count))
        g = max(1, math.ceil(math.sqrt(max(count, 1))))
        for j in range(min(count, len(topo) - first)):
            uv[topo[first + j, 0:3]] = ((np.array([j % g, j // g], np.float64) + corner) / g).astype(np.float32)
    return uv, len(seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    b = W.WorldBridge()
    b.loadScene(SCENE)
    r = W.WebGPURenderer(0)
    W.upload_scene(r, b, 16, 16)
    r.setKernelTiming(True)      # kernel_ms of the gather stats: events around the gather launch
    n_inst = np.asarray(b.draw_commands).size // 4
    n = SIDE * SIDE
    insts = [e % n_inst for e in range(n)]
    entries = [(insts[e], (e % SIDE) * CELL, (e // SIDE) * CELL, CELL, CELL) for e in range(n)]
    uv, n_geom = merged_grid_uv(b, insts)
    size = SIDE * CELL

    def atlas():
        t0 = time.perf_counter()
        _, covered, st = r.bakeAtlasIrradiance(entries, size, size, DEPTH, SPP, SEED, atlas_uv=uv, stats=True)
        return (time.perf_counter() - t0) * 1e3, st["kernel_ms"], covered

    def loop():
        t0 = time.perf_counter()
        kernel, covered = 0.0, 0
        for inst in insts:
            _, c, st = r.bakeIrradiance(inst, CELL, CELL, DEPTH, SPP, SEED, atlas_uv=uv, stats=True)
            kernel += st["kernel_ms"]
            covered += c
        return (time.perf_counter() - t0) * 1e3, kernel, covered

    covered_a, covered_l = atlas()[2], loop()[2]      # the warm-up
    res = {"atlas": ([], []), "loop": ([], [])}
    for _ in range(ROUNDS):
        for name, fn in (("atlas", atlas), ("loop", loop)):
            wall, kernel, _ = fn()
            res[name][0].append(wall)
            res[name][1].append(kernel)
    r.destroy()
    lines = ["whole-scene lightmap bake, %s: %d entries (%d instances, %d geometries) as %d x %d rectangles of %d x %d texels in a "
             "%d x %d atlas; gather at depth %d, spp %d" % (SCENE, n, n_inst, n_geom, SIDE, SIDE, CELL, CELL, size, size, DEPTH, SPP),
             "covered texels: atlas %d, loop %d (summed over the calls)" % (covered_a, covered_l)]
    for name, what in (("atlas", "one bakeAtlasIrradiance"), ("loop", "%d bakeIrradiance calls" % n)):
        lines.append("%-28s wall %s; gather kernel_ms summed %s" % (what, fmt(res[name][0]), fmt(res[name][1])))
    wa, wl = statistics.median(res["atlas"][0]), statistics.median(res["loop"][0])
    lines.append("loop wall / atlas wall = %.1f" % (wl / wa))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
