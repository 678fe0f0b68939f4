"""Wall time of the finished lightmap in ONE call (rt_bake_atlas_lightmap: bake, filter, gutter fill and encode on the device,
one copy back) at its three texel formats, beside the slow route of the same build, bakeAtlasIrradiance(denoise=..., dilate=...):
the bake, a second point pass on host arrays for the filter's guides, denoiseAtlas and dilateAtlas, each with its own round
trips of the atlas.  The comparison is always against the slow route, never against the new call alone.

Scene instanced1000, 1024 entries as 32 x 32 rectangles of 32 x 32 texels in a 1024 x 1024 atlas, depth 4, spp 16 (the
entries, layout and seed of atlas_bake_time.py); the filter of denoise_time.py at 3 passes (normal_cos 0.9, plane_eps 0.02,
max_dist 0.5, step 1); a gutter of radius 4.
  one call  bakeAtlasLightmap at "f32", "f16" and "rgbe": wall time around the call
  slow      bakeAtlasIrradiance(denoise=..., dilate=4): wall time around the call; its words are compared with the f32 result
One warm-up of each, then five rounds, the four alternated; every figure the median with (min .. max).
  encode    k_encode_atlas alone: REPS encodeAtlasDevice calls back to back on a side stream between two device events, the
            elapsed time / REPS, per format; one warm-up, five rounds.
Nothing is gated on these numbers.

usage: python tools/lightmap_time.py [--out profiles/lightmap_rate.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from atlas_bake_time import CELL, DEPTH, SCENE, SEED, SIDE, SPP, fmt, merged_grid_uv  # noqa: E402

ROUNDS, REPS, RADIUS = 5, 20, 4
FILTER = dict(normal_cos=0.9, plane_eps=0.02, max_dist=0.5, passes=3, step=1)
FORMATS = (("f32", 16), ("f16", 8), ("rgbe", 4))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    b = W.WorldBridge()
    b.loadScene(SCENE)
    r = W.WebGPURenderer(0)
    W.upload_scene(r, b, 16, 16)
    n_inst = np.asarray(b.draw_commands).size // 4
    n = SIDE * SIDE
    insts = [e % n_inst for e in range(n)]
    entries = [(insts[e], (e % SIDE) * CELL, (e // SIDE) * CELL, CELL, CELL) for e in range(n)]
    uv, _ = merged_grid_uv(b, insts)
    size = SIDE * CELL

    def one_call(name):
        t0 = time.perf_counter()
        out, covered, filled, _ = r.bakeAtlasLightmap(entries, size, size, DEPTH, SPP, SEED, atlas_uv=uv, denoise=FILTER,
                                                      dilate=RADIUS, format=name, stats=True)
        return (time.perf_counter() - t0) * 1e3, out, covered, filled

    def slow():
        t0 = time.perf_counter()
        out, covered, _ = r.bakeAtlasIrradiance(entries, size, size, DEPTH, SPP, SEED, atlas_uv=uv, denoise=FILTER, dilate=RADIUS,
                                                stats=True)
        return (time.perf_counter() - t0) * 1e3, out, covered, None

    routes = [(name, (lambda name=name: one_call(name))) for name, _ in FORMATS] + [("slow", slow)]
    last = {name: fn() for name, fn in routes}         # the warm-up
    wall = {name: [] for name, _ in routes}
    for _ in range(ROUNDS):
        for name, fn in routes:
            last[name] = fn()
            wall[name].append(last[name][0])
    covered, filled = last["f32"][2], last["f32"][3]
    same = np.array_equal(np.ascontiguousarray(last["f32"][1]).view(np.uint32), np.ascontiguousarray(last["slow"][1]).view(np.uint32))
    lines = ["finished lightmap, %s: the %d x %d atlas of %d entries of %d x %d texels (depth %d, spp %d); %d of %d texels covered, "
             "%d filled by the gutter" % (SCENE, size, size, n, CELL, CELL, DEPTH, SPP, covered, size * size, filled),
             "filter: normal_cos %(normal_cos)g, plane_eps %(plane_eps)g, max_dist %(max_dist)g, step %(step)d, passes %(passes)d" % FILTER
             + "; gutter radius %d" % RADIUS]
    for name, bytes_per in FORMATS:
        lines.append("one call, bakeAtlasLightmap format %-4s (%2d MiB back)   wall %s"
                     % (name, size * size * bytes_per >> 20, fmt(wall[name])))
    lines.append("slow route, bakeAtlasIrradiance(denoise=, dilate=)     wall %s" % fmt(wall["slow"]))
    ms = statistics.median(wall["slow"])
    lines.append("slow wall - one-call wall: " + ", ".join("%s %.2f ms" % (name, ms - statistics.median(wall[name])) for name, _ in FORMATS))
    lines.append("slow wall / one-call wall: " + ", ".join("%s %.2f" % (name, ms / statistics.median(wall[name])) for name, _ in FORMATS))
    lines.append("the f32 result holds the words of the slow route: %s" % same)
    # the encode kernel alone, on the finished f32 atlas
    side = torch.cuda.Stream()
    r.setStream(side.cuda_stream)
    with torch.cuda.stream(side):
        d_in = torch.from_numpy(np.ascontiguousarray(last["f32"][1]).view(np.int32).copy()).to("cuda")
        d_out = torch.empty(size * size * 4, dtype=torch.int32, device="cuda")
    for name, bytes_per in FORMATS:
        us = []
        for rnd in range(ROUNDS + 1):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                ev0.record(side)
                for _ in range(REPS):
                    r.encodeAtlasDevice(d_in.data_ptr(), size, size, name, d_out.data_ptr(), size * size * bytes_per)
                ev1.record(side)
            side.synchronize()
            if rnd:                                # round 0 is the warm-up
                us.append(ev0.elapsed_time(ev1) * 1e3 / REPS)
        got = d_out.cpu().numpy().view(np.uint32)[:size * size * bytes_per // 4]
        agrees = np.array_equal(got, np.ascontiguousarray(last[name][1]).view(np.uint32).reshape(-1))
        what = "k_encode_atlas" if name != "f32" else "a device-to-device copy"
        lines.append("encode alone, format %-4s (%s)   %s per call (%d back to back per round); the words of the one call: %s"
                     % (name, what, fmt(us, "us"), REPS, agrees))
    r.setStream(None)
    r.destroy()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
