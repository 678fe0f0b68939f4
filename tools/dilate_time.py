"""Stream time of atlas dilation (rt_dilate_atlas_device: k_dilate_mask, k_dilate_source, k_dilate_apply) on the atlas of
tools/atlas_bake_time.py, beside that bake's own wall time and a numpy nearest-source fill of the same atlas.

Scene instanced1000, 1024 entries as 32 x 32 rectangles of 32 x 32 texels in a 1024 x 1024 atlas, depth 4, spp 16 (the
entries, layout and seed of atlas_bake_time.py).  The baked atlas goes to a torch tensor once; radius 4 and 16:
  device   per round the atlas is restored from a pristine copy, then REPS dilations in place run back to back on a side
           stream between two device events; the figure is the elapsed time / REPS.  A second dilation finds the same
           coverage and the same sources (filled texels stay uncovered), so every repetition does the work of the first.  No
           source map or count is asked for: the three kernels and nothing else.  One warm-up, five rounds.
  host     dilateAtlas on the host array: the same three kernels plus the atlas up and down (wall time, five rounds).
  numpy    the same rule on the host: the offsets of the disc in ascending (d2, dy, dx), each a shifted copy into the texels
           still open (wall time, once); its source map is compared with the device's.
Nothing is gated on these numbers.

usage: python tools/dilate_time.py [--out profiles/dilate_rate.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from atlas_bake_time import CELL, DEPTH, SCENE, SEED, SIDE, SPP, fmt, merged_grid_uv  # noqa: E402

ROUNDS, REPS, RADII = 5, 20, (4, 16)
NONE = 0xffffffff


def numpy_fill(atlas, radius):
    """(dilated (H, W, 4) f32, source map (H, W) u32) by the dilation rule of include/mi355rt.h"""
    H, W_ = atlas.shape[:2]
    with np.errstate(invalid="ignore"):
        covered = atlas[..., 3] >= 0
    own = np.arange(H * W_, dtype=np.uint32).reshape(H, W_)
    src = np.where(covered, own, np.uint32(NONE))
    still = ~covered
    offsets = sorted((dx * dx + dy * dy, dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)
                     if 0 < dx * dx + dy * dy <= radius * radius)
    for _, dy, dx in offsets:
        ys, ye = max(0, -dy), min(H, H - dy)      # texel rows whose source row y + dy exists
        xs, xe = max(0, -dx), min(W_, W_ - dx)
        take = still[ys:ye, xs:xe] & covered[ys + dy:ye + dy, xs + dx:xe + dx]
        src[ys:ye, xs:xe][take] = own[ys + dy:ye + dy, xs + dx:xe + dx][take]
        still[ys:ye, xs:xe][take] = False
    out = atlas.view(np.uint32).copy()
    filled = (src != NONE) & (src != own)
    out[filled, 0:3] = atlas.view(np.uint32).reshape(-1, 4)[src[filled], 0:3]
    out[filled, 3] = 0xc0000000
    return out.view(np.float32), src


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

    def bake():
        t0 = time.perf_counter()
        atlas, covered, _ = r.bakeAtlasIrradiance(entries, size, size, DEPTH, SPP, SEED, atlas_uv=uv, stats=True)
        return (time.perf_counter() - t0) * 1e3, atlas, covered

    bake()
    bake_ms = []
    for _ in range(ROUNDS):
        ms, baked, covered = bake()
        bake_ms.append(ms)
    atlas = np.ascontiguousarray(baked).view(np.float32).reshape(size, size, 4)
    lines = ["atlas dilation, %s: the %d x %d atlas of %d entries of %d x %d texels (depth %d, spp %d); %d of %d texels covered"
             % (SCENE, size, size, n, CELL, CELL, DEPTH, SPP, covered, size * size),
             "the bake itself (one bakeAtlasIrradiance)        wall %s" % fmt(bake_ms)]
    side = torch.cuda.Stream()
    r.setStream(side.cuda_stream)
    with torch.cuda.stream(side):
        pristine = torch.from_numpy(atlas.view(np.int32).copy()).to("cuda")
        work = torch.empty_like(pristine)
        d_src = torch.zeros(size * size, dtype=torch.int32, device="cuda")
        d_filled = torch.zeros(4, dtype=torch.int32, device="cuda")
    for radius in RADII:
        device_us = []
        for rnd in range(ROUNDS + 1):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                work.copy_(pristine)
                ev0.record(side)
                for _ in range(REPS):
                    r.dilateAtlasDevice(work.data_ptr(), size, size, radius)
                ev1.record(side)
            side.synchronize()
            if rnd:                                # round 0 is the warm-up
                device_us.append(ev0.elapsed_time(ev1) * 1e3 / REPS)
        with torch.cuda.stream(side):
            work.copy_(pristine)
            r.dilateAtlasDevice(work.data_ptr(), size, size, radius, src_ptr=d_src.data_ptr(), filled_ptr=d_filled.data_ptr())
        side.synchronize()
        host_ms = []
        r.dilateAtlas(atlas, radius)
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            r.dilateAtlas(atlas, radius)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        want, want_src = numpy_fill(atlas, radius)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        same = (np.array_equal(d_src.cpu().numpy().view(np.uint32).reshape(size, size), want_src)
                and np.array_equal(work.cpu().numpy().view(np.uint32), want.view(np.uint32)))
        lines += ["radius %2d: %d texels filled" % (radius, int(d_filled[0])),
                  "  device, mask + source + apply in place        %s per dilation (%d back to back per round)"
                  % (fmt(device_us, "us"), REPS),
                  "  host entry (dilateAtlas: atlas up, three kernels, atlas down)   wall %s" % fmt(host_ms),
                  "  numpy nearest-source fill on the host         wall %.1f ms (once); same words as the device: %s"
                  % (numpy_ms, same)]
    r.setStream(None)
    r.destroy()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
