"""Stream time of atlas denoising (rt_denoise_atlas_device: the index build and k_denoise_pass once per pass) on the atlas of
tools/atlas_bake_time.py with the guides of its own point pass, beside that bake's wall time and a numpy restatement of the
rule on the same atlas.

Scene instanced1000, 1024 entries as 32 x 32 rectangles of 32 x 32 texels in a 1024 x 1024 atlas, depth 4, spp 16 (the
entries, layout and seed of atlas_bake_time.py).  Atlas, points and texels go to torch tensors once; passes 1 and 3 at step 1:
  device   REPS denoise calls back to back on a side stream between two device events, each from the same input atlas into
           the same output; the figure is the elapsed time / REPS.  One warm-up, five rounds.
  host     denoiseAtlas on the host arrays: the same launches plus atlas, points and texels up and the atlas down (wall time,
           five rounds).
  numpy    the same rule on the host: one shifted, masked accumulation per tap, f32 in the order of the rule (wall time,
           once); its words are compared with the device's.
World units: the instances of instanced1000 are unit-sized, so plane_eps 0.02 and max_dist 0.5 as in the tests.
Nothing is gated on these numbers.

usage: python tools/denoise_time.py [--out profiles/denoise_rate.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from atlas_bake_time import CELL, DEPTH, SCENE, SEED, SIDE, SPP, fmt, merged_grid_uv  # noqa: E402

ROUNDS, REPS, PASSES = 5, 20, (1, 3)
PARAMS = dict(normal_cos=0.9, plane_eps=0.02, max_dist=0.5)
KW = (0.375, 0.25, 0.0625)


def numpy_pass(atlas, guide, P, N, step, normal_cos, plane_eps, max_dist):
    """one pass of the denoise rule of include/mi355rt.h: atlas (H, W, 4) f32, guide (H, W) bool, P and N (H, W, 3) f32"""
    f = np.float32
    H, W_ = guide.shape
    acc = np.zeros((H, W_, 4), f)
    wsum = np.zeros((H, W_), f)
    md2 = f(max_dist) * f(max_dist)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            h = f(KW[abs(dx)]) * f(KW[abs(dy)])
            oy, ox = dy * step, dx * step
            ys, ye = max(0, -oy), min(H, H - oy)      # texel rows whose tap row y + oy exists
            xs, xe = max(0, -ox), min(W_, W_ - ox)
            if ys >= ye or xs >= xe:
                continue
            here = (slice(ys, ye), slice(xs, xe))
            tap = (slice(ys + oy, ye + oy), slice(xs + ox, xe + ox))
            ok = guide[here] & guide[tap]
            if dx or dy:
                n, nq, d = N[here], N[tap], P[tap] - P[here]
                with np.errstate(invalid="ignore", over="ignore"):
                    ok = ok & ((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2] >= f(normal_cos))
                    ok &= np.abs((n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]) <= f(plane_eps)
                    ok &= (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= md2
            a, w = acc[here], wsum[here]
            a[ok] = a[ok] + h * atlas[tap][ok]
            w[ok] = w[ok] + h
    out = atlas.copy()
    out[guide] = acc[guide] / wsum[guide][:, None]
    return out


def numpy_denoise(atlas, points, texels, passes, step=1, **params):
    H, W_ = atlas.shape[:2]
    idx = np.full(H * W_, -1, np.int64)
    tex = np.asarray(texels, np.int64)
    j = np.flatnonzero(tex < H * W_)[::-1]
    idx[tex[j]] = j                                   # descending j: the lowest is assigned last and stays
    guide = (idx >= 0).reshape(H, W_)
    P = np.zeros((H * W_, 3), np.float32)
    N = np.zeros((H * W_, 3), np.float32)
    P[idx >= 0] = points[idx[idx >= 0], 0:3]
    N[idx >= 0] = points[idx[idx >= 0], 4:7]
    a = atlas
    for p in range(passes):
        a = numpy_pass(a, guide, P.reshape(H, W_, 3), N.reshape(H, W_, 3), step << p, **params)
    return a


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
    t0 = time.perf_counter()
    points, texels = r.bakeAtlasPoints(entries, size, size, atlas_uv=uv)
    points_ms = (time.perf_counter() - t0) * 1e3
    assert len(texels) == covered
    atlas = np.ascontiguousarray(baked).view(np.float32).reshape(size, size, 4)
    lines = ["atlas denoise, %s: the %d x %d atlas of %d entries of %d x %d texels (depth %d, spp %d); %d of %d texels guided"
             % (SCENE, size, size, n, CELL, CELL, DEPTH, SPP, covered, size * size),
             "normal_cos %(normal_cos)g, plane_eps %(plane_eps)g, max_dist %(max_dist)g, step 1" % PARAMS,
             "the bake itself (one bakeAtlasIrradiance)        wall %s" % fmt(bake_ms),
             "the extra point pass of denoise= (bakeAtlasPoints, host arrays)   wall %.2f ms (once)" % points_ms]
    side = torch.cuda.Stream()
    r.setStream(side.cuda_stream)
    with torch.cuda.stream(side):
        d_in = torch.from_numpy(atlas.view(np.int32).copy()).to("cuda")
        d_out = torch.empty_like(d_in)
        d_points = torch.from_numpy(points.view(np.int32).copy()).to("cuda")
        d_texels = torch.from_numpy(texels.view(np.int32).copy()).to("cuda")
    for passes in PASSES:
        device_us = []
        for rnd in range(ROUNDS + 1):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                ev0.record(side)
                for _ in range(REPS):
                    r.denoiseAtlasDevice(d_in.data_ptr(), d_points.data_ptr(), d_texels.data_ptr(), covered, d_out.data_ptr(),
                                         size, size, passes=passes, **PARAMS)
                ev1.record(side)
            side.synchronize()
            if rnd:                                # round 0 is the warm-up
                device_us.append(ev0.elapsed_time(ev1) * 1e3 / REPS)
        host_ms = []
        r.denoiseAtlas(atlas, points, texels, passes=passes, **PARAMS)
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            r.denoiseAtlas(atlas, points, texels, passes=passes, **PARAMS)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        want = numpy_denoise(atlas, points, texels, passes, **PARAMS)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        got = d_out.cpu().numpy().view(np.uint32).reshape(size, size, 4)
        same = np.array_equal(got, want.view(np.uint32))
        changed = int((got != atlas.view(np.uint32)).any(axis=2).sum())
        lines += ["passes %d: %d texels changed" % (passes, changed),
                  "  device, index build + %d pass launches          %s per call (%d back to back per round)"
                  % (passes, fmt(device_us, "us"), REPS),
                  "  host entry (denoiseAtlas: atlas, points, texels up, the launches, atlas down)   wall %s" % fmt(host_ms),
                  "  numpy restatement on the host                 wall %.1f ms (once); same words as the device: %s"
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
