"""Stream time of frame motion (RT_FRAME_TEMPORAL_MOTION: k_frame_motion, k_frame_temporal_motion, the snapshot) in the loop it
exists for: the animated 262 k-triangle glTF of the live-loop benchmark at 1920 x 1080 and 1 spp, the world updated on the
device every frame.

The filter {step 1, passes 1, DEMODULATE, normal_cos 0.9, plane_eps 0.02, sigma_lum 4} behind the stage {max_history 32,
var_history 4, normal_cos 0.8, plane_eps 0.02}, once with the flag and once without.  One warm-up and five rounds; a round is
one frame: update(t), the camera and accumulation reset of sync_world, compute(f), one denoiseFrameDevice.  The kernels' times
are those of the library's own device events around the launches (rt_frame_denoise_stats).  The snapshot - a device copy of
the vertices and the scatter of the transforms - has no event pair of its own: the context runs on the caller's stream here,
events of the caller's bracket the whole call, and what the call takes beyond the sum of its reported stages is reported with
the flag and without it; the difference is the snapshot.  Every median comes with its spread.  Nothing is gated on these numbers.

usage: python tools/frame_motion_time.py [--out profiles/frame_motion_rate.txt] [--nu 512 --nv 256]"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
import webgpu_raytracer_amd as W  # noqa: E402
from webgpu_raytracer_amd import renderer as R  # noqa: E402
import test_gltf  # noqa: E402
import timing_util  # noqa: E402

ROUNDS, DEPTH = 5, 8
WIDTH, HEIGHT = 1920, 1080
FILTER = dict(plane_eps=0.02, normal_cos=0.9, sigma_lum=4.0)
STAGE = dict(max_history=32, var_history=4, plane_eps=0.02, normal_cos=0.8)
BYTES_MOTION = 16 + 32 + 16 + 4 + 64 + 64 + 6 * 16 + 32 + 4
BYTES_TEMPORAL = 16 + 32 + 4 * (32 + 16 + 8) + 16 + 16 + 8


def run(glb, motion):
    import torch
    r = W.WebGPURenderer(0)
    r.buildPipeline(DEPTH, 1)
    stream = torch.cuda.Stream()             # a stream of the caller's, not the default one: its events bracket the library's work
    r.setStream(stream.cuda_stream)
    b = W.WorldBridge(zero_copy=True)
    b.setDeviceUpdater(r)
    b.loadScene("viewer", glbData=glb)
    W.upload_scene(r, b, WIDTH, HEIGHT)
    desc = R.frame_denoise_desc(1, 1, **FILTER)
    t = torch.zeros((HEIGHT, WIDTH, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    times = {k: [] for k in ("prepare", "motion", "temporal", "pass", "rest")}
    for rnd in range(ROUNDS + 4):            # three updates in which the device path learns the trees' depths, one warm-up
        b.update((rnd + 1) / 60)
        assert b.deviceResident, b.deviceWarning
        W.sync_world(r, b, WIDTH, HEIGHT)
        if rnd == 0:
            r.setFrameTemporal(R.frame_temporal_desc(motion=motion, **STAGE))
        r.compute(rnd + 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r.denoiseFrameDevice(t, desc)
        e1.record(stream)
        e1.synchronize()
        s = r.frameDenoiseStats()
        assert s["temporal"] == "ran" and s["motion"] is motion and not s["cache_hit"]
        if rnd >= 4:
            stages = s["prepare_ms"] + s["motion_ms"] + s["temporal_ms"] + s["pass_ms"][0] + s["finish_ms"]
            times["prepare"].append(s["prepare_ms"] * 1e3)
            times["motion"].append(s["motion_ms"] * 1e3)
            times["temporal"].append(s["temporal_ms"] * 1e3)
            times["pass"].append(s["pass_ms"][0] * 1e3)
            times["rest"].append((e0.elapsed_time(e1) - stages) * 1e3)
    col, _, frames = r.readFrameHistory()
    n = np.bincount(col[..., 3].astype(np.int64).reshape(-1))
    status = None
    if motion:
        status = np.bincount(np.ascontiguousarray(r.readFrameMotion()[..., 3]).view(np.uint32).reshape(-1), minlength=4)
    verts = len(r.worldRead("vertices")) // 4
    r.setStream(None)
    r.destroy()
    return times, n, status, frames, verts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--nu", type=int, default=512)
    ap.add_argument("--nv", type=int, default=256)
    args = ap.parse_args()
    glb, n_tris = test_gltf.big_skinned_glb(W, args.nu, args.nv)
    on, n_on, status, frames, verts = run(glb, True)
    off, n_off, _, _, _ = run(glb, False)
    npx = WIDTH * HEIGHT
    f = lambda v: timing_util.fmt(v, "us", 1)
    med = lambda v: sorted(v)[len(v) // 2]
    lines = ["frame motion, %d triangles and %d vertices skinned and rebuilt on the device every frame, %d x %d (depth %d, 1 spp): "
             "{max_history %d, var_history %d, normal_cos %g, plane_eps %g}"
             % (n_tris, verts, WIDTH, HEIGHT, DEPTH, STAGE["max_history"], STAGE["var_history"], STAGE["normal_cos"], STAGE["plane_eps"]),
             "the library's own device events around every launch; one warm-up, %d rounds of one frame each" % ROUNDS,
             "k_frame_motion (18 wave-level loads, %d B per pixel)                  %s   = %.0f GB/s of %d B per pixel"
             % (BYTES_MOTION, f(on["motion"]), npx * BYTES_MOTION / med(on["motion"]) / 1e3, BYTES_MOTION),
             "k_frame_temporal_motion (25 wave-level loads, %d B per pixel)        %s" % (BYTES_TEMPORAL + 32 + 16, f(on["temporal"])),
             "k_frame_temporal, the flag clear (19 wave-level loads, %d B)         %s" % (BYTES_TEMPORAL, f(off["temporal"])),
             "k_frame_prepare ahead of them                                         %s with the flag, %s without" % (f(on["prepare"]), f(off["prepare"])),
             "the call beyond its reported stages (caller's events), with the flag  %s" % f(on["rest"]),
             "the same without the flag                                             %s" % f(off["rest"]),
             "the snapshot (%d B of vertices copied, one transform scattered), by difference of the medians: %.1f us"
             % (verts * 16, med(on["rest"]) - med(off["rest"])),
             "carry after %d frames: %d background, %d untracked, %d unmoved, %d moved" % ((frames,) + tuple(int(v) for v in status[:4])),
             "history with the flag: " + ", ".join("n = %d: %d pixels" % (k, c) for k, c in enumerate(n_on) if c),
             "history without it:    " + ", ".join("n = %d: %d pixels" % (k, c) for k, c in enumerate(n_off) if c)]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
