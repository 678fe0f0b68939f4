"""Stream time of the temporal stage of the frame denoiser (rt_set_frame_temporal: k_frame_temporal, between k_frame_prepare and
the first pass) on cornell at 1920 x 1080 with the camera moving between frames.

Cornell, depth 8, 1 spp, the filter {step 1, passes 1, DEMODULATE, normal_cos 0.9, plane_eps 0.02, sigma_lum 4} behind the
stage {max_history 32, var_history 4, normal_cos 0.9, plane_eps 0.02}.  One warm-up and five rounds; a round is one frame: the
camera translated by a third of a pixel of the image plane sideways and a sixth upwards, the accumulation reset, compute(f),
one denoiseFrameDevice.  The times are those of the library's own device events around the launches (rt_frame_denoise_stats):
the stage, and beside it the prepare stage it follows and the pass it feeds.  After the rounds the history is read back once:
how many pixels carry how many frames.  Every median comes with its spread.  Nothing is gated on these numbers.

usage: python tools/frame_temporal_time.py [--out profiles/frame_temporal_rate.txt] [--width 1920 --height 1080]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from webgpu_raytracer_amd import renderer as R  # noqa: E402
import timing_util  # noqa: E402

ROUNDS, DEPTH = 5, 8
STEP = (1.0 / 3.0, 1.0 / 6.0)    # pixels of the image plane per frame
FILTER = dict(plane_eps=0.02, normal_cos=0.9, sigma_lum=4.0)
STAGE = dict(max_history=32, var_history=4, plane_eps=0.02, normal_cos=0.9)
BYTES = 16 + 32 + 4 * (32 + 16 + 8) + 16 + 16 + 8   # per pixel: its own texels, four taps, the three stores


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    width, height = args.width, args.height
    b = W.WorldBridge()
    b.loadScene("cornell")
    r = W.WebGPURenderer(0)
    r.buildPipeline(DEPTH, 1)
    W.upload_scene(r, b, width, height)
    base = np.array(b.cameraData, dtype=np.float32).reshape(6, 4)
    r.setFrameTemporal(R.frame_temporal_desc(**STAGE))
    desc = R.frame_denoise_desc(1, 1, **FILTER)
    t = torch.zeros((height, width, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    times = {"prepare": [], "temporal": [], "pass": []}
    for rnd in range(ROUNDS + 1):            # round 0 is the warm-up, and the first frame: it has no history to gather
        cam = base.copy()
        shift = base[2, :3] * np.float32(rnd * STEP[0] / width) + base[3, :3] * np.float32(rnd * STEP[1] / height)
        cam[0, :3] += shift
        cam[1, :3] += shift
        r.updateSceneUniforms(cam.reshape(-1), 0, b.lightCount)
        r.resetAccumulation()
        r.compute(rnd + 1)
        r.denoiseFrameDevice(t, desc)
        s = r.frameDenoiseStats()
        assert s["temporal"] == "ran" and not s["cache_hit"]
        if rnd:
            times["prepare"].append(s["prepare_ms"] * 1e3)
            times["temporal"].append(s["temporal_ms"] * 1e3)
            times["pass"].append(s["pass_ms"][0] * 1e3)
    col, _, frames = r.readFrameHistory()
    assert frames == ROUNDS + 1
    n = col[..., 3].astype(np.int64)
    counts = np.bincount(n.reshape(-1), minlength=ROUNDS + 2)
    npx = width * height
    med = sorted(times["temporal"])[ROUNDS // 2]
    lines = ["frame temporal, cornell %d x %d (depth %d, 1 spp), the camera moved by (%.3f, %.3f) pixels of the image plane per "
             "frame: {max_history %d, var_history %d, normal_cos %g, plane_eps %g}"
             % (width, height, DEPTH, STEP[0], STEP[1], STAGE["max_history"], STAGE["var_history"], STAGE["normal_cos"],
                STAGE["plane_eps"]),
             "the library's own device events around every launch; one warm-up (the first frame), %d rounds of one frame each" % ROUNDS,
             "k_frame_temporal (19 wave-level loads, %d B per pixel)              %s   = %.0f GB/s of %d B per pixel"
             % (BYTES, timing_util.fmt(times["temporal"], "us", 1), npx * BYTES / med / 1e3, BYTES),
             "k_frame_prepare ahead of it                                          %s" % timing_util.fmt(times["prepare"], "us", 1),
             "the pass at spacing 1 behind it (auto form)                          %s" % timing_util.fmt(times["pass"], "us", 1),
             "history after %d frames: " % frames + ", ".join("n = %d: %d pixels" % (k, c) for k, c in enumerate(counts) if c)]
    r.destroy()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
