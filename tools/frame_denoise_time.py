"""Stream time of the frame denoiser (rt_denoise_frame_device: k_frame_prepare, k_frame_pass_lds / k_frame_pass_direct once
per pass, k_frame_finish) on cornell at 1920 x 1080 after one compute(), beside the frame it filters and the numpy route it
replaces.

Cornell, depth 8, 1 spp, {step 1, passes 5, DEMODULATE, normal_cos 0.9, plane_eps 0.02, sigma_lum 4}.  One warm-up and five
rounds; in every round the forced LDS form ({step 1, passes 3}: spacings 1, 2, 4) and the forced direct form ({step 1, passes
5}: spacings 1 .. 16) alternate, each after the cache of the prepare stage has been dropped (rt_bind_accum(NULL)), and the
times are those of the library's own device events around every launch (rt_frame_denoise_stats).  Then, in the same process:
  frame    compute(f); present() of the live loop, plain and with setPresentDenoise, alternated: device events around 20
           frames, five rounds each
  host     denoiseFrame (the launches and the image down; wall, five rounds)
  numpy    what a caller did before: the accumulator, the three G-buffer planes and the uniform block over PCIe (wall), the
           prepare stage and ONE pass at spacing 1 in numpy, f32 in the order of the rule with one masked accumulation per tap
           (wall, once; sigma_lum 0, numpy has no rt_exp); its words are compared with the device's {step 1, passes 1, sigma_lum 0}
Every median comes with its spread.  Nothing is gated on these numbers.

usage: python tools/frame_denoise_time.py [--out profiles/frame_denoise_rate.txt] [--width 1920 --height 1080]"""
import argparse
import functools
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from webgpu_raytracer_amd import renderer as R  # noqa: E402
import timing_util  # noqa: E402

ROUNDS, FRAMES, DEPTH = 5, 20, 8
PARAMS = dict(plane_eps=0.02, normal_cos=0.9, sigma_lum=4.0)
KW = (0.375, 0.25, 0.0625)
F = np.float32
fmt = functools.partial(timing_util.fmt, median=statistics.median_high)   # of 2 x ROUNDS values: the upper one


def numpy_prepare(accum, alb, nid, depth, u):
    """the prepare stage of the frame denoise rule, DEMODULATE on: -> col (H, W, 4), P, N (H, W, 3), inst (H, W) u32, surface (H, W)
    bool, mod (H, W, 4), all f32 in the order of the rule"""
    H, Wd = depth.shape
    with np.errstate(all="ignore"):
        rad = np.where((accum[..., 3] <= 0)[..., None], F(0), accum[..., 0:3] / accum[..., 3:4]).astype(F)
        word = np.ascontiguousarray(alb).view(np.uint32).reshape(H, Wd)
        surface = (word >> 24) != 0
        m = np.maximum(alb[..., 0:3].astype(F) / F(255.0), F(0.00392156886))
        m[~surface] = 1.0
        q = (rad / m).astype(F)
        lum = (F(0.2126) * q[..., 0] + F(0.7152) * q[..., 1]) + F(0.0722) * q[..., 2]
        m1 = np.zeros((H, Wd), F)
        m2 = np.zeros((H, Wd), F)
        ys, xs = np.mgrid[0:H, 0:Wd]
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                l = lum[np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, Wd - 1)]
                m1 = m1 + l
                m2 = m2 + l * l
        mean = m1 / F(9.0)
        var = np.maximum(m2 / F(9.0) - mean * mean, F(0))
        f = u.view(F)
        eye, ll, hor, ver = f[0:3], f[4:7], f[8:11], f[12:15]
        center = ll + hor * F(0.5) + ver * F(0.5)
        e = center - eye
        focal = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        ox, oy = nid[..., 0], nid[..., 1]
        n = np.stack([ox, oy, F(1.0) - np.abs(ox) - np.abs(oy)], axis=-1).astype(F)
        t = np.clip(-n[..., 2], F(0), F(1))
        n[..., 0] += np.where(n[..., 0] >= 0, -t, t)
        n[..., 1] += np.where(n[..., 1] >= 0, -t, t)
        inv = F(1.0) / np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
        N = n * inv[..., None]
        uu = ((xs.astype(F) + F(0.5) + f[56] * F(Wd)) / F(Wd)).astype(F)
        vv = (F(1.0) - (ys.astype(F) + F(0.5) + f[57] * F(H)) / F(H)).astype(F)
        d = ((ll + uu[..., None] * hor) + vv[..., None] * ver) - eye
        ca = F(10000.0) / (F(10000.0) - F(0.001))
        cb = (F(10000.0) * F(0.001)) / (F(10000.0) - F(0.001))
        th = (cb / (ca - depth)) / focal
        P = (eye + d * th[..., None]).astype(F)
    col = np.concatenate([q, var[..., None]], axis=-1).astype(F)
    mod = np.concatenate([m, (accum[..., 3:4] > 0).astype(F)], axis=-1).astype(F)
    return col, P, N.astype(F), nid[..., 3].view(np.uint32), surface, mod


def numpy_pass(col, P, N, surface, step, normal_cos, plane_eps):
    """one pass, sigma_lum <= 0, SAME_INSTANCE off: one shifted, masked accumulation per tap"""
    H, Wd = surface.shape
    acc = np.zeros((H, Wd, 4), F)
    wsum = np.zeros((H, Wd), F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            h = F(KW[abs(dx)]) * F(KW[abs(dy)])
            oy, ox = dy * step, dx * step
            ys, ye = max(0, -oy), min(H, H - oy)
            xs, xe = max(0, -ox), min(Wd, Wd - ox)
            if ys >= ye or xs >= xe:
                continue
            here = (slice(ys, ye), slice(xs, xe))
            tap = (slice(ys + oy, ye + oy), slice(xs + ox, xe + ox))
            ok = surface[here] & surface[tap]
            if dx or dy:
                n, nq, e = N[here], N[tap], P[tap] - P[here]
                with np.errstate(invalid="ignore", over="ignore"):
                    ok = ok & ((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2] >= F(normal_cos))
                    ok &= np.abs((n[..., 0] * e[..., 0] + n[..., 1] * e[..., 1]) + n[..., 2] * e[..., 2]) <= F(plane_eps)
            a, w = acc[here], wsum[here]
            c = col[tap][ok]
            with np.errstate(all="ignore"):
                a[ok] = a[ok] + np.concatenate([h * c[:, 0:3], (h * h) * c[:, 3:4]], axis=1)
                w[ok] = w[ok] + h
    out = col.copy()
    with np.errstate(all="ignore"):
        out[surface, 0:3] = acc[surface, 0:3] / wsum[surface][:, None]
        out[surface, 3] = acc[surface, 3] / (wsum[surface] * wsum[surface])
    return out


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
    r.compute(1)
    r.sync()
    npx = width * height
    full = R.frame_denoise_desc(5, 1, **PARAMS)
    staged = R.frame_denoise_desc(3, 1, **PARAMS)
    t = torch.zeros((height, width, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    times = {}          # (stage, form) -> [us per round]

    def one(form, desc):
        r.setFrameDenoiseForm(form)
        r.bindAccum(None)                    # drops the prepare stage's cache: every call prepares
        r.denoiseFrameDevice(t, desc)
        s = r.frameDenoiseStats()
        assert not s["cache_hit"] and s["forms"] == [form] * len(s["forms"])
        return s

    for rnd in range(ROUNDS + 1):            # round 0 is the warm-up
        for form, desc in (("lds", staged), ("direct", full)):
            s = one(form, desc)
            if not rnd:
                continue
            times.setdefault(("prepare", ""), []).append(s["prepare_ms"] * 1e3)
            times.setdefault(("finish", ""), []).append(s["finish_ms"] * 1e3)
            for p, ms in enumerate(s["pass_ms"]):
                times.setdefault((1 << p, form), []).append(ms * 1e3)
    lines = ["frame denoise, cornell %d x %d after one compute() (depth %d, 1 spp): {step 1, passes 5, DEMODULATE, normal_cos "
             "%g, plane_eps %g, sigma_lum %g}" % (width, height, DEPTH, PARAMS["normal_cos"], PARAMS["plane_eps"], PARAMS["sigma_lum"]),
             "the library's own device events around every launch; one warm-up, %d rounds, the two forms alternated" % ROUNDS,
             "k_frame_prepare (reads 24 B of G-buffer and 9 x 20 B of neighbourhood, writes 64 B per pixel)   %s"
             % fmt(times[("prepare", "")], "us", 1),
             "k_frame_finish  (48 B per pixel)                                                                %s"
             % fmt(times[("finish", "")], "us", 1)]
    verdict = []
    for step in (1, 2, 4, 8, 16):
        for form in ("lds", "direct"):
            if (step, form) in times:
                v = times[(step, form)]
                med = sorted(v)[len(v) // 2]
                lines.append("pass at spacing %2d, %-6s form   %s   = %.0f GB/s of (48 B in + 16 B out) per pixel"
                             % (step, form, fmt(v, "us", 1), npx * 64 / med / 1e3))
        if (step, "lds") in times:
            l, d = (sorted(times[(step, f)])[ROUNDS // 2] for f in ("lds", "direct"))
            verdict.append("%d: %s" % (step, "lds" if l < d else "direct"))
    lines.append("faster form per spacing (medians): " + ", ".join(verdict))

    # the frame the filter serves: compute(f); present(), plain and filtered, alternated
    side = torch.cuda.Stream()
    r.setStream(side.cuda_stream)
    r.setFrameDenoiseForm("auto")
    frame_ms = {"plain": [], "filtered": []}
    f = 2
    for rnd in range(ROUNDS + 1):
        for name in ("plain", "filtered"):
            r.setPresentDenoise(full if name == "filtered" else None)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                ev0.record(side)
                for _ in range(FRAMES):
                    r.compute(f)
                    r.present()
                    f += 1
                ev1.record(side)
            side.synchronize()
            if rnd:
                frame_ms[name].append(ev0.elapsed_time(ev1) / FRAMES)
    r.setPresentDenoise(None)
    r.setStream(None)
    lines += ["the 1-spp frame, compute(f); present(), device events around %d frames:" % FRAMES,
              "  plain                                   %s per frame" % fmt(frame_ms["plain"], "ms"),
              "  with setPresentDenoise (auto forms)     %s per frame" % fmt(frame_ms["filtered"], "ms")]

    # the host entry, and the numpy route
    r.compute(f)
    host_ms = []
    r.denoiseFrame(full)
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        r.denoiseFrame(full)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    lines.append("host entry (denoiseFrame: the launches, the image down)   wall %s" % fmt(host_ms, "ms"))
    t0 = time.perf_counter()
    accum = r.readAccum()
    alb, nid, depth = r.readGBuffer()
    u = r.readUniforms()
    read_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    col, P, N, inst, surface, mod = numpy_prepare(accum, alb, nid, depth, u)
    prep_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    out = numpy_pass(col, P, N, surface, 1, PARAMS["normal_cos"], PARAMS["plane_eps"])
    pass_ms = (time.perf_counter() - t0) * 1e3
    want = np.concatenate([out[..., 0:3] * mod[..., 0:3], mod[..., 3:4]], axis=-1).astype(F)
    got = r.denoiseFrame(R.frame_denoise_desc(1, 1, **dict(PARAMS, sigma_lum=0.0)))
    diff = int((got.view(np.uint32) != want.view(np.uint32)).any(axis=2).sum())
    lines += ["the numpy route: read-backs (accumulator, three planes, uniforms) wall %.1f ms; prepare in numpy wall %.0f ms; ONE "
              "pass at spacing 1 in numpy wall %.0f ms (once each)" % (read_ms, prep_ms, pass_ms),
              "  its words against the device's {step 1, passes 1, sigma_lum 0}: %d of %d pixels differ" % (diff, npx)]
    r.destroy()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
