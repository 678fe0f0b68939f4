"""Rate of the reflection sampler (rt_sample_reflection_device, k_reflection_sample<PARALLAX>) beside the route that existed
before it, from one process.  No scene is needed.

Chains: N probes (1 and 8) of size 128, 6 levels, random radiance; N_QUERIES queries, roughness uniform in [0, 1], positions
inside each probe's box:
  coherent   directions in the order of a 2048 x 2048 octahedral raster: neighbouring lanes read neighbouring texels
  random     the same directions shuffled: every lane of a wave reads another part of the map, and another probe
  both kernel forms; queries/s, lookups/s at 8 texel loads per query, and GB/s at 16 B per lookup, to hold against
  tools/gather_peak.hip's figures in profiles/r03_gather_peak.txt.
  host route the route it replaces: the chains pulled back from the device (wall) and the rule - pack, the level pick, the seam
             fold, the bilinear gather, the mix - in numpy float32 on the host (wall); without parallax.  Its words are
             compared with the kernel's (rounding differs where numpy fuses nothing but orders alike: reported, not gated).
Device events for the kernel times; one warm-up pass; 5 rounds that alternate the cases, each round behind one launch that is
not recorded (the device idles for seconds while numpy runs); every figure is the median of the rounds with (min .. max)
beside it.  Nothing is gated on these numbers.  What to hold the first run against: DESIGN.md 4.1q.

usage: python tools/reflection_sample_time.py [--out profiles/reflection_sample_rate.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from webgpu_raytracer_amd import renderer as R  # noqa: E402
from timing_util import fmt  # noqa: E402

SIZE, LEVELS, RASTER, ROUNDS = 128, 6, 2048, 5
N_QUERIES = RASTER * RASTER
F = np.float32


def host_sample(chains, queries):
    """the rule without parallax in numpy float32: (n, 4) f32.  Weights of zero are multiplied, not skipped: finite chains."""
    q = queries.view(F).reshape(-1, 8)
    pr = queries["probe"].astype(np.int64)
    x, y, z = q[:, 4], q[:, 5], q[:, 6]
    s = F(1.0) / (np.abs(x) + np.abs(y) + np.abs(z))
    px, py = x * s, y * s
    ox = (F(1.0) - np.abs(py)) * np.where(px >= 0, F(1.0), F(-1.0))
    oy = (F(1.0) - np.abs(px)) * np.where(py >= 0, F(1.0), F(-1.0))
    qx, qy = np.where(z < 0, ox, px), np.where(z < 0, oy, py)
    r = np.minimum(np.where(q[:, 7] > 0, q[:, 7], F(0.0)), F(1.0))
    xl = r * F(LEVELS - 1)
    m0 = np.minimum(xl.astype(np.int64), LEVELS - 2)
    g = xl - m0.astype(F)
    off = R.reflection_level_offsets(SIZE, LEVELS)
    out = np.zeros((q.shape[0], 4), F)
    for lv, wl in ((m0, F(1.0) - g), (m0 + 1, g)):
        S = SIZE >> lv
        fS = S.astype(F)
        tap = []
        for c in (qx, qy):
            u = (c * F(0.5) + F(0.5)) * fS - F(0.5)
            u = np.minimum(np.where(u >= F(-0.5), u, F(-0.5)), fS - F(0.5))
            fl = np.floor(u)
            tap.append((fl.astype(np.int64), u - fl))
        (i0, fx), (j0, fy) = tap
        val = np.zeros((q.shape[0], 4), F)
        for a, b in ((0, 0), (1, 0), (0, 1), (1, 1)):
            i, j = i0 + a, j0 + b
            oi = (i < 0) | (i >= S)
            i, j = np.where(oi, np.where(i < 0, -1 - i, 2 * S - 1 - i), i), np.where(oi, S - 1 - j, j)
            oj = (j < 0) | (j >= S)
            j, i = np.where(oj, np.where(j < 0, -1 - j, 2 * S - 1 - j), j), np.where(oj, S - 1 - i, i)
            w = (fx if a else F(1.0) - fx) * (fy if b else F(1.0) - fy)
            val = val + w[:, None] * chains[pr, off[lv] + j * S + i]
        out = out + wl[:, None] * val
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    r = W.WebGPURenderer(0)                                           # nothing uploaded: the sampler needs no scene
    stream = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rng = np.random.default_rng(3)
    chain = int(R.reflection_level_offsets(SIZE, LEVELS)[-1])
    dirs = R.octa_directions(RASTER).reshape(-1, 3)
    shuffle = rng.permutation(N_QUERIES)
    rough = rng.uniform(0.0, 1.0, size=N_QUERIES)
    descs = {False: R.reflection_sample_desc(SIZE, LEVELS), True: R.reflection_sample_desc(SIZE, LEVELS, parallax=True)}
    d_out = torch.empty((N_QUERIES, 4), dtype=torch.float32, device="cuda")
    cases, state = [], {}
    for n_probes in (1, 8):
        host = rng.uniform(0.0, 4.0, size=(n_probes, chain, 4)).astype(F)
        centre = rng.uniform(-0.25, 0.25, size=(n_probes, 3))
        probes = np.zeros(n_probes, R.PROBE_DTYPE)
        probes["position"], probes["t_max"] = centre, 1e30
        boxes = np.zeros(n_probes, R.REFLECTION_BOX_DTYPE)
        boxes["lo"], boxes["hi"] = centre - 1.0, centre + 1.0
        # a probe per block of the raster, so that a coherent wave stays inside one chain
        pr = (np.arange(N_QUERIES) * n_probes // N_QUERIES).astype(np.uint32)
        pos = centre[pr] + rng.uniform(-0.9, 0.9, size=(N_QUERIES, 3))
        q = R.reflection_queries(pos, pr, dirs, rough)
        state[n_probes] = dict(host=host, q={"coherent": q, "random": q[shuffle]},
                               d_chains=torch.from_numpy(host).cuda(), d_probes=torch.from_numpy(probes.view(F).reshape(-1, 8)).cuda(),
                               d_boxes=torch.from_numpy(boxes.view(F).reshape(-1, 8)).cuda())
        for order in ("coherent", "random"):
            state[n_probes]["d_" + order] = torch.from_numpy(state[n_probes]["q"][order].view(F).reshape(-1, 8)).cuda()
            for parallax in (False, True):
                cases.append((n_probes, order, parallax))
    torch.cuda.synchronize()
    r.setStream(stream.cuda_stream)

    def timed(n_probes, order, parallax):
        s = state[n_probes]
        with torch.cuda.stream(stream):
            ev[0].record(stream)
            r.sampleReflectionDevice(descs[parallax], s["d_chains"].data_ptr(), n_probes, s["d_" + order].data_ptr(), N_QUERIES,
                                     d_out.data_ptr(), s["d_probes"].data_ptr(), s["d_boxes"].data_ptr())
            ev[1].record(stream)
        stream.synchronize()
        return ev[0].elapsed_time(ev[1])

    def host_route(n_probes, order):
        s = state[n_probes]
        t0 = time.perf_counter()
        pulled = s["d_chains"].cpu().numpy()
        pull = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        out = host_sample(pulled, s["q"][order])
        return out, pull, (time.perf_counter() - t0) * 1e3

    for c in cases:
        timed(*c)
    ms = {c: [] for c in cases}
    host_ms = {(1, "coherent"): ([], []), (8, "random"): ([], [])}
    worst = 0.0
    for _ in range(ROUNDS):
        timed(*cases[-1])                                             # not recorded: the device idled through the host route
        for c in cases:
            ms[c].append(timed(*c))
        for (n_probes, order), (pull, gather) in host_ms.items():
            timed(n_probes, order, False)
            got = d_out.cpu().numpy()
            out, a, b = host_route(n_probes, order)
            pull.append(a)
            gather.append(b)
            worst = max(worst, float(np.abs(out - got).max()))
    r.setStream(None)
    lines = ["reflection sampler: %d queries, chains of size %d, %d levels (%d texels, %d KiB per probe); lookups = 8 per query; "
             "GB/s = 1e-9 * 16 B * lookups / seconds" % (N_QUERIES, SIZE, LEVELS, chain, chain * 16 // 1024)]
    for c in cases:
        n_probes, order, parallax = c
        lines.append("  %d probe%s %-9s %-9s %s; %s; %s; gather %s" % (
            n_probes, " " if n_probes == 1 else "s", order, "parallax" if parallax else "plain", fmt(ms[c], "ms"),
            fmt([N_QUERIES / (v * 1e-3) * 1e-9 for v in ms[c]], "Gqueries/s"),
            fmt([8.0 * N_QUERIES / (v * 1e-3) * 1e-9 for v in ms[c]], "Glookups/s", 1),
            fmt([128.0 * N_QUERIES / (v * 1e-3) * 1e-9 for v in ms[c]], "GB/s", 0)))
    lines.append("host route (plain): the chains pulled back, the rule in numpy float32; largest |numpy - kernel| %.3g" % worst)
    for (n_probes, order), (pull, gather) in host_ms.items():
        lines.append("  %d probe%s %-9s pull %s; numpy %s" % (n_probes, " " if n_probes == 1 else "s", order, fmt(pull, "ms"),
                                                              fmt(gather, "ms", 0)))
    r.destroy()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
