#!/usr/bin/env python3
"""Time the two copies of a gather on ONE GPU: the library's own rt_pack_stripes + rt_unpack_stripes (k_stripes.hip.h)
against the index_select + index_copy_ pair that distributed.ShardedImage issues, on the same shapes.

For world = 8, stripe 8 at 1920 x 1080 and 3840 x 2160, as rank 0 with all eight receive blocks resident (the exchange
itself is not timed here: it needs more than one GPU).  Both variants run on one torch side stream (the renderer is pointed
at it with rt_set_stream), each repetition is bracketed by device events, the two variants alternate inside one process,
and the whole series is repeated in rounds: the spread of the round medians is the run-to-run noise a difference has to
beat.  Before timing, the native result is checked bit for bit against the torch result on the same random data.

  python tools/gather_time.py [--reps 200] [--rounds 5] [--warmup 20] > profiles/native_gather_time.txt
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

COPY_PEAK = 6.29e12   # measured float4 copy rate of the MI355X, bytes moved per second (read + write)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="repetitions per variant per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--stripe", type=int, default=8)
    args = ap.parse_args()

    import torch
    import webgpu_raytracer_amd as pkg
    from webgpu_raytracer_amd.distributed import ShardedImage

    pkg._build.build_rt()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    world, stripe = args.world, args.stripe
    print("gather copies on one GPU: world %d, stripe %d, rank 0; %d rounds x %d alternated repetitions, %d warm-up"
          % (world, stripe, args.rounds, args.reps, args.warmup))
    ok = True
    for w, h in ((1920, 1080), (3840, 2160)):
        r = pkg.WebGPURenderer(0)
        r.updateScreenSize(w, h)
        r.distInit(0, world, stripe)
        r.setStream(stream.cuda_stream)
        spec = ShardedImage.__new__(ShardedImage)    # only its row arithmetic is used
        spec.stripe_rows, spec.world = stripe, world
        mr = spec.max_rows(h)
        own = spec.rows_of(0, h)
        assert r.distBlockBytes() == mr * w * 16
        rng = np.random.default_rng(w)
        accum = rng.random((h, w, 4), dtype=np.float32)
        blocks = rng.random((world, mr, w, 4), dtype=np.float32)
        r.writeAccum(accum)
        for k in range(world):
            r.writeBlock(k, blocks[k])
        with torch.cuda.stream(stream):
            # the tensors of ShardedImage.bind() / _plan() for rank 0
            t_stripe = torch.from_numpy(accum).to(dev)
            t_send = torch.zeros((mr, w, 4), dtype=torch.float32, device=dev)
            t_recv = torch.from_numpy(blocks).to(dev)
            t_disp = torch.zeros((max(h, world * mr), w, 4), dtype=torch.float32, device=dev)
            t_own = torch.from_numpy(own).to(dev)
            dst, scratch = [], h
            for k in range(world):
                rk = spec.rows_of(k, h)
                dst += list(rk) + list(range(scratch, scratch + mr - len(rk)))
                scratch += mr - len(rk)
            t_dst = torch.tensor(dst, dtype=torch.int64, device=dev)

        def native():
            r.packStripes()
            r.unpackStripes()

        def torch_pair():
            with torch.cuda.stream(stream):
                torch.index_select(t_stripe, 0, t_own, out=t_send[:len(own)])
                t_disp.index_copy_(0, t_dst, t_recv.view(-1, w, 4))

        # same data, same result: bit for bit
        native()
        torch_pair()
        stream.synchronize()
        same = (np.array_equal(r.readDisplay().view(np.uint32), t_disp[:h].cpu().numpy().view(np.uint32)) and
                np.array_equal(r.readBlock()[:len(own)].view(np.uint32), t_send[:len(own)].cpu().numpy().view(np.uint32)))
        for _ in range(args.warmup):
            native()
            torch_pair()
        stream.synchronize()

        ms = {"native": [], "torch": []}
        for _ in range(args.rounds):
            ev = {"native": [], "torch": []}
            for _ in range(args.reps):
                for name, fn in (("native", native), ("torch", torch_pair)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    ev[name].append((e0, e1))
            stream.synchronize()
            for name in ms:
                ms[name].append(np.array([a.elapsed_time(b) for a, b in ev[name]]))

        img = h * w * 16
        moved = {"native": 2 * len(own) * w * 16 + 2 * img,                 # pack: own rows in + out; unpack: the image in + out
                 "torch": 2 * len(own) * w * 16 + 2 * world * mr * w * 16}   # ... and the padding rows of every block as well
        print("\n%d x %d: block %d rows (%.2f MB), rank 0 owns %d rows; results identical: %s"
              % (w, h, mr, mr * w * 16 / 1e6, len(own), "yes" if same else "NO"))
        stat = {}
        for name in ("native", "torch"):
            allv = np.concatenate(ms[name])
            rmed = np.array([np.median(x) for x in ms[name]])
            stat[name] = (float(np.median(allv)), float(rmed.max() - rmed.min()))
            print("  %-6s pair: median %.4f ms   p10 %.4f   p90 %.4f   round medians %s (range %.4f)   %.1f MB moved, %.0f GB/s"
                  % (name, np.median(allv), np.percentile(allv, 10), np.percentile(allv, 90),
                     " ".join("%.4f" % x for x in rmed), rmed.max() - rmed.min(), moved[name] / 1e6,
                     moved[name] / (np.median(allv) * 1e-3) / 1e9))
        spread = max(stat["native"][1], stat["torch"][1])
        frac = moved["native"] / (stat["native"][0] * 1e-3) / COPY_PEAK
        verdict = stat["native"][0] <= stat["torch"][0] + spread
        ok = ok and verdict and same
        print("  native pair = %.1f %% of the 6.29 TB/s float4 copy rate (two launches; the events also span the gap between them)"
              % (100 * frac))
        print("  native median - torch median = %+.4f ms, run-to-run spread %.4f ms: %s"
              % (stat["native"][0] - stat["torch"][0], spread, "not slower" if verdict else "SLOWER"))
        r.destroy()
    print("\ncollective over xGMI: not measured (needs two or more GPUs)")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
