#!/usr/bin/env python3
"""Lane utilisation of k_pathtrace_persistent by part of a trip (Cornell, one 32-frame batch of the bench workload).
DIAGNOSTIC build -DRT_LANE_STATS: a ballot + two atomics where a wave enters a part (counts, no timing; the share of a wave's
cycles each section takes comes from tools/pt_sections.py, its own process and build).  Rebuilds the product library at the end.
usage: lane_stats.py [scene]"""
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import webgpu_raytracer_amd as W  # noqa: E402

scene = sys.argv[1] if len(sys.argv) > 1 else "cornell"
# one-leaf forms: a new hit only records itself (part 5) and a new sample only makes its camera ray and loads its G-buffer
# words (part 6); one pass at the start of the trip makes the surface frame of both (part 8).  The other forms make the
# frame in parts 5 and 6 and have no part 8.
# a sweep form (k_traverse.hip.h traverse_leaves; MI355RT_LEAF_SWEEP=0 gives the node walk) counts a leaf step as a node step
PARTS = ("shade", "shadow walk: node step (sweep: leaf step)", "shadow walk: triangle chunk", "extension walk: node step (sweep: leaf step)",
         "extension walk: triangle chunk", "new hit (one-leaf: recorded; else + surface frame)",
         "start of a sample (one-leaf: camera ray + G-buffer words; else + surface frame)", "end of a sample",
         "surface frame, one pass (one-leaf forms)")
# sweep forms only, per walk that has a walking lane: all of them, those that take the node sweep (a lane with a non-finite
# reciprocal direction or origin term sends its wave there), and the lanes that have such a term
WALKS = ("sweep-form walk", "... through the node sweep (cold path)", "... with a lane of a non-finite slab operand")


def render(flags):
    W._build.build_rt(force=True, extra_flags=flags)
    b = W.WorldBridge()
    b.loadScene(scene)
    r = W.WebGPURenderer(0)
    r.buildPipeline(8, 1)
    W.upload_scene(r, b, 1920, 1080)
    r.setKernelVariant(1)
    fl = list(range(1, 33))
    r.computeBatch(fl)
    r.sync()
    return r, fl


try:
    r, fl = render(["-DRT_LANE_STATS"])
    buf = np.zeros(32, dtype=np.uint64)
    r.L.rt_debug_lane_stats(r.ctx, buf.ctypes.data_as(ctypes.c_void_p), 1)
    r.computeBatch(fl)
    r.sync()
    r.L.rt_debug_lane_stats(r.ctx, buf.ctypes.data_as(ctypes.c_void_p), 1)
    n, lanes = buf[0:18:2].astype(float), buf[1:18:2].astype(float)
    trips = n[0]
    print("scene=%s, one 32-frame batch: %d wave-level trips that shade (walk: %s)" % (scene, trips, r.debugPtWalk()))
    print("   %-80s %14s %12s %12s" % ("part", "runs per trip", "lanes / run", "utilisation"))
    for k, name in enumerate(PARTS):
        if n[k]:
            print("   %-80s %14.2f %12.1f %12.3f" % (name, n[k] / trips, lanes[k] / n[k], lanes[k] / n[k] / 64.0))
    wn, wl = buf[18:24:2].astype(float), buf[19:24:2].astype(float)
    if wn[0]:
        print("   %-80s %14s %12s %12s" % ("walks", "per trip", "lanes / walk", "share of walks"))
        for k, name in enumerate(WALKS):
            print("   %-80s %14.4f %12.1f %12.6f" % (name, wn[k] / trips, wl[k] / wn[k] if wn[k] else 0.0, wn[k] / wn[0]))
        print("   lanes with a non-finite slab operand: %d of %d walking lanes (%.3g)" % (wl[2], wl[0], wl[2] / wl[0]))
    r.destroy()
finally:
    W._build.build_rt(force=True)
