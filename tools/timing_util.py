"""Shared pieces of the timing tools (tools/*_time.py): the line a list of rounds prints as, the pinhole rays of the scene
camera, and the project's RNG (init_rng / rand_pcg of mi355rt.h) in numpy uint32 / float32 arithmetic."""
import functools
import statistics

import numpy as np

U = np.uint32


def fmt(vals, unit="ms", digits=3, median=statistics.median):
    """the median of the rounds with (min .. max) beside it, `digits` decimals"""
    f = "%%.%df" % digits
    return (f + " %s (min " + f + " .. max " + f + " over %d rounds)") % (median(vals), unit, min(vals), max(vals), len(vals))


fmt2 = functools.partial(fmt, digits=2)   # the atlas tools print two decimals


def camera_rays(bridge, width, height, pads=False):
    """one pinhole ray per cell centre of a width x height raster, row order, rt_ray layout; pads: pad = cell index"""
    cam = np.asarray(bridge.cameraData, np.float32).reshape(6, 4)
    o, ll, hz, vt = cam[0, :3], cam[1, :3], cam[2, :3], cam[3, :3]
    u = (np.arange(width, dtype=np.float32) + np.float32(0.5)) / np.float32(width)
    v = (np.arange(height, dtype=np.float32) + np.float32(0.5)) / np.float32(height)
    d = ll[None, None, :] + u[None, :, None] * hz[None, None, :] + v[:, None, None] * vt[None, None, :] - o[None, None, :]
    rays = np.zeros((height * width, 8), np.float32)
    rays[:, 0:3] = o
    rays[:, 3] = 1e30
    rays[:, 4:7] = d.reshape(-1, 3)
    if pads:
        rays.view(U)[:, 7] = np.arange(height * width, dtype=U)
    return rays


def init_rng(a, b):
    """the state of stream a (u32 array) at frame b (u32 scalar or array): the hash of a + b * 719393"""
    with np.errstate(over="ignore"):
        s = (a + b * U(719393)).astype(U)
        s ^= U(2747636419)
        for _ in range(2):
            s *= U(2654435769)
            s ^= s >> U(16)
        s *= U(2654435769)
    return s


def rand_pcg(state):
    """steps `state` (u32 array, in place) and -> the float32 in [0, 1) of the step: word * 2^-32"""
    with np.errstate(over="ignore"):
        old = state.copy()
        state *= U(747796405)
        state += U(2891336453)
        word = (state >> ((old >> U(28)) + U(4))) ^ state
    return ((word >> U(22)) ^ word).astype(np.float32) / np.float32(4294967296.0)
