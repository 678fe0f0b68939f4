"""Contexts come and go without touching one another (rt_create / rt_destroy; csrc/device_owned.h).  A context's device
buffers, events, streams and pinned blocks belong to member types and go with it, so what this test can see of a wrong owner
is a result that changes, or a call that fails, once another context has been destroyed or one has been created where an
old one lay: a buffer or an event freed twice, freed while its context lives, or handed from one state to another.

Cornell, a 16 x 16 screen, depth 2, spp 2, kernel timing on (so every family creates its events).  One ROUND runs one call of
every family that owns state, at the smallest shapes.  Two contexts run a round each; the first is destroyed; the second runs
the round again and must return, word for word, what it returned before.  Then a context is created, runs the round and is
destroyed, three times, with the same words.  Only equality and clean return codes are asserted: no memory counter is read
(on a shared card, free memory moves with other people's work)."""
import numpy as np
import pytest

import bake_util as bu
import denoise_util as du
import parity_util as pu

pytestmark = pytest.mark.gpu

SCREEN, DEPTH, SPP, SEED = 16, 2, 2, 7
ATLAS = 8
FILTER = dict(du.PARAMS, passes=1, step=1)
GRID = (2, 2, 2)


def _words(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8).copy()


def _counts(stats):
    """a stats dict without its one measured figure, which must be there: timing is on and the family has recorded its events"""
    assert stats["kernel_ms"] > 0.0, stats
    return {k: v for k, v in stats.items() if k != "kernel_ms"}


def _new_context(W):
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    r.buildPipeline(DEPTH, SPP)
    r.setKernelTiming(True)
    return r


def _round(W, r, b):
    """One call of every family -> [(name, words or counts)], in the order of the calls."""
    from webgpu_raytracer_amd import renderer as R
    out = []

    def keep(name, *items):
        for k, it in enumerate(items):
            out.append(("%s[%d]" % (name, k), it if isinstance(it, (dict, int)) else _words(it)))

    # frames: a fresh screen and accumulation, a batch of two frames, a present.  The jitter of a frame is Halton at the
    # context's frame total modulo 16, which no call resets: the round ends with 14 frames more, so the next one starts where
    # this one did.
    W.upload_scene(r, b, SCREEN, SCREEN)
    r.computeBatch([1, 2])
    r.present()
    keep("frames", r.readAccum(), r.captureFrame()["data"])
    keep("kernel times", int(r.kernelTimeMs()["launches"] > 0))
    r.computeBatch(list(range(3, 17)))

    # the point pass of a whole-atlas bake of instance 0, its triangles laid out as charts with gutters between them: its first
    # four points feed the queries
    uv = bu.grid_uv(b, 0)
    points, texels = r.bakePoints(0, ATLAS, ATLAS, t_max=5.0, pad_base=100, atlas_uv=uv)
    assert len(texels) >= 4
    keep("bakePoints", points, texels)
    p4 = points[:4].copy()
    rays = p4.copy()
    rays[:, 0:3] = p4[:, 0:3] + np.float32(0.01) * p4[:, 4:7]     # from just above the surface along its normal
    probes = p4.copy()
    probes[:, 0:3] = p4[:, 0:3] + np.float32(0.25) * p4[:, 4:7]
    probes[:, 4:7] = 0.0

    hits, st = r.traceRays(rays, stats=True)
    keep("traceRays", hits, _counts(st))
    for name, call, items in (("traceRadiance", r.traceRadiance, rays), ("gatherIrradiance", r.gatherIrradiance, p4),
                              ("gatherProbes", r.gatherProbes, probes), ("gatherDirectional", r.gatherDirectional, p4)):
        res, st = call(items, DEPTH, SPP, SEED, stats=True)
        keep(name, res, _counts(st))

    entries = [(0, 0, 0, ATLAS, ATLAS)]
    bake = dict(t_max=5.0, pad_base=100, atlas_uv=uv, denoise=FILTER, dilate=1, stats=True)
    atlas, n, filled, st = r.bakeAtlasLightmap(entries, ATLAS, ATLAS, DEPTH, SPP, SEED, **bake)
    keep("bakeAtlasLightmap", atlas, n, filled, _counts(st))
    layers, n, filled, st = r.bakeAtlasDirectionalLightmap(entries, ATLAS, ATLAS, DEPTH, SPP, SEED, **bake)
    keep("bakeAtlasDirectionalLightmap", layers, n, filled, _counts(st))

    keep("dilateAtlas", *r.dilateAtlas(atlas, 1, src=True, filled=True))
    keep("denoiseAtlas", r.denoiseAtlas(atlas, points, texels, **FILTER))
    keep("encodeAtlas", r.encodeAtlas(atlas, "f16"), r.encodeAtlas(atlas, "rgbe"))

    lo = points[:, 0:3].min(axis=0)
    step = np.maximum((points[:, 0:3].max(axis=0) - lo) / np.float32(2.0), np.float32(0.05))
    desc = R.volume_desc(tuple(lo + 0.25 * step), tuple(step), GRID, t_max=5.0, pad_first=200)
    volume, st = r.bakeVolume(desc, DEPTH, SPP, SEED, stats=True)
    keep("bakeVolume", volume, _counts(st))
    keep("sampleVolume", r.sampleVolume(desc, volume, p4))
    keep("encodeVolume", r.encodeVolume(desc, volume, "f16"))
    r.sync()
    return out


def _same(got, want, tag):
    assert [n for n, _ in got] == [n for n, _ in want], tag
    for (name, a), (_, b) in zip(got, want):
        if isinstance(a, np.ndarray):
            assert a.shape == b.shape and np.array_equal(a, b), "%s: %s differs in %d bytes" % (tag, name, int((a != b).sum()))
        else:
            assert a == b, "%s: %s: %r != %r" % (tag, name, a, b)


def test_contexts_come_and_go(W):
    b = pu.bridge_for(W, "cornell")
    first, second = _new_context(W), _new_context(W)
    try:
        want_first = _round(W, first, b)
        want = _round(W, second, b)
        # the round is not empty: something was hit, lit, covered and filled
        named = dict(want)
        assert named["bakeAtlasLightmap[1]"] >= 4 and named["bakeAtlasLightmap[2]"] >= 1 and named["bakeAtlasDirectionalLightmap[2]"] >= 1
        for name in ("frames[0]", "traceRadiance[0]", "gatherProbes[0]", "gatherDirectional[0]", "bakeVolume[0]"):
            assert named[name].view(np.float32).max() > 0.0, name
        _same(want_first, want, "two contexts side by side")
        first.destroy()
        _same(_round(W, second, b), want, "after the other context was destroyed")
    finally:
        first.destroy()
        second.destroy()
    for k in range(3):
        r = _new_context(W)
        try:
            _same(_round(W, r, b), want, "context %d created after the others were destroyed" % k)
        finally:
            r.destroy()
