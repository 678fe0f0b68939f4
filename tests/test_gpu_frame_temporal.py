"""The temporal stage of the frame denoiser on the GPU (rt_set_frame_temporal / rt_reset_frame_history / rt_read_frame_history,
csrc/k_frame_temporal.hip.h) against the reference model (tests/model/frame_temporal_model.cpp, held to its properties by
tests/test_frame_temporal_model.py), word for word: the filtered image and the history, colour and moments, after every frame
of a sequence of three on cornell with the camera translated between them - once by less than a pixel, once by about two.

The shapes are the smallest where the kernel can go wrong: 1 x 1, one column and one row of 40, 33 x 9, 70 x 37 and 260 x 2,
where the footprint crosses the seam of the 256-thread blocks.  The accumulator is the renderer's own and, in the middle frame,
one overwritten with special values through rt_write_accum.  Every test makes its contexts and destroys them."""
import numpy as np
import pytest

import frame_denoise_util as fu
import frame_temporal_util as tu
import parity_util as pu

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (1, 40), (40, 1), (33, 9), (70, 37), (260, 2))
D = fu.CORNELL
T = tu.CORNELL
# the camera of frame k, in pixels along the camera's horizontal and vertical - pixels of an image of at least 70 x 37, so that
# the degenerate shapes move by the same world distances: a sub-pixel step, then one of about two pixels (surfaces lie behind
# the image plane, so they move by less on the screen)
OFFSETS = ((0.0, 0.0), (0.6, 0.35), (3.4, 1.9))
# at 260 x 2 a pixel of the image plane is wider than cornell's box, which then covers four pixels in the middle of the row: from
# 100 pixels to the side the camera sees its outer wall across columns 199 .. 259, over the seam of the blocks at 255 | 256
BASE = {(260, 2): -100.0}


def camera_of(b, width, height, k):
    cam = np.array(b.cameraData, dtype=np.float32).reshape(6, 4).copy()
    ox = OFFSETS[k][0] / max(width, 70) + BASE.get((width, height), 0.0) / width
    shift = cam[2, :3] * np.float32(ox) + cam[3, :3] * np.float32(OFFSETS[k][1] / max(height, 37))
    cam[0, :3] += shift
    cam[1, :3] += shift
    return cam.reshape(-1)


def start(W, r, width, height):
    b = pu.bridge_for(W, "cornell")
    r.buildPipeline(4, 1)
    W.upload_scene(r, b, width, height)
    return b


def render(r, b, width, height, k):
    """frame k of the sequence: its camera, a fresh accumulation, one sample per pixel"""
    r.updateSceneUniforms(camera_of(b, width, height, k), 0, b.lightCount)
    r.resetAccumulation()
    r.compute(k + 1)


def frame(r):
    return fu.frame_of(r.readAccum(), r.readGBuffer(), r.readUniforms())


def same(got, want, tag):
    bad = fu.differing(got, want)
    assert not bad.any(), (tag, "pixels differ at", np.argwhere(bad)[:8].tolist(), np.asarray(got)[bad][:4].tolist(),
                           np.asarray(want)[bad][:4].tolist())


def same_history(r, st, tag):
    col, mom, frames = r.readFrameHistory()
    same(col, st.hist, (tag, "history colour"))
    same(mom, st.mom, (tag, "history moments"))
    assert frames == st.frames == r.readFrameHistory(frames_only=True), tag


def sequence_condition(st, width, height):
    """frame 2 of a shape above 40 pixels has surface pixels with history and surface pixels without: both paths ran"""
    if width * height <= 40:
        return
    surf = fu.words(st.guide[..., 7]) != 0
    n = st.n()[surf]
    assert (n >= 2).any() and (n == 1).any(), (width, height, n.tolist())
    if width > 256:
        cols = np.nonzero(surf)[1]
        assert (cols <= 255).any() and (cols >= 256).any(), "the surface lies across the seam of the 256-thread blocks"


@pytest.mark.parametrize("width,height", SHAPES)
def test_bit_parity_with_the_model_over_a_sequence(W, gpu_renderer, width, height):
    r = gpu_renderer
    b = start(W, r, width, height)
    r.setFrameTemporal(tu.desc(**T))
    st = tu.History()
    for k in range(3):
        render(r, b, width, height, k)
        if k == 1:
            r.writeAccum(fu.specials(r.readAccum()))
        fr = frame(r)
        want, _, acc = tu.call(fr, D, T, st)
        same(r.denoiseFrame(fu.desc(**D)), want, (width, height, k))
        same_history(r, st, (width, height, k))
        s = r.frameDenoiseStats()
        assert s["temporal"] == "ran" and s["temporal_ms"] > 0.0 and s["cache_hit"] is False
        if k == 1:
            sequence_condition(st, width, height)
        if k == 2 and width * height > 40:
            assert np.isnan(st.hist).any() and np.isfinite(st.hist[..., :3]).any(), "the specials of frame 1 are in the history"
    assert (fr.albedo >> 24).any(), "cornell's walls fill the view: no surface pixel?"


@pytest.mark.parametrize("t", (dict(T, flags=tu.SAME_INSTANCE, max_history=2, var_history=1), dict(T, max_history=1),
                               dict(T, normal_cos=float("nan"))))
def test_bit_parity_under_other_descriptors(W, gpu_renderer, t):
    r = gpu_renderer
    width, height = 70, 37
    b = start(W, r, width, height)
    r.setFrameTemporal(tu.desc(**t))
    st = tu.History()
    d = dict(D, passes=2, flags=fu.SAME_INSTANCE)      # no demodulation: the history holds radiance
    for k in range(3):
        render(r, b, width, height, k)
        want, _, _ = tu.call(frame(r), d, t, st)
        same(r.denoiseFrame(fu.desc(**d)), want, (t, k))
        same_history(r, st, (t, k))
    assert st.n().max() == min(2, t["max_history"]) or t["normal_cos"] != t["normal_cos"]


def test_the_two_forms_behind_the_stage_give_the_same_words(W):
    d3 = dict(D, passes=3)                               # spacings 1, 2, 4: every one has both forms
    outs = {}
    for form in ("lds", "direct"):
        r = W.WebGPURenderer(0)
        try:
            b = start(W, r, 70, 37)
            r.setFrameTemporal(tu.desc(**T))
            r.setFrameDenoiseForm(form)
            outs[form] = []
            for k in range(3):
                render(r, b, 70, 37, k)
                outs[form].append(r.denoiseFrame(fu.desc(**d3)))
                assert r.frameDenoiseStats()["forms"] == [form] * 3
        finally:
            r.destroy()
    for k, (a, c) in enumerate(zip(outs["lds"], outs["direct"])):
        assert np.array_equal(fu.words(a), fu.words(c)), k


def test_host_call_equals_device_call_and_a_second_call_reuses_the_image(W, gpu_renderer):
    import torch
    r = gpu_renderer
    b = start(W, r, 70, 37)
    r.setFrameTemporal(tu.desc(**T))
    d = fu.desc(**D)
    t = torch.zeros((37, 70, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = tu.History()
    for k in range(3):
        render(r, b, 70, 37, k)
        fr = frame(r)
        if k % 2 == 0:
            host = r.denoiseFrame(d)
            assert r.frameDenoiseStats()["temporal"] == "ran"
            before = r.readFrameHistory()
            r.denoiseFrameDevice(t, d)
            r.sync()
        else:                                            # ... and the device entry first
            r.denoiseFrameDevice(t, d)
            r.sync()
            assert r.frameDenoiseStats()["temporal"] == "ran"
            before = r.readFrameHistory()
            host = r.denoiseFrame(d)
        s = r.frameDenoiseStats()
        assert s["temporal"] == "reused" and s["temporal_ms"] == 0.0 and s["cache_hit"] is True
        after = r.readFrameHistory()
        assert after[2] == before[2] == k + 1
        assert np.array_equal(fu.words(after[0]), fu.words(before[0])) and np.array_equal(fu.words(after[1]), fu.words(before[1]))
        assert np.array_equal(fu.words(t.cpu().numpy()), fu.words(host)), k
        same(host, tu.call(fr, D, T, st)[0], k)


def _present_outputs(r):
    return r.captureFrame()["data"].copy(), r.readHistory()


def test_present_with_the_stage_on_equals_the_explicit_sequence(W, gpu_renderer):
    import torch
    d = fu.desc(**D)
    r = gpu_renderer
    b = start(W, r, 70, 37)
    r.setPresentDenoise(d)
    r.setFrameTemporal(tu.desc(**T))
    got = []
    for k in range(3):
        render(r, b, 70, 37, k)
        r.present()
        assert r.frameDenoiseStats()["temporal"] == "ran"
        got.append(_present_outputs(r))
    assert r.readFrameHistory(frames_only=True) == 3
    r.destroy()
    r = W.WebGPURenderer(0)
    try:
        b = start(W, r, 70, 37)
        r.setFrameTemporal(tu.desc(**T))
        t = torch.zeros((37, 70, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for k in range(3):
            r.bindPresentSource(None)
            render(r, b, 70, 37, k)
            r.denoiseFrameDevice(t, d)
            r.bindPresentSource(t.data_ptr())
            r.present()
            rgba, hist = _present_outputs(r)
            assert np.array_equal(rgba, got[k][0]) and np.array_equal(hist, got[k][1]), k
        r.bindPresentSource(None)
    finally:
        r.destroy()
    # and the stage is not a no-op in that sequence: the spatial filter alone presents other bytes from the second frame on
    r = W.WebGPURenderer(0)
    try:
        b = start(W, r, 70, 37)
        r.setPresentDenoise(d)
        for k in range(2):
            render(r, b, 70, 37, k)
            r.present()
            assert np.array_equal(_present_outputs(r)[0], got[k][0]) == (k == 0), k
    finally:
        r.destroy()


def test_lookahead_gives_the_same_filtered_frames(W, gpu_renderer):
    d = fu.desc(**D)
    outs = []
    r = gpu_renderer
    for look in (0, 8):
        if look:
            r.destroy()
            r = W.WebGPURenderer(0)
        try:
            r.setLookahead(look)
            start(W, r, 33, 9)
            r.setFrameTemporal(tu.desc(**T))
            r.setPresentDenoise(d if look else None)
            got = []
            for f in range(1, 9):
                r.compute(f)
                got.append(r.denoiseFrame(d))
                r.present()
            assert r.readFrameHistory(frames_only=True) == 8
            outs.append(got)
        finally:
            if look:
                r.destroy()
    for f, (a, b) in enumerate(zip(*outs)):
        assert np.array_equal(fu.words(a), fu.words(b)), "frame %d" % (f + 1)


def test_the_history_is_dropped_by_reset_demodulate_flip_and_resize_and_kept_by_the_rest(W, gpu_renderer):
    r = gpu_renderer
    width, height = 33, 9
    b = start(W, r, width, height)
    r.setFrameTemporal(tu.desc(**T))
    st = tu.History()

    def step(k, d, tag):
        render(r, b, r.width, r.height, k)
        same(r.denoiseFrame(fu.desc(**d)), tu.call(frame(r), d, T, st)[0], tag)
        same_history(r, st, tag)

    step(0, D, "first")
    step(1, D, "second")
    assert st.n().max() == 2
    r.resetFrameHistory()
    assert r.readFrameHistory(frames_only=True) == 0
    with pytest.raises(W.RendererError, match="frame temporal: no history yet"):
        r.readFrameHistory()
    st = tu.History()
    step(2, D, "after rt_reset_frame_history")
    assert st.n().max() == 1
    step(1, D, "one more")
    assert st.n().max() == 2
    step(2, dict(D, flags=0), "after a DEMODULATE flip")      # tu.call drops its state as the library must
    assert st.n().max() == 1 and st.frames == 1
    # not dropped: a scene upload, rt_set_scene and rt_reset_accum (render() does the last two every frame)
    r.updateBuffer("instance", b.instances)
    step(1, dict(D, flags=0), "after an upload")
    assert st.n().max() == 2
    r.updateScreenSize(21, 13)
    assert r.readFrameHistory(frames_only=True) == 0
    b.updateCamera(21, 13)
    st = tu.History()
    step(0, D, "after rt_resize")
    assert st.n().max() == 1
    step(1, D, "and on")
    assert st.n().max() == 2
    b.updateCamera(width, height)


def test_null_restores_the_words_of_a_context_that_never_enabled_the_stage(W, gpu_renderer):
    r = gpu_renderer
    b = start(W, r, 70, 37)
    d = fu.desc(**D)
    r.setFrameTemporal(tu.desc(**T))
    for k in range(2):
        render(r, b, 70, 37, k)
        r.denoiseFrame(d)
    r.setFrameTemporal(None)
    got = []
    got.append(r.denoiseFrame(d))                        # the same G-buffer again, now plain
    s = r.frameDenoiseStats()
    assert s["temporal"] == "off" and s["temporal_ms"] == 0.0
    same(got[0], fu.call(frame(r), D), "plain, same frame")
    render(r, b, 70, 37, 2)
    got.append(r.denoiseFrame(d))
    same(got[1], fu.call(frame(r), D), "plain, next frame")
    assert r.readFrameHistory(frames_only=True) == 0
    with pytest.raises(W.RendererError, match="frame temporal: the stage is off"):
        r.readFrameHistory()
    r.destroy()
    r = W.WebGPURenderer(0)
    try:
        b = start(W, r, 70, 37)
        for k in range(3):
            render(r, b, 70, 37, k)
            if k >= 1:
                assert np.array_equal(fu.words(r.denoiseFrame(d)), fu.words(got[k - 1])), k
    finally:
        r.destroy()


def test_refusals_on_a_context(W, gpu_renderer):
    r = gpu_renderer
    d = fu.desc(**D)
    for bad in (dict(flags=2), dict(flags=1 << 31), dict(reserved=(0, 0, 1)), dict(max_history=0), dict(max_history=257),
                dict(var_history=0)):
        with pytest.raises(W.RendererError, match="frame temporal:"):
            r.setFrameTemporal(tu.desc(**dict(T, **bad)))
    r.setFrameTemporal(tu.desc(**dict(T, max_history=256, var_history=1 << 31, normal_cos=float("nan"))))   # the limits are legal
    r.setFrameTemporal(tu.desc(**T))
    with pytest.raises(W.RendererError, match="frame denoise:"):      # no screen
        r.denoiseFrame(d)
    b = start(W, r, 33, 9)
    render(r, b, 33, 9, 0)
    r.setStripes(8, 0, 2)
    with pytest.raises(W.RendererError, match="frame denoise: stripes are on"):
        r.denoiseFrame(d)
    r.setStripes(0, 0, 1)
    r.distInit(0, 1, 8)
    try:
        with pytest.raises(W.RendererError, match="frame denoise: the context is a rank"):
            r.denoiseFrame(d)
        with pytest.raises(W.RendererError, match="frame denoise: the context is a rank"):
            r.setPresentDenoise(d)
    finally:
        r.distShutdown()
    assert r.readFrameHistory(frames_only=True) == 0                  # a refused call integrates nothing
