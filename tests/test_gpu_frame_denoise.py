"""The frame denoiser on the GPU (rt_denoise_frame / rt_denoise_frame_device / rt_set_present_denoise, csrc/k_frame_denoise.hip.h)
against the reference model (tests/model/frame_denoise_model.cpp, held to its properties by tests/test_frame_denoise_model.py),
word for word.

The G-buffer is cornell's after one compute() at the smallest shapes where the kernels can go wrong: 1 x 1, one column and one
row of 40, 33 x 9 (one 32 x 8 tile plus a column and a row), 70 x 37 (three tile columns, five tile rows; a spacing of 16
exceeds half the image) and 64 x 16 (whole tiles, five passes).  The accumulator is the renderer's own and one overwritten with
special values through rt_write_accum.  Every test makes one context and destroys it."""
import re

import numpy as np
import pytest

import frame_denoise_util as fu
import parity_util as pu

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (1, 40), (40, 1), (33, 9), (70, 37), (64, 16))
DESCS = (dict(fu.CORNELL, passes=1), dict(fu.CORNELL, step=16, passes=1), dict(fu.CORNELL, passes=5),
         dict(fu.CORNELL, step=3, passes=2, flags=fu.SAME_INSTANCE, sigma_lum=0.0))
NOT_READY = re.escape("frame denoise: the albedo plane was overwritten by present(); call compute first")


def start(W, r, width, height, frames=(1,)):
    """cornell, depth 4, 1 spp, the frames computed; -> the bridge"""
    b = pu.bridge_for(W, "cornell")
    r.buildPipeline(4, 1)
    W.upload_scene(r, b, width, height)
    for f in frames:
        r.compute(f)
    return b


def frame(r):
    """what the model needs, read back through the existing ABI"""
    return fu.frame_of(r.readAccum(), r.readGBuffer(), r.readUniforms())


def same(got, want, tag):
    bad = fu.differing(got, want)
    assert not bad.any(), (tag, "pixels differ at", np.argwhere(bad)[:8].tolist(), np.asarray(got)[bad][:4].tolist(),
                           np.asarray(want)[bad][:4].tolist())


@pytest.mark.parametrize("width,height", SHAPES)
def test_bit_parity_with_the_model(W, gpu_renderer, width, height):
    r = gpu_renderer
    start(W, r, width, height)
    fr = frame(r)
    assert (fr.albedo >> 24).any(), "cornell's walls fill the view: no surface pixel?"
    for special in (False, True):
        if special:
            r.writeAccum(fu.specials(fr.accum))
            fr = frame(r)
        for d in DESCS:
            want = fu.call(fr, d)
            same(r.denoiseFrame(fu.desc(**d)), want, (width, height, special, d))
            if special and width * height > 40:
                assert np.isnan(want).any() and np.isfinite(want).any()
    stats = r.frameDenoiseStats()
    assert stats["forms"] == ["lds", "direct"] and len(stats["pass_ms"]) == 2   # the last call: spacings 3 and 6, and 6 has no window


@pytest.mark.parametrize("width,height", ((33, 9), (70, 37)))
def test_the_two_forms_give_the_same_words(W, gpu_renderer, width, height):
    r = gpu_renderer
    start(W, r, width, height)
    r.writeAccum(fu.specials(r.readAccum()))
    fr = frame(r)
    for step in (1, 2, 3, 4):
        d = dict(fu.CORNELL, step=step, passes=1)
        out = {}
        for form in ("lds", "direct", "auto"):
            r.setFrameDenoiseForm(form)
            out[form] = r.denoiseFrame(fu.desc(**d))
            if form != "auto":
                assert r.frameDenoiseStats()["forms"] == [form]
        assert np.array_equal(fu.words(out["lds"]), fu.words(out["direct"])), step
        assert np.array_equal(fu.words(out["auto"]), fu.words(out["direct"])), step
        same(out["lds"], fu.call(fr, d), step)
    # a spacing without a window: the forced LDS form is refused before anything runs, the direct form serves it
    r.setFrameDenoiseForm("lds")
    with pytest.raises(W.RendererError, match="frame denoise: the LDS form is forced"):
        r.denoiseFrame(fu.desc(**dict(fu.CORNELL, step=1, passes=4)))
    r.setFrameDenoiseForm("direct")
    d = dict(fu.CORNELL, step=1, passes=4)
    same(r.denoiseFrame(fu.desc(**d)), fu.call(fr, d), "direct, four passes")


def test_host_call_equals_device_call(W, gpu_renderer):
    import torch
    r = gpu_renderer
    start(W, r, 70, 37)
    d = fu.desc(**fu.CORNELL)
    host = r.denoiseFrame(d)
    t = torch.zeros((37, 70, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.denoiseFrameDevice(t, d)
    r.sync()
    assert np.array_equal(fu.words(t.cpu().numpy()), fu.words(host))
    same(host, fu.call(frame(r), fu.CORNELL), "host")
    # refusals of the device entry: the accumulator as output, a misaligned or NULL output
    call = r.L.rt_denoise_frame_device
    for out in (r.accumDevicePtr(), t.data_ptr() + 4, None):
        assert call(r.ctx, d.ctypes.data, out) == -1
        assert r.L.rt_last_error(r.ctx).startswith(b"frame denoise:"), out


def _present_outputs(r):
    return r.captureFrame()["data"].copy(), r.readHistory()


def test_present_with_denoise_equals_the_explicit_sequence(W, gpu_renderer):
    import torch
    d = fu.desc(**fu.CORNELL)
    r = gpu_renderer
    start(W, r, 70, 37)
    r.setPresentDenoise(d)
    r.present()
    got = _present_outputs(r)
    r.compute(2)
    r.present()
    got2 = _present_outputs(r)
    r.destroy()
    r = W.WebGPURenderer(0)
    try:
        start(W, r, 70, 37)
        t = torch.zeros((37, 70, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for want in (got, got2):
            if want is got2:
                r.bindPresentSource(None)
                r.compute(2)
            r.denoiseFrameDevice(t, d)
            r.bindPresentSource(t.data_ptr())
            r.present()
            rgba, hist = _present_outputs(r)
            assert np.array_equal(rgba, want[0]) and np.array_equal(hist, want[1])
        # and it is not the plain path: the unfiltered present of the same frames differs
        r.bindPresentSource(None)
    finally:
        r.destroy()
    r = W.WebGPURenderer(0)
    try:
        start(W, r, 70, 37)
        r.setPresentDenoise(d)
        r.setPresentDenoise(None)        # NULL restores the plain path exactly
        r.present()
        plain = _present_outputs(r)
        assert not np.array_equal(plain[0], got[0])
    finally:
        r.destroy()
    r = W.WebGPURenderer(0)
    try:
        start(W, r, 70, 37)
        r.present()
        rgba, hist = _present_outputs(r)
        assert np.array_equal(rgba, plain[0]) and np.array_equal(hist, plain[1])
    finally:
        r.destroy()


def test_cache_serves_calls_after_present_until_the_next_compute(W, gpu_renderer):
    r = gpu_renderer
    start(W, r, 33, 9)
    d = fu.desc(**fu.CORNELL)
    first = r.denoiseFrame(d)
    assert r.frameDenoiseStats()["cache_hit"] is False
    r.setPresentDenoise(d)
    r.present()
    assert r.frameDenoiseStats()["cache_hit"] is True       # the explicit call before it prepared this G-buffer
    r.present()
    s = r.frameDenoiseStats()
    assert s["cache_hit"] is True and s["prepare_ms"] == 0.0 and len(s["pass_ms"]) == 4 and s["forms"] == ["lds", "lds", "direct", "direct"]
    assert np.array_equal(fu.words(r.denoiseFrame(d)), fu.words(first))     # the albedo plane is gone: the cache serves
    other = fu.desc(**dict(fu.CORNELL, flags=0))
    with pytest.raises(W.RendererError, match=NOT_READY):                  # another modulation needs the plane
        r.denoiseFrame(other)
    r.compute(2)
    fr = frame(r)
    r.present()
    assert r.frameDenoiseStats()["cache_hit"] is False
    same(r.denoiseFrame(d), fu.call(fr, fu.CORNELL), "frame 2 from the cache")
    assert r.frameDenoiseStats()["cache_hit"] is True
    r.setPresentDenoise(None)
    r.compute(3)
    r.present()
    with pytest.raises(W.RendererError, match=NOT_READY):                  # no cache and the plane gone
        r.denoiseFrame(d)
    r.compute(4)
    same(r.denoiseFrame(d), fu.call(frame(r), fu.CORNELL), "frame 4")


def test_lookahead_gives_the_same_filtered_frames(W, gpu_renderer):
    d = fu.desc(**fu.CORNELL)
    outs = []
    r = gpu_renderer
    for look in (0, 8):
        if look:
            r.destroy()
            r = W.WebGPURenderer(0)
        try:
            r.setLookahead(look)
            start(W, r, 33, 9, frames=())
            r.setPresentDenoise(d if look else None)
            got = []
            for f in range(1, 9):
                r.compute(f)
                got.append(r.denoiseFrame(d))
                r.present()
            outs.append(got)
        finally:
            if look:
                r.destroy()
    for f, (a, b) in enumerate(zip(*outs)):
        assert np.array_equal(fu.words(a), fu.words(b)), "frame %d" % (f + 1)


def test_resize_drops_the_state(W, gpu_renderer):
    r = gpu_renderer
    b = start(W, r, 64, 16)
    d = fu.desc(**fu.CORNELL)
    r.denoiseFrame(d)
    r.setPresentDenoise(d)
    r.present()
    r.updateScreenSize(21, 13)
    with pytest.raises(W.RendererError, match="frame denoise: no G-buffer yet; call compute first"):
        r.denoiseFrame(d)
    with pytest.raises(W.RendererError, match="frame denoise: no G-buffer yet; call compute first"):
        r.present()
    b.updateCamera(21, 13)
    r.updateSceneUniforms(b.cameraData, 0, b.lightCount)
    r.compute(1)
    fr = frame(r)
    same(r.denoiseFrame(d), fu.call(fr, fu.CORNELL), "after the resize")
    r.present()
    assert r.frameDenoiseStats()["cache_hit"] is True


def test_the_explicit_calls_have_no_side_effects(W, gpu_renderer):
    import torch
    r = gpu_renderer
    start(W, r, 70, 37, frames=(1, 2))
    r.present()
    r.compute(3)

    def state():
        return [r.readAccum(), r.readHistory(), r.readUniforms()] + list(r.readGBuffer()) + [np.array(list(r.getCounters().values()))]

    before = state()
    t = torch.zeros((37, 70, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for d in DESCS:
        r.denoiseFrame(fu.desc(**d))
        r.denoiseFrameDevice(t, fu.desc(**d))
    r.sync()
    for a, b in zip(before, state()):
        assert np.array_equal(pu.bits(a), pu.bits(b))


def test_refusals_on_a_context(W, gpu_renderer):
    import torch
    r = gpu_renderer
    d = fu.desc(**fu.CORNELL)
    with pytest.raises(W.RendererError, match="frame denoise:"):      # no screen
        r.denoiseFrame(d)
    start(W, r, 33, 9, frames=())
    with pytest.raises(W.RendererError, match="frame denoise: no G-buffer yet"):
        r.denoiseFrame(d)
    r.compute(1)
    for bad in (dict(passes=0), dict(passes=6), dict(step=0), dict(step=2, passes=5), dict(step=17, passes=1), dict(flags=4),
                dict(reserved=(0, 1))):
        for call in (r.denoiseFrame, r.setPresentDenoise):
            with pytest.raises(W.RendererError, match="frame denoise:"):
                call(fu.desc(**dict(fu.CORNELL, **bad)))
    out = np.zeros((9, 33, 4), np.float32)
    assert r.L.rt_denoise_frame(r.ctx, d.ctypes.data, out.ctypes.data, out.nbytes - 1) == -1
    assert r.L.rt_last_error(r.ctx).startswith(b"frame denoise:")
    # a bound present source, stripes: the setting is refused, and refuses them while it is set
    t = torch.zeros((9, 33, 4), dtype=torch.float32, device="cuda")
    r.bindPresentSource(t.data_ptr())
    with pytest.raises(W.RendererError, match="frame denoise: a present source is bound"):
        r.setPresentDenoise(d)
    r.bindPresentSource(None)
    r.setStripes(8, 0, 2)
    with pytest.raises(W.RendererError, match="frame denoise: stripes are on"):
        r.setPresentDenoise(d)
    with pytest.raises(W.RendererError, match="frame denoise: stripes are on"):
        r.denoiseFrame(d)
    r.setStripes(0, 0, 1)
    r.setPresentDenoise(d)
    with pytest.raises(W.RendererError, match="rt_bind_present_source: present\\(\\) filters the frame"):
        r.bindPresentSource(t.data_ptr())
    with pytest.raises(W.RendererError, match="rt_set_stripes: present\\(\\) filters the frame"):
        r.setStripes(8, 0, 2)
    assert r.L.rt_dist_init(r.ctx, 0, 2, 8, None) == -1
    assert b"rt_dist_init: present() filters the frame" in r.L.rt_last_error(r.ctx)
    r.setPresentDenoise(None)
    r.bindPresentSource(t.data_ptr())
    r.bindPresentSource(None)
