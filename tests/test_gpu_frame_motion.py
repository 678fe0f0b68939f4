"""Frame motion on the GPU (RT_FRAME_TEMPORAL_MOTION: csrc/k_frame_motion.hip.h, k_frame_temporal_motion, the snapshot) against
the reference model (tests/model/frame_motion_model.cpp, held to its properties by tests/test_frame_motion_model.py), word for
word: the carry plane, the filtered image, the history colour, the moments and the frame count after every frame of a sequence
of three.

Sequence (a) is frame_motion_util.sequence_a on the upload path: a wall, a card that translates and rotates and one that stays,
the TLAS order changed every frame with the ids declared (tests/test_frame_motion_sequences.py checks on the oracle's frames that
it meets the conditions asserted here).  Sequence (b) is test_gltf.build_skinned through the device updater at t = 0, 0.3 and
0.9, the scene arrays and RT_WORLD_INSTANCE_ORDER read back for the model.  The shapes are those of the temporal tests; the
middle frame's accumulator holds special values.  Every test makes its contexts and destroys them."""
import numpy as np
import pytest

import frame_denoise_util as fu
import frame_motion_util as mu
import frame_temporal_util as tu
import test_gltf

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (1, 40), (40, 1), (33, 9), (70, 37), (260, 2))
D = fu.CORNELL
T = dict(tu.CORNELL, flags=mu.MOTION | mu.SAME_INSTANCE)


def frame(r):
    return fu.frame_of(r.readAccum(), r.readGBuffer(), r.readUniforms())


def same(got, want, tag):
    bad = fu.differing(got, want)
    assert not bad.any(), (tag, "pixels differ at", np.argwhere(bad)[:8].tolist(), np.asarray(got)[bad][:4].tolist(),
                           np.asarray(want)[bad][:4].tolist())


def check(r, st, want, carry, tag, d=D):
    same(r.denoiseFrame(fu.desc(**d)), want, (tag, "filtered image"))
    got = r.readFrameMotion()
    assert np.array_equal(fu.words(got[..., 3]), fu.words(carry[..., 3])), (tag, "status")
    assert np.array_equal(fu.words(got[..., 7]), fu.words(carry[..., 7])), (tag, "stable ids")
    same(got, carry, (tag, "carry"))
    col, mom, frames = r.readFrameHistory()
    same(col, st.hist, (tag, "history colour"))
    same(mom, st.mom, (tag, "history moments"))
    assert frames == st.frames, tag
    s = r.frameDenoiseStats()
    assert s["temporal"] == "ran" and s["motion"] is True and s["motion_ms"] > 0.0 and s["temporal_ms"] > 0.0, (tag, s)


def render_a(W, r, k, width, height):
    b, ids = mu.sequence_a(k, width, height)
    mu.upload_frame(W, r, b, ids, width, height, k == 0)
    r.compute(k + 1)
    return b, ids


@pytest.mark.parametrize("width,height", SHAPES)
def test_sequence_a_moving_card_and_reordered_tlas(W, gpu_renderer, width, height):
    r = gpu_renderer
    r.buildPipeline(4, 1)
    st = mu.History()
    for k in range(3):
        b, ids = render_a(W, r, k, width, height)
        if k == 0:
            r.setFrameTemporal(tu.desc(**T))
        if k == 1:
            r.writeAccum(fu.specials(r.readAccum()))
        fr = frame(r)
        want, _, _, c = mu.call(fr, mu.scene_of(b, ids), D, T, st)
        check(r, st, want, c, ("a", width, height, k))
        if k == 1:
            mu.sequence_conditions(c, st.n(), st.guide, width, height)
    assert st.frames == 3


def skinned(W, r, width, height):
    b = W.WorldBridge()
    b.setDeviceUpdater(r)
    b.loadScene("viewer", glbData=test_gltf.build_skinned(W)[0].glb())
    W.upload_scene(r, b, width, height)
    return b


def world_scene(r):
    return mu.Scene(r.worldRead("mesh_topology"), r.worldRead("vertices"), r.worldRead("instances"), r.worldRead("instance_order"))


@pytest.mark.parametrize("width,height", SHAPES)
def test_sequence_b_skinned_mesh_through_the_device_updater(W, gpu_renderer, width, height):
    r = gpu_renderer
    r.buildPipeline(4, 1)
    b = skinned(W, r, width, height)
    r.setFrameTemporal(tu.desc(**T))
    st = mu.History()
    for k, t in enumerate((0.0, 0.3, 0.9)):
        b.update(t)
        assert b.deviceResident, b.deviceWarning
        W.sync_world(r, b, width, height)
        r.compute(k + 1)
        if k == 1:
            r.writeAccum(fu.specials(r.readAccum()))
        scene = world_scene(r)
        assert sorted(scene.ids.tolist()) == list(range(len(scene.inst)))
        want, _, _, c = mu.call(frame(r), scene, D, T, st)
        check(r, st, want, c, ("b", width, height, k))
        if k == 1 and (width, height) == (70, 37):   # the strip is a few pixels wide: it crosses no block seam at 260 x 2
            s = mu.status(c)
            surf = fu.words(st.guide[..., 7]) != 0
            assert ((s == mu.MOVED) & (st.n() >= 2)).any() and (s == mu.UNMOVED).any() and (surf & (st.n() == 1)).any()
    b.close()


def test_flag_off_on_a_context_that_had_it_on_restores_the_static_words(W, gpu_renderer):
    r = gpu_renderer
    r.buildPipeline(4, 1)
    width, height = 70, 37
    static = dict(T, flags=tu.SAME_INSTANCE)
    for k in range(2):
        render_a(W, r, k, width, height)
        if k == 0:
            r.setFrameTemporal(tu.desc(**T))
        r.denoiseFrame(fu.desc(**D))
    r.setFrameTemporal(tu.desc(**static))
    with pytest.raises(W.RendererError, match="frame motion: the stage has not run yet"):
        r.readFrameMotion()
    st = tu.History()
    for k in range(3):
        render_a(W, r, k, width, height)
        want, _, _ = tu.call(frame(r), D, static, st)
        same(r.denoiseFrame(fu.desc(**D)), want, ("static again", k))
        s = r.frameDenoiseStats()
        assert s["motion"] is False and s["motion_ms"] == 0.0
        col, mom, frames = r.readFrameHistory()
        same(col, st.hist, k)
        assert frames == st.frames


def test_host_path_device_path_and_filtered_present_agree(W, gpu_renderer):
    import torch
    r = gpu_renderer
    r.buildPipeline(4, 1)
    width, height = 70, 37
    d = fu.desc(**D)
    t = torch.zeros((height, width, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = mu.History()
    shown = []
    for k in range(3):
        b, ids = render_a(W, r, k, width, height)
        if k == 0:
            r.setFrameTemporal(tu.desc(**T))
        want, _, _, c = mu.call(frame(r), mu.scene_of(b, ids), D, T, st)
        if k % 2 == 0:
            host = r.denoiseFrame(d)
            r.denoiseFrameDevice(t, d)
        else:
            r.denoiseFrameDevice(t, d)
            r.sync()
            host = r.denoiseFrame(d)
        r.sync()
        s = r.frameDenoiseStats()
        assert s["temporal"] == "reused" and s["motion"] is False, "the second call on a G-buffer runs neither stage again"
        assert np.array_equal(fu.words(t.cpu().numpy()), fu.words(host)), k
        same(host, want, k)
        same(r.readFrameMotion(), c, (k, "carry"))
        assert r.readFrameHistory(frames_only=True) == k + 1
        r.bindPresentSource(t.data_ptr())
        r.present()
        shown.append(r.captureFrame()["data"].copy())
        r.bindPresentSource(None)
    r.destroy()
    r = W.WebGPURenderer(0)
    try:
        r.buildPipeline(4, 1)
        for k in range(3):
            render_a(W, r, k, width, height)
            if k == 0:
                r.setPresentDenoise(d)
                r.setFrameTemporal(tu.desc(**T))
            r.present()
            s = r.frameDenoiseStats()
            assert s["temporal"] == "ran" and s["motion"] is True
            assert np.array_equal(r.captureFrame()["data"], shown[k]), k
    finally:
        r.destroy()


def test_not_ready_while_the_scene_is_newer_than_the_g_buffer(W, gpu_renderer):
    r = gpu_renderer
    r.buildPipeline(4, 1)
    width, height = 33, 9
    d = fu.desc(**D)
    b = skinned(W, r, width, height)
    r.setFrameTemporal(tu.desc(**T))
    b.update(0.0)
    W.sync_world(r, b, width, height)
    r.compute(1)
    r.denoiseFrame(d)
    b.update(0.3)                                      # rt_world_update, and no compute() since
    assert b.deviceResident, b.deviceWarning
    with pytest.raises(W.RendererError, match=r"frame motion: the scene changed since the last compute\(\)"):
        r.denoiseFrame(d)
    assert r.readFrameHistory(frames_only=True) == 1, "a refused call integrates nothing"
    W.sync_world(r, b, width, height)                  # a camera change and an accumulation reset alone do not help ...
    with pytest.raises(W.RendererError, match="frame motion: the scene changed"):
        r.denoiseFrame(d)
    r.compute(2)
    r.denoiseFrame(d)                                  # ... a compute() does
    r.updateSceneUniforms(b.cameraData, 0, b.lightCount)
    r.denoiseFrame(d)                                  # and a camera change alone does not trigger it
    for upload in (lambda: r.updateBuffer("instance", r.worldRead("instances")),
                   lambda: r.updateBuffer("topology", r.worldRead("mesh_topology")),
                   lambda: r.updateCombinedGeometry(r.worldRead("vertices"), r.worldRead("normals"), r.worldRead("uvs")),
                   lambda: r.updateCombinedBVH(r.worldRead("tlas"), r.worldRead("blas"))):
        upload()
        with pytest.raises(W.RendererError, match="frame motion: the scene changed"):
            r.denoiseFrame(d)
        r.compute(3)
        r.denoiseFrame(d)
    # with the flag clear the same call order is the parent's: no refusal
    r.setFrameTemporal(tu.desc(**dict(T, flags=0)))
    r.updateBuffer("instance", r.worldRead("instances"))
    r.denoiseFrame(d)
    b.close()


def test_the_flag_and_the_ids_on_a_context(W, gpu_renderer):
    r = gpu_renderer
    with pytest.raises(W.RendererError, match="frame temporal: RT_FRAME_TEMPORAL_MOTION needs an uploaded scene"):
        r.setFrameTemporal(tu.desc(**T))
    with pytest.raises(W.RendererError, match="frame motion: n must be the instance count"):
        r.setFrameMotionIds([0])
    r.buildPipeline(4, 1)
    b, ids = mu.sequence_a(0, 33, 9)
    W.upload_scene(r, b, 33, 9)
    r.setFrameTemporal(tu.desc(**T))                   # accepted
    r.setFrameTemporal(tu.desc(**dict(T, flags=mu.MOTION)))
    with pytest.raises(W.RendererError, match="frame temporal: unknown flag bit"):
        r.setFrameTemporal(tu.desc(**dict(T, flags=mu.MOTION | 4)))
    with pytest.raises(W.RendererError, match="frame motion: the stage has not run yet"):
        r.readFrameMotion()
    for bad in ([0, 1], [0, 1, 2, 3], [0, 1, 1], [0, 1, 3], [0, 1, 0xffffffff]):
        with pytest.raises(W.RendererError, match="frame motion:"):
            r.setFrameMotionIds(bad)
    r.setFrameMotionIds([2, 0, 1])
    # an upload of instances means the identity again: frame 1 under frame 0's snapshot with NO ids declared is the model's
    # frame with ids = None
    st = mu.History()
    r.compute(1)
    want, _, _, c = mu.call(frame(r), mu.scene_of(b, ids), D, T, st)
    r.setFrameMotionIds(ids)
    r.setFrameTemporal(tu.desc(**T))
    check(r, st, want, c, "first")
    b1, _ = mu.sequence_a(1, 33, 9)
    mu.upload_frame(W, r, b1, np.arange(3, dtype=np.uint32), 33, 9, False)
    r.updateBuffer("instance", b1.instances)           # ... again, after the ids: the identity holds
    r.compute(2)
    want, _, _, c = mu.call(frame(r), mu.scene_of(b1, None), D, T, st)
    check(r, st, want, c, "identity after an upload")
