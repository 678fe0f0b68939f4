"""k_postprocess alone, on what the path tracer never hands it.

The accumulation buffer is an input of the C ABI (rt_write_accum, rt_bind_accum, rt_bind_present_source, the gathered
stripes of other ranks), so the kernel is presented structured images (tests/post_model.py) and `specials`: NaN, +-inf,
weights of NaN / -0 / -1 / inf, denormals, FLT_MAX and the f16 overflow / subnormal boundaries, at image corners, on the
16-pixel seams of the LDS tiles, on the last row / column and inside a tile.  One context per (shape, frame count); both
sides get the host state from compute(), the same array through writeAccum, then present(); all images follow one another
on the same context, so a history holding inf / NaN is read back, clamped and blended.  After every present RGBA8, history
and uniform block must equal the CPU oracle's BIT FOR BIT, with two masks on the f16 history:

  * +0 / -0 are the same value (as in parity_util.assert_parity);
  * NaNs are compared as a class: WGSL gives a NaN no payload, and the sign of a NaN that an operation generates
    (inf - inf, 0 * inf, 0 / 0) is a property of the machine (x86 SSE produces the negative quiet NaN, f32 0xffc00000,
    f16 0xfe00).  A NaN on one side and a number on the other is a failure.  The patterns each side produced, and how
    many components were NaN on both sides with different bits, are printed at the end of the module (`pytest -s`).

On the images without special values the kernel is also compared with the float64 model directly, under the conditions
of post_model.check(), so the device result does not lean on the oracle alone.  Frame count 0 is the recorder's warm-up
(non-finite average jitter, alpha = 1 / 0: the direct path instead of the LDS tiles); the model does not cover it.

These inputs are data, never addresses: every coordinate is clamped to the image and pp_texel saturates.

Measured on an MI355X (this file alone: 62 tests in 13 s, of which 12 s are the torch start-up of the last test; run it
under `timeout 120`): every present bit-identical to the oracle under the two masks, no fix to the kernel or to the host
branch of include/mi355rt_math.h was needed.  Both f16 NaN patterns, 0x7e00 and 0xfe00, occur in the device's history and in the
oracle's.  The kernel against the model: 1 code value at most, 0.12 % of
a present's components differing at worst, the differing byte 0.5003 from the unrounded model value; history 0.61 f16 ulp
well conditioned, 0.92 ulp flagged; 0 % of the pixels left out beyond 16 frames.
"""
import numpy as np
import pytest

import parity_util as pu
import post_model as pm

pytestmark = pytest.mark.gpu

SHAPES = pm.SHAPES + [(15, 15), (17, 17), (257, 3), (64, 48)]
FRAME_COUNTS = [0, 1, 2, 16, 17, 64]

_stats = {}
_nan_bits = {"gpu": set(), "oracle": set()}
_nan_count = {"both": 0, "bits differ": 0}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_stats):
        print("gpu post vs model, worst %s: %.4f" % (k, _stats[k]))
    for side in ("gpu", "oracle"):
        print("f16 NaN patterns in the %s history: %s" % (side, sorted("0x%04x" % b for b in _nan_bits[side])))
    print("history components NaN on both sides: %d, of which with different bits: %d" % (_nan_count["both"], _nan_count["bits differ"]))


def _is_nan16(h):
    return (h & 0x7fff) > 0x7c00


def assert_history_equal(gh, ch, what):
    for side, h in (("gpu", gh), ("oracle", ch)):
        _nan_bits[side].update(int(b) for b in np.unique(h[_is_nan16(h)]))
    both = _is_nan16(gh) & _is_nan16(ch)
    _nan_count["both"] += int(both.sum())
    _nan_count["bits differ"] += int((gh[both] != ch[both]).sum())
    gz, cz = gh.copy(), ch.copy()
    gz[gz == 0x8000] = 0                  # +0 / -0 are the same value
    cz[cz == 0x8000] = 0
    gz[_is_nan16(gz)] = 0x7e00            # NaN is a class (sign and payload are the machine's, see the module docstring)
    cz[_is_nan16(cz)] = 0x7e00
    assert np.array_equal(gz, cz), pu.describe_mismatch(what + ": history (rgba16f)", gh, ch)


def assert_post_parity(gpu, cpu, what):
    go, co = gpu.captureFrame()["data"], cpu.captureFrame()["data"]
    assert np.array_equal(go, co), pu.describe_mismatch(what + ": RGBA8 output", go, co)
    assert_history_equal(gpu.readHistory(), cpu.readHistory(), what)
    assert np.array_equal(gpu.readUniforms(), cpu.readUniforms()), what + ": uniform block differs"


def set_host_state(W, r, w, h, frame_count, upload=True):
    """frame_count and average jitter as after `frame_count` dispatches (0: the warm-up dispatch alone)."""
    if upload:
        r.buildPipeline(2, 1)
        W.upload_scene(r, pu.bridge_for(W, "cornell"), w, h)
    if frame_count == 0:
        r.compute(0)
    else:
        r.compute(1)
        if frame_count > 1:
            r.compute(frame_count)


def present_both(gpu, cpu, acc):
    for r in (gpu, cpu):
        r.writeAccum(acc)
        r.present()
    gpu.sync()


@pytest.mark.parametrize("frame_count", FRAME_COUNTS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_post_pass_equals_oracle_and_model(W, oracle_lib, gpu_renderer, w, h, frame_count):
    gpu, cpu = gpu_renderer, oracle_lib.OracleRenderer()
    for r in (gpu, cpu):
        set_host_state(W, r, w, h, frame_count)
    jitter = pm.average_jitter(gpu.readUniforms())
    assert np.isfinite(jitter).all() == (frame_count > 0)
    sequence = [(name, pm.accum(name, w, h, frame_count)) for name in pm.IMAGES]
    special = pm.specials(w, h, frame_count)
    sequence += [("specials", special), ("specials again", special), ("lognormal after specials", sequence[0][1])]
    for name, acc in sequence:
        what = "%dx%d, %d frames, %s" % (w, h, frame_count, name)
        before = pm.widen_history(gpu.readHistory())
        present_both(gpu, cpu, acc)
        assert_post_parity(gpu, cpu, what)
        if name in pm.IMAGES and frame_count >= 1 and pm.runs_against_model(name, w, h, frame_count):
            m = pm.model(acc, before, frame_count, jitter)
            pm.check(m, gpu.captureFrame()["data"], gpu.readHistory(), frame_count, what + " (kernel against the model)", _stats)


def test_resize_between_presents_starts_from_a_zero_history(W, oracle_lib, gpu_renderer):
    """updateScreenSize on a live context recreates both history textures zero-filled: the first present at the new size
    must equal the model fed a ZERO history, on both sides, whatever the old history held."""
    gpu, cpu = gpu_renderer, oracle_lib.OracleRenderer()
    w, h, n = 23, 17, 2
    for r in (gpu, cpu):
        set_host_state(W, r, w, h, n)
    for name in ("lognormal", "checker", "fireflies_holes"):      # an odd number: the ping-pong index is left at 1
        present_both(gpu, cpu, pm.accum(name, w, h, n))
        assert_post_parity(gpu, cpu, "before the resize, " + name)
    w, h = 64, 48
    b = pu.bridge_for(W, "cornell")
    b.updateCamera(w, h)
    for r in (gpu, cpu):
        r.updateScreenSize(w, h)
        r.updateSceneUniforms(b.cameraData, 0, b.lightCount)
        r.resetAccumulation()
        set_host_state(W, r, w, h, n, upload=False)
        assert not r.readHistory().any()
    jitter = pm.average_jitter(gpu.readUniforms())
    for i, name in enumerate(("fireflies_holes", "ramp")):
        acc = pm.accum(name, w, h, n)
        before = pm.widen_history(gpu.readHistory()) if i else np.zeros((h, w, 4))
        present_both(gpu, cpu, acc)
        what = "after the resize, " + name
        assert_post_parity(gpu, cpu, what)
        for r in (gpu, cpu):
            pm.check(pm.model(acc, before, n, jitter), r.captureFrame()["data"], r.readHistory(), n, what, _stats)


def test_present_source_tensor_equals_the_accumulator(W, oracle_lib):
    """`specials` presented through bindPresentSource from a torch tensor == the same array presented from the
    accumulation buffer (same device: every bit, NaNs included), and == the oracle under the two masks."""
    import torch
    W._build.build_rt()
    w, h, n = 47, 31, 5
    bound, plain, cpu = W.WebGPURenderer(0), W.WebGPURenderer(0), oracle_lib.OracleRenderer()
    try:
        for r in (bound, plain, cpu):
            set_host_state(W, r, w, h, n)
        special = pm.specials(w, h, n)
        t = torch.from_numpy(special).to("cuda:0").contiguous()
        torch.cuda.synchronize()
        bound.writeAccum(pm.accum("checker", w, h, n))            # what present() must NOT read
        bound.bindPresentSource(t.data_ptr())
        for i in range(2):
            bound.present()
            bound.sync()
            present_both(plain, cpu, special)
            what = "present %d from the bound tensor" % i
            assert np.array_equal(bound.captureFrame()["data"], plain.captureFrame()["data"]), what + ": RGBA8"
            assert np.array_equal(bound.readHistory(), plain.readHistory()), what + ": history"
            assert_post_parity(bound, cpu, what)
        bound.bindPresentSource(0)
        assert np.array_equal(pu.bits(bound.readAccum()), pu.bits(pm.accum("checker", w, h, n)))
    finally:
        bound.destroy()
        plain.destroy()
