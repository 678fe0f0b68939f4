"""The CPU oracle's post pass against tests/post_model.py, an independent float64 statement of PostProcess.wgsl, on
structured images: HDR noise, fireflies and holes, step edges, a one-pixel checker, a ramp, and edges / bright pixels on
the 16-pixel tile seams.  (tests/test_post_kat.py feeds uniform images, on which every filter is the identity.)

For each shape and frame count all images are presented one after another on ONE renderer; the model is fed the history
the oracle wrote the time before, so the ping-pong and a history far from the new image are both exercised.  The
conditions are those of post_model.check().  Worst values measured on the CPU oracle over the 36 (shape, frame count)
sequences, 218 compared presents (`pytest -s` prints them):

    well-conditioned pixels   RGBA8: 3 presents with ONE differing component each, by 1 code value, the byte 0.5002 from
                              the unrounded model value at most ((47, 31): `lognormal` at 1 and 5 frames, 0.02 % of the
                              components; `seams` at 5 frames, 0.11 %); the other 215 presents 0 differing bytes;
                              history 0.60 f16 ulp
    flagged, <= 16 frames     RGBA8 0 code values, history 1.00 f16 ulp (0.9955: the 1 x 1 image; 0.92 elsewhere);
                              up to 100 % of the pixels of a flat image
    flagged, > 16 frames      left out: 0 % of the pixels in every case that is run (cap 2 %)
    `seams` (<= 16 frames)    1 differing byte in all (above); history 0.50 ulp well conditioned, 0.92 ulp flagged
    (47, 31)                  3 differing bytes in all (above); history 0.52 ulp well conditioned, 0.92 ulp flagged

The 17 one-token mutants of the oracle's post pass that this file was written to catch (firefly threshold, headroom,
centre in the neighbour maximum, jitter sign, either `> 16`, either filter denominator, k, first-frame alpha, 1 / (n + 1),
sharpening sign and operand order, gamma, history side, border wrap, `a < 0`) each fail it; 14 of them pass
tests/test_post_kat.py.
"""
import numpy as np
import pytest

import parity_util as pu
import post_model as pm

_stats = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_stats):
        print("post model, worst %s: %.4f" % (k, _stats[k]))


def oracle_at(W, oracle_lib, w, h, frame_count):
    """An oracle renderer with the host state (frame_count, average jitter) as after `frame_count` dispatches."""
    r = oracle_lib.OracleRenderer()
    r.buildPipeline(2, 1)
    W.upload_scene(r, pu.bridge_for(W, "cornell"), w, h)
    r.compute(1)
    if frame_count > 1:
        r.compute(frame_count)
    return r


@pytest.mark.parametrize("frame_count", pm.FRAME_COUNTS)
@pytest.mark.parametrize("w,h", pm.SHAPES)
def test_oracle_post_pass_equals_the_float64_model(W, oracle_lib, w, h, frame_count):
    r = oracle_at(W, oracle_lib, w, h, frame_count)
    jitter = pm.average_jitter(r.readUniforms())
    assert np.isfinite(jitter).all() and (np.abs(jitter * np.array([w, h])) <= 0.5).all()
    compared = 0
    for image in pm.IMAGES:
        acc = pm.accum(image, w, h, frame_count)
        before = pm.widen_history(r.readHistory())       # what this present() reads
        r.writeAccum(acc)
        r.present()
        if not pm.runs_against_model(image, w, h, frame_count):
            continue                                     # presented all the same: the next image blends with it
        m = pm.model(acc, before, frame_count, jitter)
        pm.check(m, r.captureFrame()["data"], r.readHistory(), frame_count,
                 "%dx%d, %d frames, %s" % (w, h, frame_count, image), _stats)
        compared += 1
    assert compared == (len(pm.IMAGES) if frame_count <= 16 else 0 if w * h == 1 else len(pm.IMAGES) - len(pm.FLAT_IMAGES))


def test_clean_value_outside_the_image_is_not_the_clamped_coordinates():
    """get_radiance_clean(-1, y) looks at columns -2..0, each clamped on its own: all of them are column 0, which is not
    the neighbourhood of clean(0, y) (columns 0 and 1).  The two differ where the radiance is negative (the firefly bound
    3 * max + 0.1 drops below zero), so a model that pads the clean image instead of gathering gets the border wrong on
    such input; this pins that post_model gathers."""
    w, h = 6, 5
    acc = np.ones((h, w, 4), dtype=np.float32)
    acc[..., :3] = 0.5
    acc[:, 0, :3] = -1.0
    m = pm.model(acc, np.zeros((h, w, 4)), 17, (0.0, 0.0))
    # clean(-1, y) = min(max(-1, 0), 3 * -1 + 0.1) = -2.9; clean(0, y) = min(max(-1, 0), 3 * 0.5 + 0.1) = 0; clean(1, y) = 0.5
    assert abs(m["mean"][2, 0, 0] - (3 * -2.9 + 3 * 0.0 + 3 * 0.5) / 9.0) < 1e-12
