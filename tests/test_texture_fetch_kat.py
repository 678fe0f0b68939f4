"""A known answer for the texture fetch (sample_tex), on the CPU: the radiance model's radiance query on the scenes of
tests/texture_fetch_util.py against a float64 statement of WebGPU's textureSampleLevel written from the specification, within
the tolerance derived in that module's docstring.  Kernel and oracle share one restated sample_tex, so a convention error in
it would pass every GPU-against-oracle test; here it cannot.  The last test shows that the comparison has teeth: the
reference recomputed with each listed convention error leaves the tolerance on a tenth of the samples at least."""
import numpy as np
import pytest

import radiance_util as ru
import texture_fetch_util as tf


@pytest.fixture(scope="module")
def textures():
    tex = tf.make_textures()
    tex.setflags(write=False)
    return tex


@pytest.fixture(scope="module")
def samples():
    return tf.sample_points()


def test_the_textures_are_what_the_tolerance_assumes(textures):
    t = textures.astype(np.int64)
    for l in range(tf.LAYERS):
        dx = np.abs(np.roll(t[l, :, :, 0], -1, axis=1) - t[l, :, :, 0])        # includes the wrap edge
        dy = np.abs(np.roll(t[l, :, :, 1], -1, axis=0) - t[l, :, :, 1])
        assert 1 <= dx.min() and dx.max() <= 8 and 1 <= dy.min() and dy.max() <= 8
        assert not np.array_equal(t[l, :, :, 2], t[l, :, :, 2].T)
        assert (t[l, :, :, 2] // 40 == l).all()
    assert not np.array_equal(t[0], t[1]) and not np.array_equal(t[1], t[2])


def test_the_sample_points_are_where_a_fetch_goes_wrong(textures, samples):
    uv, word, slot = samples
    _, i0, layer = tf.reference(textures, uv, word)
    p = uv.astype(np.float64) * tf.N - 0.5
    frac = p - np.floor(p)
    for axis in (0, 1):
        assert (frac[:, axis] == 0.0).any() and (frac[:, axis] == 0.5).any()          # texel centres and texel borders
        assert ((i0[:, axis] == -1)).any() and ((i0[:, axis] == tf.N - 1)).any()      # x0 = 1023, x1 = 0 from both sides
        assert (uv[:, axis] == np.float32(-1.25)).any() and (uv[:, axis] == np.float32(2.5)).any()
    assert (uv[:, 0] != uv[:, 1]).all()
    assert set(np.float32(tf.WORDS).tolist()) <= set(word[slot == 0].tolist())
    assert sorted(set(layer.tolist())) == [-1, 0, 1, 2]
    assert tf.decode_layer([3.0, 0.7, 1.999, -0.4, -0.5, -0.4999, float("nan")]).tolist() == [2, 0, 1, 0, -1, 0, -1]
    assert {0, 3} == set(slot.tolist())
    tol = tf.tolerance(textures, uv, word)
    print("tolerance: largest %.3g, median of the textured samples %.3g" % (tol.max(), np.median(tol[layer >= 0])))
    assert tol.max() <= 2e-4                                                           # what the derivation promises


def test_the_model_fetches_what_the_specification_says(W, textures, samples):
    uv, word, slot = samples
    want, _, _ = tf.reference(textures, uv, word)
    tol = tf.tolerance(textures, uv, word)
    worst = 0.0
    for b, rays, sl in tf.scenes(textures):
        assert b.lightCount == 2 and len(b.tlas) // 8 == 1
        m = ru.model_for(W, b)
        out, counts = m.traceRadiance(rays, 1, 1, ru.SEED)
        assert (np.abs(out[:, 3] - 1.0) < 1e-5).all(), "every ray hits its triangle, at t = 1"
        assert (counts[:, 2] == 1).all()
        err = np.abs(out[:, :3].astype(np.float64) - want[sl])
        worst = max(worst, float((err / np.maximum(tol[sl], 1e-30)).max()))
        bad = np.argwhere(err > tol[sl])
        assert bad.size == 0, (len(bad), bad[:4].tolist(), out[bad[:4, 0], :3].tolist(), want[sl][bad[:4, 0]].tolist(),
                               uv[sl][bad[:4, 0]].tolist(), word[sl][bad[:4, 0]].tolist())
    print("largest error / tolerance %.3f" % worst)


@pytest.mark.parametrize("error", tf.ERRORS)
def test_the_tolerance_tells_every_convention_error(textures, samples, error):
    uv, word, slot = samples
    right, _, _ = tf.reference(textures, uv, word)
    wrong, _, _ = tf.reference(textures, uv, word, error=error)
    tol = tf.tolerance(textures, uv, word)
    caught = (np.abs(wrong - right) > tol).any(axis=1)
    print(error, "caught on %d of %d samples" % (caught.sum(), len(uv)))
    assert 10 * caught.sum() >= len(uv), (error, int(caught.sum()), len(uv))
