"""The known answer of the texture fetch (tests/texture_fetch_util.py, tests/test_texture_fetch_kat.py) on the GPU: the
radiance query of k_radiance_query on one tiny textured triangle per sample point, against the float64 statement of WebGPU's
textureSampleLevel within the tolerance derived there, and against the radiance model bit for bit; with the scene's records in
LDS and behind the L1 (MI355RT_NO_LDS_STAGING=1)."""
import numpy as np
import pytest

import radiance_util as ru
import texture_fetch_util as tf

pytestmark = pytest.mark.gpu

_made = []


def _answers(W):
    """(samples, scenes, reference, tolerance, the model's records per scene), made once and left unchanged"""
    if not _made:
        tex = tf.make_textures()
        uv, word, slot = tf.sample_points()
        want, _, _ = tf.reference(tex, uv, word)
        tol = tf.tolerance(tex, uv, word)
        scenes = tf.scenes(tex)
        model = []
        for b, rays, sl in scenes:
            out, counts = ru.model_for(W, b).traceRadiance(rays, 1, 1, ru.SEED)
            model.append((out, counts))
        for a in (want, tol) + tuple(x for pair in model for x in pair):
            a.setflags(write=False)
        _made.append(((uv, word, slot), scenes, want, tol, model))
    return _made[0]


@pytest.mark.parametrize("no_lds", [None, "1"])
def test_the_kernel_fetches_what_the_specification_says(W, monkeypatch, no_lds):
    (uv, word, slot), scenes, want, tol, model = _answers(W)
    if no_lds is None:
        monkeypatch.delenv("MI355RT_NO_LDS_STAGING", raising=False)
    else:
        monkeypatch.setenv("MI355RT_NO_LDS_STAGING", no_lds)
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    worst = 0.0
    try:
        for (b, rays, sl), (ref, counts) in zip(scenes, model):
            tag = "no_lds=%s samples %d.." % (no_lds, sl.start)
            W.upload_scene(r, b, 16, 16)
            res, st = r.traceRadiance(rays, 1, 1, ru.SEED, stats=True)
            assert st["lds"] == (1 if no_lds is None else 0), (tag, st)
            err = np.abs(res["rgb"].astype(np.float64) - want[sl])
            worst = max(worst, float((err / np.maximum(tol[sl], 1e-30)).max()))
            print(tag, "largest error / tolerance so far %.3f" % worst)
            bad = np.argwhere(err > tol[sl])
            assert bad.size == 0, (tag, len(bad), bad[:4].tolist(), res["rgb"][bad[:4, 0]].tolist(), want[sl][bad[:4, 0]].tolist(),
                                   uv[sl][bad[:4, 0]].tolist(), word[sl][bad[:4, 0]].tolist())
            ru.check_against_model(res, ref, tag)
            ru.check_counts(st, counts, rays.shape[0], 1, tag)
            plain = r.traceRadiance(rays, 1, 1, ru.SEED)
            assert np.array_equal(ru.result_words(plain), ru.result_words(res)), (tag, "counting and product kernel differ")
    finally:
        r.destroy()
