"""The denoise model (tests/model/denoise_model.cpp, the plain-loop restatement of the denoise rule of include/mi355rt.h) held
to paper: the hand-worked cases of denoise_util.hand_cases with their written-out answers, the six tap counts of the named
patterns against a numpy restatement, the composition identity, and the figure the filter exists for - a 4 spp bake of cornell
is more than twice as near a 512 spp one after three passes.  No GPU needed."""
import numpy as np
import pytest

import bake_util as bu
import denoise_util as du
import parity_util as pu

CASES = du.hand_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_worked_case(name):
    atlas, points, texels, kw, want = CASES[name]
    out, _ = du.denoise_model(atlas, points, texels, **kw)
    assert du.words(out).tolist() == du.words(want).tolist(), (name, out[..., 0], want[..., 0])


def test_no_colour_crosses_the_edge_between_floor_and_wall():
    """the floor-and-wall case with a random colour per texel: every floor texel stays within the floor's range"""
    atlas, points, texels, kw, _ = CASES["floor_and_wall"]
    rng = np.random.default_rng(5)
    atlas = atlas.copy()
    atlas[:, :4] = rng.uniform(0.0, 1.0, (5, 4, 4))
    atlas[:, 4:] = rng.uniform(10.0, 11.0, (5, 4, 4))
    out, counts = du.denoise_model(atlas, points, texels, **kw)
    assert all(c[3] > 0 and c[0] > 0 for c in counts), counts       # the normal stop worked, and taps were accepted
    assert out[:, :4].max() <= 1.0 and out[:, 4:].min() >= 10.0
    assert not np.array_equal(out, atlas)


@pytest.mark.parametrize("key", sorted(du.PATTERNS))
def test_pattern_counts(key):
    width, height, p, seed, step = key
    atlas, points, texels = du.two_walls(width, height, p, seed)
    _, counts = du.model_pass(atlas, points, texels, step, **du.PARAMS)
    print(key, dict(zip(du.COUNTS, counts)))
    assert counts == du.PATTERNS[key]
    assert counts == du.numpy_counts(atlas, points, texels, step, **du.PARAMS)
    assert min(counts) > 0
    assert sum(counts) == 24 * len(texels)


def test_a_call_is_the_composition_of_its_passes():
    atlas, points, texels = du.two_walls(37, 21, 0.6, 3)
    a = atlas
    for step in (1, 2, 4):
        a, _ = du.model_pass(a, points, texels, step, **du.PARAMS)
    whole, counts = du.denoise_model(atlas, points, texels, passes=3, step=1, **du.PARAMS)
    assert np.array_equal(du.words(whole), du.words(a)) and len(counts) == 3
    two, _ = du.denoise_model(atlas, points, texels, passes=2, step=2, **du.PARAMS)
    b = du.model_pass(du.model_pass(atlas, points, texels, 2, **du.PARAMS)[0], points, texels, 4, **du.PARAMS)[0]
    assert np.array_equal(du.words(two), du.words(b))
    assert not np.array_equal(du.words(whole), du.words(two))


def test_without_points_the_atlas_is_copied():
    atlas = du.special_values(du.two_walls(9, 7, 1.0, 2)[0], 3)
    out, counts = du.denoise_model(atlas, np.zeros((0, 8), np.float32), np.zeros(0, np.uint32), **du.PARAMS)
    assert np.array_equal(du.words(out), du.words(atlas)) and counts == [(0,) * 6] * 3


def test_a_noisy_bake_of_cornell_comes_nearer_the_converged_one(W):
    """cornell under grid_uv at 64 x 64, depth 2: 4 spp at bu.SEED against 512 spp at seed 99; normal_cos 0.9, plane_eps
    0.02, max_dist 0.5, three passes.  The denoised rgb RMSE over the covered texels must be below half the raw one (a numpy
    restatement of the rule gave 0.26 of it; the rule is deterministic, so half leaves a factor of two)."""
    b = pu.bridge_for(W, "cornell")
    m = bu.model_for(W, b)
    uv = bu.grid_uv(b, 0)
    noisy, points, texels, _ = m.bakeIrradiance(0, 64, 64, 2, 4, bu.SEED, atlas_uv=uv)
    ref = m.bakeIrradiance(0, 64, 64, 2, 512, 99, atlas_uv=uv)[0]
    out, counts = du.denoise_model(noisy, points, texels, normal_cos=0.9, plane_eps=0.02, max_dist=0.5, passes=3)
    covered = np.zeros(64 * 64, bool)
    covered[texels] = True
    covered = covered.reshape(64, 64)

    def rmse(a):
        return float(np.sqrt(np.mean((a[covered][:, 0:3].astype(np.float64) - ref[covered][:, 0:3]) ** 2)))

    raw, den = rmse(noisy), rmse(out)
    print("covered", len(texels), "raw rmse", raw, "denoised rmse", den, "ratio", den / raw, "counts", counts)
    assert len(texels) == 1193
    assert all(min(c) > 0 for c in counts), counts          # every way a tap can be decided occurred in every pass
    assert den < 0.5 * raw, (raw, den)
    assert np.array_equal(du.words(out)[~covered], du.words(noisy)[~covered])
