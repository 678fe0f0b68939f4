"""The dilation model (tests/model/dilate_model.cpp, the brute-force restatement of the dilation rule of include/mi355rt.h)
held to paper: the hand-worked cases of dilate_util.hand_cases with their written-out source maps and tie positions, the
figures of the random patterns the GPU tests use, and the consequences the header states - a second dilation changes nothing,
covered texels and texels without a source keep their words.  No GPU needed."""
import numpy as np
import pytest

import dilate_util as du

CASES = du.hand_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_worked_case(name):
    atlas, radius, want_src, want_ties = CASES[name]
    out, src, filled, tie = du.dilate_model(atlas, radius)
    assert src.tolist() == want_src.tolist(), name
    own = np.arange(src.size, dtype=np.uint32).reshape(src.shape)
    assert filled == int(((src != du.NONE) & (src != own)).sum())
    assert sorted((int(x), int(y)) for y, x in np.argwhere(tie)) == sorted(want_ties), name
    assert np.array_equal(du.words(out), du.apply_source_map(atlas, want_src)), name


def test_the_disc_of_radius_3_has_28_texels():
    atlas, radius, want_src, _ = CASES["disc_r3"]
    assert du.dilate_model(atlas, radius)[2] == 28
    # ... and every one of them lies within 3 texels of the centre, every other texel beyond
    ys, xs = np.mgrid[0:9, 0:9]
    inside = (xs - 4) ** 2 + (ys - 4) ** 2 <= 9
    assert np.array_equal(want_src != du.NONE, inside)


def test_w_values_decide_coverage():
    atlas, radius, _, _ = CASES["w_values"]
    assert du.covered_mask(atlas).tolist() == [[False, True, False, True, False]]   # NaN, -0.0, -1, +inf, -2
    out = du.words(du.dilate_model(atlas, radius)[0])[0]
    before = du.words(atlas)[0]
    assert np.array_equal(out[[1, 3]], before[[1, 3]])                  # covered texels: untouched, -0.0 and +inf stay
    assert out[:, 3].tolist() == [du.MINUS_TWO, 0x80000000, du.MINUS_TWO, 0x7f800000, du.MINUS_TWO]
    assert np.array_equal(out[[0, 2], 0:3], before[[1, 1], 0:3])        # bit for bit, the NaN / denormal colours included
    assert np.array_equal(out[4, 0:3], before[3, 0:3])


@pytest.mark.parametrize("key", sorted(du.PATTERNS))
def test_pattern_figures(key):
    width, height, p, seed, radius = key
    assert du.figures(du.pattern(width, height, p, seed), radius) == du.PATTERNS[key]


@pytest.mark.parametrize("key", sorted(du.PATTERNS))
def test_consequences_of_the_rule(key):
    width, height, p, seed, radius = key
    atlas = du.pattern(width, height, p, seed)
    out, src, filled, _ = du.dilate_model(atlas, radius)
    before, after = du.words(atlas), du.words(out)
    own = np.arange(src.size, dtype=np.uint32).reshape(src.shape)
    got = (src != du.NONE) & (src != own)
    assert np.array_equal(after[~got], before[~got])                    # covered texels and texels without a source
    assert np.array_equal(after, du.apply_source_map(atlas, src))
    assert np.array_equal(src == own, du.covered_mask(atlas))
    # every source is a covered texel within the radius, and no covered texel is nearer
    ys, xs = np.nonzero(got)
    sy, sx = np.divmod(src[got].astype(np.int64), width)
    assert du.covered_mask(atlas)[sy, sx].all()
    d2 = (sx - xs) ** 2 + (sy - ys) ** 2
    assert d2.max() <= radius * radius
    cy, cx = np.nonzero(du.covered_mask(atlas))
    all_d2 = (cx[None, :] - xs[:, None]) ** 2 + (cy[None, :] - ys[:, None]) ** 2
    assert np.array_equal(all_d2.min(axis=1), d2)
    # a texel that stayed has no covered texel within the radius
    uy, ux = np.nonzero(src == du.NONE)
    if len(uy) and len(cy):
        assert ((cx[None, :] - ux[:, None]) ** 2 + (cy[None, :] - uy[:, None]) ** 2).min(axis=1).min() > radius * radius
    # idempotence: filled texels are uncovered and find the same sources
    again, src2, filled2, _ = du.dilate_model(out, radius)
    assert np.array_equal(du.words(again), after) and np.array_equal(src2, src) and filled2 == filled
