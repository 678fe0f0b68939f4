"""Shared pieces of the atlas-dilation tests (rt_dilate_atlas): the reference model (tests/model/dilate_model.cpp, a brute
force over every texel of the disc), built with the flags of oracle/Makefile as bake_util builds its model; the hand-worked
cases with written-out source maps; the random patterns of the GPU tests with the figures they must show; and the numpy
application of a source map, which ties the model's atlas to its own source map."""
import ctypes
import functools
import os

import numpy as np

import model_build
import radiance_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "model", "dilate_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libdilate_model.so")
NONE = 0xffffffff
MINUS_TWO = 0xc0000000            # the bits of -2.0f
NAN, INF = float("nan"), float("inf")


@functools.lru_cache(maxsize=None)
def model_lib():
    L = ctypes.CDLL(model_build.build(SRC, LIB, ru.FLAGS + ["-shared"]))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.dilate_model.argtypes = [vp, u32, u32, u32, vp, vp]
    L.dilate_model.restype = u32
    return L


def dilate_model(atlas, radius):
    """atlas (H, W, 4) f32 -> (dilated copy, source map (H, W) u32, filled count, tie map (H, W) bool: filled texels whose
    smallest d2 more than one covered texel attained)"""
    out = np.array(atlas, dtype=np.float32, order="C")
    assert out.ndim == 3 and out.shape[2] == 4
    H, W = out.shape[:2]
    src = np.empty((H, W), np.uint32)
    tie = np.empty((H, W), np.uint8)
    filled = model_lib().dilate_model(out.ctypes.data, W, H, int(radius), src.ctypes.data, tie.ctypes.data)
    return out, src, int(filled), tie.astype(bool)


def words(a):
    """any 16-byte-texel atlas -> (H, W, 4) u32"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(a.shape[0], a.shape[1], 4)


def covered_mask(atlas):
    with np.errstate(invalid="ignore"):
        return np.asarray(atlas, np.float32)[..., 3] >= 0


def apply_source_map(atlas, src):
    """the result the rule names for a source map, in numpy: -> (H, W, 4) u32"""
    w = words(np.array(atlas, dtype=np.float32, order="C")).copy()
    flat = w.reshape(-1, 4)
    before = flat.copy()
    s = np.asarray(src, np.uint32).reshape(-1)
    filled = (s != NONE) & (s != np.arange(s.size, dtype=np.uint32))
    flat[filled, 0:3] = before[s[filled], 0:3]
    flat[filled, 3] = MINUS_TWO
    return w


def figures(atlas, radius):
    """(covered, filled, ties, unfilled) of the model on a pattern"""
    _, src, filled, tie = dilate_model(atlas, radius)
    covered = int(covered_mask(atlas).sum())
    assert int((src != NONE).sum()) == covered + filled
    return covered, filled, int(tie.sum()), atlas.shape[0] * atlas.shape[1] - covered - filled


def colours(shape, seed):
    """(H, W, 3) u32 of random bit patterns, NaNs (quiet and signalling, both signs), infinities, denormals and both zeros
    among them"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 1 << 32, size=tuple(shape) + (3,), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7fc00000, 0x7f800001, 0xffc12345, 0xff800001, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x0,
                        0x80000000], np.uint32)
    pick = rng.random(c.shape) < 0.2
    c[pick] = special[rng.integers(0, len(special), size=int(pick.sum()))]
    return c


def pattern(width, height, p, seed):
    """The atlas of a random pattern: coverage is np.random.default_rng(seed).random((H, W)) < p; colours() in the first
    three words; w is a non-negative value where covered (0, -0.0, +inf and ordinary ones) and an uncovered one elsewhere
    (-1, -2, NaN, -inf and ordinary negative ones)."""
    cover = np.random.default_rng(seed).random((height, width)) < p
    rng = np.random.default_rng(seed + 1000)
    a = np.empty((height, width, 4), np.uint32)
    a[..., 0:3] = colours((height, width), seed + 2000)
    yes = np.array([0.0, -0.0, INF, 1.0, 0.25, 1e-45], np.float32).view(np.uint32)
    no = np.array([-1.0, -2.0, NAN, -INF, -0.5, -1e-45], np.float32).view(np.uint32)
    k = rng.integers(0, 6, size=(height, width))
    a[..., 3] = np.where(cover, yes[k], no[k])
    a = a.view(np.float32)
    assert np.array_equal(covered_mask(a), cover)
    return a


# (width, height, p, seed, radius) -> (covered, filled, ties, unfilled), from a numpy brute force
PATTERNS = {
    (65, 63, 0.05, 1, 7): (212, 3882, 449, 1),
    (65, 63, 0.05, 1, 2): (212, 1803, 137, 2080),
    (130, 70, 0.002, 2, 24): (20, 8650, 57, 430),     # the disc's edge at full radius
    (65, 63, 0.3, 1, 24): (1240, 2855, 1301, 0),      # dense, tie-heavy
}


def _from_map(rows, legend_extra=None):
    """A hand case from rows of characters: an upper-case letter is a covered texel, its lower-case form a texel it is the
    source of, '.' a texel that stays.  -> (atlas (H, W, 4) f32, expected source map (H, W) u32)"""
    H, W = len(rows), len(rows[0])
    idx = {}
    for y, row in enumerate(rows):
        assert len(row) == W
        for x, ch in enumerate(row):
            if ch.isupper():
                idx[ch.lower()] = y * W + x
    a = np.zeros((H, W, 4), np.float32)
    a[..., 3] = -1.0
    src = np.full((H, W), NONE, np.uint32)
    for y, row in enumerate(rows):
        for x, ch in enumerate(row):
            if ch.isupper():
                i = y * W + x
                a[y, x] = (i + 0.5, -(i + 0.25), 1.0 / (i + 1), 0.5)
                src[y, x] = i
            elif ch != ".":
                src[y, x] = idx[ch]
    return a, src


def hand_cases():
    """name -> (atlas (H, W, 4) f32, radius, expected source map (H, W) u32, expected tie positions [(x, y)] or None)"""
    cases = {}

    def add(name, rows, radius, ties=None):
        a, src = _from_map(rows)
        cases[name] = (a, radius, src, ties)

    # the disc of radius 3: dy = 0 reaches |dx| = 3, |dy| = 1 and 2 reach |dx| = 2 (8, 5 <= 9 - dy^2 < 9), |dy| = 3 only dx = 0
    add("disc_r3", [".........",
                    "....a....",
                    "..aaaaa..",
                    "..aaaaa..",
                    ".aaaAaaa.",
                    "..aaaaa..",
                    "..aaaaa..",
                    "....a....",
                    "........."], 3, [])
    # column 4 is as far from A (index 38) as from B (index 42): the lower index
    add("two_in_a_row", [".........",
                         "..a...b..",
                         "aaaaabbbb",
                         "aaaaabbbb",
                         "aaAaabBbb",
                         "aaaaabbbb",
                         "aaaaabbbb",
                         "..a...b..",
                         "........."], 3, [(4, y) for y in range(2, 7)])
    # A = (3, 1), B = (1, 3): (1, 1), (2, 2) and (3, 3) are as far from both - ties across ROWS - and go to the lower row
    add("diagonal", ["..aaa",
                     ".aaAa",
                     "bbaaa",
                     "bBba.",
                     "bbb.."], 2, [(1, 1), (2, 2), (3, 3)])
    # the corners of 5 x 5 at radius 3: the middle column and row are two-way ties, the centre a four-way one
    add("corners", ["AaabB",
                    "aaabb",
                    "aaabb",
                    "cccdd",
                    "CccdD"], 3, [(2, 0), (2, 1), (0, 2), (1, 2), (2, 2), (3, 2), (4, 2), (2, 3), (2, 4)])
    add("radius_0", ["..A..", ".....", "B...C"], 0, [])
    add("all_covered", ["AB", "CD", "EF"], 5, [])
    add("none_covered", ["....", "....", "...."], 24, [])
    add("1x1_covered", ["A"], 24, [])
    add("1x1_uncovered", ["."], 24, [])
    add("1x9", [".", "a", "a", "a", "A", "a", "a", "a", "."], 3, [])
    add("9x1", [".aaaAaaa."], 3, [])
    # the w values: NaN is uncovered, -0.0 and +inf are covered, -1 and -2 are uncovered; the -1 between them is a tie
    a = np.zeros((1, 5, 4), np.float32)
    a[0, :, 0] = [10, 11, 12, 13, 14]
    a[0, :, 1] = [NAN, -0.0, 1e-40, -INF, 3.0]
    a[0, :, 3] = [NAN, -0.0, -1.0, INF, -2.0]
    cases["w_values"] = (a, 1, np.array([[1, 1, 1, 3, 3]], np.uint32), [(2, 0)])
    return cases
