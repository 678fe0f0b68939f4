"""The encoding rule of include/mi355rt.h "lightmaps" on paper, without a GPU: the numpy restatement (tests/encode_util.py)
on hand-worked texels and on the special inputs; the properties that follow from the rule - the largest byte of a non-zero
word lies in 128 .. 255, a decoder gets every channel back within half a quantisation step, 2^(E - 137); F16 is numpy's
float16 conversion - and then the host build of rt_rgbe8 / rt_f32_to_f16 (include/mi355rt_math.h), the source k_encode_atlas
compiles for the device, against that restatement on the same inputs and on two million random texels.  Also decode_rgbe
and write_hdr of the package."""
import numpy as np

import encode_util as eu


def word(r, g, b, e):
    return r | g << 8 | b << 16 | e << 24


def rgbe_of(*texel):
    return int(eu.encode_rgbe(np.array([texel], np.float32))[0])


def test_hand_worked_texels():
    assert rgbe_of(1, 1, 1, 0.5) == word(128, 128, 128, 129)
    assert rgbe_of(0.5, 0.25, 0, 1) == word(128, 64, 0, 128)
    assert rgbe_of(1, 1, 1, -1) == 0                      # no surface, not filled
    assert rgbe_of(1, 1, 1, -2) == word(128, 128, 128, 129)   # filled: encoded
    assert rgbe_of(3, 1.5, 0.75, 0) == word(192, 96, 48, 130)   # 3 = 0.75 * 2^2: scale 2^6
    assert rgbe_of(255.5, 1, 0.99, 0.3) == word(255, 1, 0, 136)   # floor, not round: 255.5 stays 255, 0.99 is 0
    assert rgbe_of(0, 0, 0, 0.3) == 0
    assert rgbe_of(1, 1, 1, eu.NAN) == word(128, 128, 128, 129)   # a NaN w is not -1


def test_special_inputs():
    lo, at, hi = eu.ulp(2.0 ** -95, -1), 2.0 ** -95, eu.ulp(2.0 ** -95, 1)
    assert rgbe_of(eu.NAN, 1, eu.NAN, 0) == word(0, 128, 0, 129)
    assert rgbe_of(eu.NAN, eu.NAN, eu.NAN, 0) == 0
    assert rgbe_of(eu.INF, 0, 0, 0) == word(255, 0, 0, 255)        # +inf is clamped to the largest colour
    assert rgbe_of(-eu.INF, 1, 0, 0) == word(0, 128, 0, 129)
    assert rgbe_of(-0.0, -3.0, 2, 0) == word(0, 0, 128, 130)
    assert rgbe_of(1e-40, 1e-40, 1e-40, 0) == 0                    # all denormal: b = 0
    assert rgbe_of(1e-40, 1, 0, 0) == word(0, 128, 0, 129)         # a denormal beside a normal: its byte is 0
    assert rgbe_of(lo, 0, 0, 0) == 0                               # v < 2^-95
    assert rgbe_of(at, 0, 0, 0) == word(128, 0, 0, 34)             # b = 32, E = 34
    assert rgbe_of(hi, at, lo, 0) == word(128, 128, 127, 34)
    assert rgbe_of(eu.TOP, eu.TOP / 2, 1, 0) == word(255, 127, 0, 255)   # b = 253: the scale is 2^-119
    assert rgbe_of(3.0e38, 0, 0, 0) == word(255, 0, 0, 255)        # above the largest colour (b = 254): clamped
    assert rgbe_of(2.0 ** -126, 0, 0, 0) == 0


def test_largest_byte_and_decode_bound():
    a = np.empty((200000, 4), np.float32)
    a[:, 0:3] = eu.random_colours(len(a), 11)
    a[:, 3] = 0.3
    a[::7, 0] = 0.0
    a[::11, 1] = -a[::11, 1]
    w = eu.encode_rgbe(a)
    assert (w != 0).all()
    assert len(np.unique(w >> 24)) >= 55, "the colours span the binades"
    top = np.max(np.stack([(w >> s) & 0xff for s in (0, 8, 16)]), axis=0)
    assert top.min() >= 128 and top.max() <= 255
    e = (w >> 24).astype(np.float64)
    err = np.abs(eu.decode_rgbe(w) - eu.sanitise(a))
    assert (err <= np.exp2(e - 137)[:, None]).all()
    assert (err.max(axis=1) > np.exp2(e - 139)).mean() > 0.5, "the bound is not idle"


def test_package_decoder_and_hdr_file(W, tmp_path):
    a = eu.special_atlas(17, 33, 5)
    w = eu.encode_rgbe(a).reshape(33, 17)
    assert (w == 0).any() and (w != 0).any()
    assert np.array_equal(W.decode_rgbe(w).reshape(-1, 3), eu.decode_rgbe(w.reshape(-1)))
    path = str(tmp_path / "atlas.hdr")
    W.write_hdr(path, w)
    # a reader of flat Radiance files, written here: header lines up to the empty one, the resolution, 4 bytes per pixel
    blob = open(path, "rb").read()
    head, _, rest = blob.partition(b"\n\n")
    lines = head.split(b"\n")
    assert lines[0] == b"#?RADIANCE" and b"FORMAT=32-bit_rle_rgbe" in lines[1:]
    res, _, pixels = rest.partition(b"\n")
    sy, h, sx, width = res.split()
    assert (sy, sx) == (b"-Y", b"+X") and (int(h), int(width)) == (33, 17)
    assert len(pixels) == 33 * 17 * 4
    px = np.frombuffer(pixels, np.uint8).reshape(33, 17, 4).astype(np.uint32)
    assert np.array_equal(px[:, :, 0] | px[:, :, 1] << 8 | px[:, :, 2] << 16 | px[:, :, 3] << 24, w)


def test_f16_is_numpys_conversion_on_finite_values():
    v = np.concatenate([eu.random_colours(100000, 3, binades=80).reshape(-1), -eu.random_colours(1000, 4).reshape(-1),
                        np.array([s for s in eu.SPECIAL if np.isfinite(s)] + [-1.0, -2.0, 0.3], np.float32)])
    with np.errstate(over="ignore"):
        want = v.astype(np.float16)
    assert np.isinf(want).any() and (want == 0).any() and ((np.abs(want) < 2.0 ** -14) & (want != 0)).any()
    assert np.array_equal(eu.host_f16(v), want.view(np.uint16))
    got = eu.host_f16(np.array([-1.0, -2.0], np.float32)).view(np.float16)
    assert got.tolist() == [-1.0, -2.0]                   # coverage survives
    a = eu.special_atlas(9, 7, 2)
    assert eu.same_f16(eu.host_f16(a), eu.encode_f16(a))
    assert eu.f16_is_nan(eu.host_f16(np.array([eu.NAN], np.float32))).all()


def test_the_host_build_of_the_device_function_is_the_rule():
    for size, seed in (((1, 1), 1), ((17, 33), 2), ((64, 5), 3), ((200, 100), 4)):
        a = eu.special_atlas(size[0], size[1], seed)
        assert np.array_equal(eu.host_rgbe(a), eu.encode_rgbe(a)), size
    rng = np.random.default_rng(9)
    bits = rng.integers(0, 1 << 32, (2000000, 4), dtype=np.uint64).astype(np.uint32)   # every class of float, NaNs included
    a = bits.view(np.float32)
    a[::3, 3] = -1.0
    got, want = eu.host_rgbe(a), eu.encode_rgbe(a)
    assert (want == 0).sum() > 1000 and (want != 0).sum() > 1000
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
