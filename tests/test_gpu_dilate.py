"""Atlas dilation on the GPU (rt_dilate_atlas / rt_dilate_atlas_device, csrc/k_dilate.hip.h) against the reference model
(tests/model/dilate_model.cpp, held to paper by tests/test_dilate_model.py), word for word: atlas bits, source map and count.

The atlas sizes are the smallest at which the kernels can go wrong: 1 x 1, one column and one row of 9, 7 x 5 (one partial 16
x 16 tile, one partial bitmap word), 65 x 63 (a second bitmap word of one bit, a fifth tile column of one texel, a partial
last tile row) and 130 x 70 (three bitmap words per row, nine tile columns; at radius 24 every window hangs over a border).
The radii are 0, 1, 2, 7 and the limit 24.  Colours are random bit patterns with NaNs, infinities and denormals among them.

Parity must not pass on emptiness: the figures of every named pattern (covered, filled, ties, unfilled) are asserted on the
model before the GPU is asked."""
import ctypes

import numpy as np
import pytest

import bake_util as bu
import dilate_util as du
import parity_util as pu

pytestmark = pytest.mark.gpu

RT_ERR_INVALID = -1
SIZES = ((1, 1), (1, 9), (9, 1), (7, 5), (65, 63), (130, 70))
RADII = (0, 1, 2, 7, 24)


@pytest.fixture(scope="module")
def r(W):
    """a context without a scene: dilation needs none"""
    W._build.build_rt()
    ctx = W.WebGPURenderer(0)
    yield ctx
    ctx.destroy()


def check(r, atlas, radius, tag, want=None):
    """the GPU's atlas, source map and count against the model's; -> the model's result"""
    want = want or du.dilate_model(atlas, radius)
    out, src, filled = r.dilateAtlas(atlas, radius, src=True, filled=True)
    assert out is not atlas and out.shape == atlas.shape
    assert np.array_equal(src, want[1]), (tag, "source maps differ at", np.argwhere(src != want[1])[:8].tolist())
    assert filled == want[2], (tag, filled, want[2])
    bad = (du.words(out) != du.words(want[0])).any(axis=2)
    assert not bad.any(), (tag, "texels differ at", np.argwhere(bad)[:8].tolist())
    return want


@pytest.mark.parametrize("width,height", SIZES)
def test_bit_parity_with_the_model(r, width, height):
    seen = 0
    for radius in RADII:
        for p in (0.002, 0.05, 0.3, 0.9):
            atlas = du.pattern(width, height, p, 7)
            seen += check(r, atlas, radius, "%dx%d R=%d p=%g" % (width, height, radius, p))[2]
    if width * height > 1:
        assert seen > 0, "nothing was filled at this size"


@pytest.mark.parametrize("key", sorted(du.PATTERNS))
def test_named_patterns(r, key):
    width, height, p, seed, radius = key
    atlas = du.pattern(width, height, p, seed)
    want = du.dilate_model(atlas, radius)
    covered = int(du.covered_mask(atlas).sum())
    figures = (covered, want[2], int(want[3].sum()), width * height - covered - want[2])
    print(key, figures)
    assert figures == du.PATTERNS[key]
    check(r, atlas, radius, str(key), want)
    # with neither optional output
    plain = r.dilateAtlas(atlas, radius)
    assert np.array_equal(du.words(plain), du.words(want[0]))


def test_hand_worked_cases(r):
    for name, (atlas, radius, want_src, _) in sorted(du.hand_cases().items()):
        out, src, filled = r.dilateAtlas(atlas, radius, src=True, filled=True)
        assert src.tolist() == want_src.tolist(), name
        own = np.arange(src.size, dtype=np.uint32).reshape(src.shape)
        assert filled == int(((src != du.NONE) & (src != own)).sum()), name
        assert np.array_equal(du.words(out), du.apply_source_map(atlas, want_src)), name
        check(r, atlas, radius, name)


def test_a_second_dilation_changes_nothing(r):
    for key in sorted(du.PATTERNS):
        width, height, p, seed, radius = key
        once, src, filled = r.dilateAtlas(du.pattern(width, height, p, seed), radius, src=True, filled=True)
        twice, src2, filled2 = r.dilateAtlas(once, radius, src=True, filled=True)
        assert np.array_equal(du.words(twice), du.words(once)), key
        assert np.array_equal(src2, src) and filled2 == filled == du.PATTERNS[key][1], key


def test_in_place_on_the_device_on_a_torch_side_stream(W):
    import torch
    width, height, p, seed, radius = 130, 70, 0.002, 2, 24
    atlas = du.pattern(width, height, p, seed)
    want = du.dilate_model(atlas, radius)
    assert want[2] == du.PATTERNS[(width, height, p, seed, radius)][1]
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    try:
        side = torch.cuda.Stream()
        r.setStream(side.cuda_stream)
        bits = torch.from_numpy(du.words(atlas).view(np.int32).copy())
        with torch.cuda.stream(side):
            d_atlas = bits.to("cuda")
            d_other = bits.to("cuda")
            d_src = torch.zeros(width * height, dtype=torch.int32, device="cuda")
            d_filled = torch.full((4,), 77, dtype=torch.int32, device="cuda")
            # nothing here waits for the GPU: the source map stays in the library's scratch for the first call
            r.dilateAtlasDevice(d_atlas.data_ptr(), width, height, radius)
            r.dilateAtlasDevice(d_other.data_ptr(), width, height, radius, src_ptr=d_src.data_ptr(), filled_ptr=d_filled.data_ptr())
            same = (d_atlas == d_other).all()             # a torch op on the same stream, behind both
        side.synchronize()
        assert bool(same)
        got = d_atlas.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, du.words(want[0]))
        assert np.array_equal(d_src.cpu().numpy().view(np.uint32).reshape(height, width), want[1])
        assert d_filled.cpu().numpy().tolist() == [want[2], 77, 77, 77]
        from webgpu_raytracer_amd import renderer as R
        d = R.RtDilateDesc(width, height, radius)
        call = r.L.rt_dilate_atlas_device
        assert call(r.ctx, ctypes.addressof(d), d_atlas.data_ptr() + 8, None, None) == RT_ERR_INVALID          # misaligned
        assert call(r.ctx, ctypes.addressof(d), d_atlas.data_ptr(), d_src.data_ptr() + 4, None) == RT_ERR_INVALID
        assert call(r.ctx, ctypes.addressof(d), d_atlas.data_ptr(), None, d_filled.data_ptr() + 4) == RT_ERR_INVALID
        assert call(r.ctx, ctypes.addressof(d), None, None, None) == RT_ERR_INVALID
        assert r.L.rt_last_error(r.ctx).startswith(b"dilate atlas: NULL")
        r.setStream(None)
    finally:
        r.destroy()


def test_a_real_bake(W):
    """cornell under the grid layout at 64 x 64: bakeIrradiance(dilate=4) is the model's dilation of bakeIrradiance(), and
    that is the bake the model makes - today's result"""
    b = pu.bridge_for(W, "cornell")
    m = bu.model_for(W, b)
    uv = bu.grid_uv(b, 0)
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    try:
        W.upload_scene(r, b, 16, 16)
        plain = r.bakeIrradiance(0, 64, 64, 2, 4, bu.SEED, atlas_uv=uv)
        assert np.array_equal(du.words(plain), du.words(m.bakeIrradiance(0, 64, 64, 2, 4, bu.SEED, atlas_uv=uv)[0]))
        as_f32 = plain.view(np.float32).reshape(64, 64, 4)
        covered = int(du.covered_mask(as_f32).sum())
        want = du.dilate_model(as_f32, 4)
        print("covered", covered, "filled", want[2])
        assert 0.1 * 4096 < covered < 0.8 * 4096 and want[2] > 400
        dilated, n, st = r.bakeIrradiance(0, 64, 64, 2, 4, bu.SEED, atlas_uv=uv, stats=True, dilate=4)
        assert n == covered and dilated.dtype == plain.dtype and dilated.shape == plain.shape
        assert np.array_equal(du.words(dilated), du.words(want[0]))
        assert int((dilated["hit_fraction"] == -2).sum()) == want[2]
        # the atlas form, one entry over the whole atlas: the same words
        atlas_form = r.bakeAtlasIrradiance([(0, 0, 0, 64, 64)], 64, 64, 2, 4, bu.SEED, atlas_uv=uv, dilate=4)
        assert np.array_equal(du.words(atlas_form), du.words(want[0]))
        again = r.bakeIrradiance(0, 64, 64, 2, 4, bu.SEED, atlas_uv=uv)
        assert np.array_equal(du.words(again), du.words(plain))
    finally:
        r.destroy()


def test_dilation_leaves_the_render_alone(W):
    """Frames 1-4, dilations, frames 5-8 with lookahead 8 against the same frames without one: accumulation, presented
    image, counters, G-buffer and uniforms are equal; the radiance query's last stats are what they were before."""
    import test_gpu_bake as tgb
    b = pu.bridge_for(W, "cornell")
    W._build.build_rt()
    rays = np.zeros((64, 8), np.float32)
    rays[:, 0:3] = np.asarray(b.cameraData, np.float32)[0:3]
    rays[:, 3] = 1e30
    rays[:, 4:7] = (0.01 * np.arange(64)[:, None] - 0.3) * np.array([1, 0.5, 0], np.float32) + np.array([0, 0, 1], np.float32)
    atlas = du.pattern(65, 63, 0.05, 1)

    def dilations(r):
        r.traceRadiance(rays, 4, 2, 3, stats=True)
        before = r.radianceQueryStats()
        for radius in (7, 24):
            check(r, atlas, radius, "between frames")
        after = r.radianceQueryStats()
        assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in before.items() if k != "kernel_ms"}

    got = tgb._render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), dilations)
    want = tgb._render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), lambda r: None)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "accumulation"
    assert np.array_equal(got[1], want[1]), "captureFrame"
    assert got[2] == want[2], (got[2], want[2])
    for a, w in zip(got[3], want[3]):
        assert np.array_equal(pu.bits(a), pu.bits(w)), "G-buffer"
    assert np.array_equal(got[4], want[4]), "uniforms"


def test_errors(r):
    from webgpu_raytracer_amd import renderer as R
    atlas = du.pattern(8, 8, 0.3, 5)
    keep = atlas.copy()
    src = np.zeros((8, 8), np.uint32)
    n = ctypes.c_uint32(0)

    def desc(width=8, height=8, radius=2, reserved=None):
        d = R.RtDilateDesc(width, height, radius)
        if reserved is not None:
            d.reserved[reserved] = 1
        return d

    def host(d, a=atlas.ctypes.data):
        return r.L.rt_dilate_atlas(r.ctx, ctypes.addressof(d) if d is not None else None, a, src.ctypes.data, ctypes.addressof(n))

    def dev(d, a=atlas.ctypes.data):
        return r.L.rt_dilate_atlas_device(r.ctx, ctypes.addressof(d) if d is not None else None, a, None, None)

    bad = [None, desc(width=0), desc(height=0), desc(width=4097, height=4096), desc(width=1 << 24, height=2),
           desc(width=1 << 31, height=1 << 31), desc(radius=25), desc(radius=0xffffffff)] + [desc(reserved=k) for k in range(5)]
    for d in bad:
        for call in (host, dev):
            assert call(d) == RT_ERR_INVALID, (call.__name__, d and (d.width, d.height, d.radius, list(d.reserved)))
            assert r.L.rt_last_error(r.ctx).startswith(b"dilate atlas:"), r.L.rt_last_error(r.ctx)
    for call in (host, dev):
        assert call(desc(), a=None) == RT_ERR_INVALID and r.L.rt_last_error(r.ctx).startswith(b"dilate atlas: NULL")
    assert np.array_equal(du.words(atlas), du.words(keep)), "a refused call wrote to the atlas"
    with pytest.raises(Exception):
        r.dilateAtlas(keep, 25)
    # the limits themselves are valid: radius 24, and radius 0, which fills nothing; a NULL source map and count
    assert host(desc(radius=24)) == 0 and n.value == du.dilate_model(keep, 24)[2] > 0
    assert np.array_equal(du.words(atlas), du.words(du.dilate_model(keep, 24)[0]))
    atlas[:] = keep
    assert host(desc(radius=0)) == 0 and n.value == 0 and np.array_equal(du.words(atlas), du.words(keep))
    assert r.L.rt_dilate_atlas(r.ctx, ctypes.addressof(desc()), atlas.ctypes.data, None, None) == 0
    assert np.array_equal(du.words(atlas), du.words(du.dilate_model(keep, 2)[0]))
