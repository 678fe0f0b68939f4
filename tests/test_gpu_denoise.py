"""Atlas denoise on the GPU (rt_denoise_atlas / rt_denoise_atlas_device, csrc/k_denoise.hip.h) against the reference model
(tests/model/denoise_model.cpp, held to paper by tests/test_denoise_model.py), word for word.

The atlas sizes are the smallest at which the kernel can go wrong: 1 x 1, one column and one row of 9, 16 x 16 (half a tile
wide, two tiles high), 17 x 33 (a partial tile, five tile rows, the last of one texel row) and 37 x 21 (a second tile column
of five texels, a partial third tile row); at every step 1 .. 4 the window hangs over every border of these.  The guides are
denoise_util.two_walls at coverages 0.1, 0.6 and 1.0.

Parity must not pass on emptiness: the six tap counts of every named pattern are asserted on the model before the GPU is
asked."""
import ctypes

import numpy as np
import pytest

import bake_util as bu
import denoise_util as du
import dilate_util as dl
import parity_util as pu

pytestmark = pytest.mark.gpu

RT_ERR_INVALID = -1
SIZES = ((1, 1), (1, 9), (9, 1), (16, 16), (17, 33), (37, 21))
CALLS = ((1, 1), (2, 1), (3, 1), (4, 1), (1, 3), (2, 2))          # (step, passes)
COVERAGES = (0.1, 0.6, 1.0)


@pytest.fixture(scope="module")
def r(W):
    """a context without a scene: denoising needs none"""
    W._build.build_rt()
    ctx = W.WebGPURenderer(0)
    yield ctx
    ctx.destroy()


def check(r, atlas, points, texels, kw, tag, want=None):
    """the GPU's atlas against the model's, every word; -> the model's atlas"""
    if want is None:
        want = du.denoise_model(atlas, points, texels, **kw)[0]
    keep = du.words(atlas).copy()
    out = r.denoiseAtlas(atlas, points, texels, **kw)
    assert out is not atlas and out.shape == atlas.shape and out.dtype == atlas.dtype
    assert np.array_equal(du.words(atlas), keep), (tag, "the input was written")
    bad = du.same_words(out, want)
    assert not bad.any(), (tag, "texels differ at", np.argwhere(bad)[:8].tolist(), du.as_f32(out)[bad][:4].tolist(),
                           want[bad][:4].tolist())
    return want


@pytest.mark.parametrize("width,height", SIZES)
def test_bit_parity_with_the_model(r, width, height):
    accepted = 0
    for p in COVERAGES:
        atlas, points, texels = du.two_walls(width, height, p, 7)
        for step, passes in CALLS:
            kw = dict(du.PARAMS, step=step, passes=passes)
            want, counts = du.denoise_model(atlas, points, texels, **kw)
            accepted += sum(c[0] for c in counts)
            check(r, atlas, points, texels, kw, "%dx%d p=%g step=%d passes=%d" % (width, height, p, step, passes), want)
    if width * height > 1:
        assert accepted > 0, "no tap was accepted at this size"


def test_special_values_among_the_colours(r):
    """inf, NaN, denormals and both zeros in a fifth of the colour words, guided and unguided texels alike: unguided texels
    keep their bits; where the model's word is a NaN the device's need only be a NaN; every other word is equal"""
    atlas, points, texels = du.two_walls(37, 21, 0.6, 3)
    atlas = du.special_values(atlas, 11)
    for step, passes in ((1, 1), (4, 1), (1, 3)):
        kw = dict(du.PARAMS, step=step, passes=passes)
        want = check(r, atlas, points, texels, kw, "special values step=%d passes=%d" % (step, passes))
        assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
        unguided = np.ones(37 * 21, bool)
        unguided[texels] = False
        out = r.denoiseAtlas(atlas, points, texels, **kw)
        assert np.array_equal(du.words(out).reshape(-1, 4)[unguided], du.words(atlas).reshape(-1, 4)[unguided])


@pytest.mark.parametrize("key", sorted(du.PATTERNS))
def test_named_patterns(r, key):
    width, height, p, seed, step = key
    atlas, points, texels = du.two_walls(width, height, p, seed)
    want, counts = du.model_pass(atlas, points, texels, step, **du.PARAMS)
    print(key, dict(zip(du.COUNTS, counts)))
    assert counts == du.PATTERNS[key] and min(counts) > 0
    check(r, atlas, points, texels, dict(du.PARAMS, step=step, passes=1), str(key), want)


def test_hand_worked_cases(r):
    for name, (atlas, points, texels, kw, want) in sorted(du.hand_cases().items()):
        out = r.denoiseAtlas(atlas, points, texels, **kw)
        assert du.words(out).tolist() == du.words(want).tolist(), name


def test_a_call_is_the_composition_of_its_passes(r):
    atlas, points, texels = du.two_walls(37, 21, 0.6, 3)
    whole = r.denoiseAtlas(atlas, points, texels, step=1, passes=3, **du.PARAMS)
    a = atlas
    for step in (1, 2, 4):
        a = r.denoiseAtlas(a, points, texels, step=step, passes=1, **du.PARAMS)
    assert np.array_equal(du.words(whole), du.words(a))
    # duplicates and entries past the atlas, shuffled: the lowest j guides, on the device as in the model
    rng = np.random.default_rng(9)
    extra = rng.integers(0, len(texels), 200)
    tex2 = np.concatenate([texels, texels[extra], np.array([37 * 21, 0xffffffff, 1 << 24], np.uint32)])
    pts2 = np.concatenate([points, points[rng.permutation(extra)], points[:3]])
    order = rng.permutation(len(tex2))
    check(r, atlas, pts2[order], tex2[order], dict(du.PARAMS, step=1, passes=3), "duplicates")
    # no points at all: a copy
    none = r.denoiseAtlas(atlas, np.zeros((0, 8), np.float32), np.zeros(0, np.uint32), **du.PARAMS)
    assert np.array_equal(du.words(none), du.words(atlas))


def test_device_entry_on_a_torch_side_stream(W):
    import torch
    width, height = 37, 21
    atlas, points, texels = du.two_walls(width, height, 0.6, 3)
    n = len(texels)
    kw3 = dict(du.PARAMS, step=1, passes=3)
    kw1 = dict(du.PARAMS, step=4, passes=1)
    want3 = du.denoise_model(atlas, points, texels, **kw3)[0]
    want31 = du.denoise_model(want3, points, texels, **kw1)[0]
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    try:
        side = torch.cuda.Stream()
        r.setStream(side.cuda_stream)
        with torch.cuda.stream(side):
            # as bakePointsDevice fills them: room for every texel, the first n records written
            d_points = torch.zeros((width * height, 8), dtype=torch.float32, device="cuda")
            d_texels = torch.zeros(width * height, dtype=torch.int32, device="cuda")
            d_points[:n] = torch.from_numpy(points.view(np.int32).copy()).to("cuda").view(torch.float32)
            d_texels[:n] = torch.from_numpy(texels.view(np.int32).copy()).to("cuda")
            d_in = torch.from_numpy(du.words(atlas).view(np.int32).copy()).to("cuda")
            d_keep = d_in.clone()
            d_a = torch.zeros_like(d_in)
            d_b = torch.zeros_like(d_in)
            # nothing here waits for the GPU: the second call reads what the first wrote, through the library's one scratch
            r.denoiseAtlasDevice(d_in.data_ptr(), d_points.data_ptr(), d_texels.data_ptr(), n, d_a.data_ptr(), width, height, **kw3)
            r.denoiseAtlasDevice(d_a.data_ptr(), d_points.data_ptr(), d_texels.data_ptr(), n, d_b.data_ptr(), width, height, **kw1)
            unchanged = (d_in == d_keep).all()            # a torch op on the same stream, behind both
        side.synchronize()
        assert bool(unchanged), "atlas_in was written"
        assert np.array_equal(d_a.cpu().numpy().view(np.uint32), du.words(want3))
        assert np.array_equal(d_b.cpu().numpy().view(np.uint32), du.words(want31))
        from webgpu_raytracer_amd import renderer as R
        d = R.RtDenoiseDesc(width, height, 1, 3, 0.9, 0.02, 0.5)
        call = r.L.rt_denoise_atlas_device
        i, p, t, o = d_in.data_ptr(), d_points.data_ptr(), d_texels.data_ptr(), d_b.data_ptr()
        for args in ((i + 8, p, t, n, o), (i, p + 8, t, n, o), (i, p, t + 4, n, o), (i, p, t, n, o + 4)):      # misaligned
            assert call(r.ctx, ctypes.addressof(d), *args) == RT_ERR_INVALID, args
            assert r.L.rt_last_error(r.ctx).startswith(b"denoise atlas:")
        for args in ((None, p, t, n, o), (i, None, t, n, o), (i, p, None, n, o), (i, p, t, n, None)):
            assert call(r.ctx, ctypes.addressof(d), *args) == RT_ERR_INVALID, args
            assert r.L.rt_last_error(r.ctx).startswith(b"denoise atlas: NULL")
        assert call(r.ctx, ctypes.addressof(d), i, p, t, n, i) == RT_ERR_INVALID                                # equal
        assert r.L.rt_last_error(r.ctx).startswith(b"denoise atlas:")
        # without points the point arrays may be NULL
        assert call(r.ctx, ctypes.addressof(d), i, None, None, 0, o) == 0
        side.synchronize()
        assert np.array_equal(d_b.cpu().numpy().view(np.uint32), du.words(atlas))
        assert np.array_equal(d_in.cpu().numpy().view(np.uint32), du.words(atlas)), "a refused call wrote to the atlas"
        r.setStream(None)
    finally:
        r.destroy()


def test_a_real_bake(W):
    """cornell under the grid layout at 64 x 64: bakeIrradiance(denoise={...}) is the model's denoise of bakeIrradiance() with
    the points of bakePoints; the one-entry atlas form gives the same words; denoise then dilate=4 is the models' composition;
    a plain bake afterwards is what it was"""
    b = pu.bridge_for(W, "cornell")
    uv = bu.grid_uv(b, 0)
    kw = dict(normal_cos=0.9, plane_eps=0.02, max_dist=0.5, passes=3)
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    try:
        W.upload_scene(r, b, 16, 16)
        plain = r.bakeIrradiance(0, 64, 64, 2, 4, bu.SEED, atlas_uv=uv)
        points, texels = r.bakePoints(0, 64, 64, atlas_uv=uv)
        want, counts = du.denoise_model(plain, points, texels, **kw)
        print("covered", len(texels), "counts", counts)
        assert len(texels) == 1193 and all(min(c) > 0 for c in counts)
        got, n, st = r.bakeIrradiance(0, 64, 64, 2, 4, bu.SEED, atlas_uv=uv, stats=True, denoise=kw)
        assert n == len(texels) and got.dtype == plain.dtype and got.shape == plain.shape
        assert np.array_equal(du.words(got), du.words(want))
        assert not np.array_equal(du.words(got), du.words(plain))
        atlas_form = r.bakeAtlasIrradiance([(0, 0, 0, 64, 64)], 64, 64, 2, 4, bu.SEED, atlas_uv=uv, denoise=kw)
        assert np.array_equal(du.words(atlas_form), du.words(want))
        both = r.bakeIrradiance(0, 64, 64, 2, 4, bu.SEED, atlas_uv=uv, denoise=kw, dilate=4)
        want_both = dl.dilate_model(want, 4)
        assert want_both[2] > 400
        assert np.array_equal(du.words(both), du.words(want_both[0]))
        again = r.bakeIrradiance(0, 64, 64, 2, 4, bu.SEED, atlas_uv=uv)
        assert np.array_equal(du.words(again), du.words(plain))
    finally:
        r.destroy()


def test_denoising_leaves_the_render_alone(W):
    """Frames 1-4, denoise calls, frames 5-8 with lookahead 8 against the same frames without one: accumulation, presented
    image, counters, G-buffer and uniforms are equal; the radiance query's last stats are what they were before."""
    import test_gpu_bake as tgb
    b = pu.bridge_for(W, "cornell")
    W._build.build_rt()
    rays = np.zeros((64, 8), np.float32)
    rays[:, 0:3] = np.asarray(b.cameraData, np.float32)[0:3]
    rays[:, 3] = 1e30
    rays[:, 4:7] = (0.01 * np.arange(64)[:, None] - 0.3) * np.array([1, 0.5, 0], np.float32) + np.array([0, 0, 1], np.float32)
    atlas, points, texels = du.two_walls(37, 21, 0.6, 3)

    def denoises(r):
        r.traceRadiance(rays, 4, 2, 3, stats=True)
        before = r.radianceQueryStats()
        for step, passes in ((1, 3), (4, 1)):
            check(r, atlas, points, texels, dict(du.PARAMS, step=step, passes=passes), "between frames")
        after = r.radianceQueryStats()
        assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in before.items() if k != "kernel_ms"}

    got = tgb._render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), denoises)
    want = tgb._render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), lambda r: None)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "accumulation"
    assert np.array_equal(got[1], want[1]), "captureFrame"
    assert got[2] == want[2], (got[2], want[2])
    for a, w in zip(got[3], want[3]):
        assert np.array_equal(pu.bits(a), pu.bits(w)), "G-buffer"
    assert np.array_equal(got[4], want[4]), "uniforms"


def test_errors(r):
    from webgpu_raytracer_amd import renderer as R
    atlas, points, texels = du.two_walls(8, 8, 0.6, 5)
    n = len(texels)
    out = np.full((8, 8, 4), 77.0, np.float32)

    def desc(width=8, height=8, step=1, passes=1, reserved=0):
        d = R.RtDenoiseDesc(width, height, step, passes, 0.9, 0.02, 0.5)
        d.reserved[0] = reserved
        return d

    def host(d, a=atlas.ctypes.data, p=points.ctypes.data, t=texels.ctypes.data, n=n, o=out.ctypes.data):
        return r.L.rt_denoise_atlas(r.ctx, ctypes.addressof(d) if d is not None else None, a, p, t, n, o)

    def dev(d, a=atlas.ctypes.data, p=points.ctypes.data, t=texels.ctypes.data, n=n, o=out.ctypes.data):
        return r.L.rt_denoise_atlas_device(r.ctx, ctypes.addressof(d) if d is not None else None, a, p, t, n, o)

    bad = [None, desc(reserved=1), desc(width=0), desc(height=0), desc(width=4097, height=4096), desc(width=1 << 24, height=2),
           desc(width=1 << 31, height=1 << 31), desc(step=0), desc(passes=0), desc(step=5), desc(step=3, passes=2),
           desc(step=2, passes=3), desc(step=1, passes=4), desc(step=1, passes=34), desc(step=1, passes=0xffffffff),
           desc(step=0x80000000, passes=2), desc(width=4, height=4)]                # the last: n = 8 x 8 x 0.6 > 16 texels
    assert n > 16
    for d in bad:
        for call in (host, dev):
            assert call(d) == RT_ERR_INVALID, (call.__name__, d and (d.width, d.height, d.step, d.passes, d.reserved[0]))
            assert r.L.rt_last_error(r.ctx).startswith(b"denoise atlas:"), r.L.rt_last_error(r.ctx)
    for call in (host, dev):
        for null in (dict(a=None), dict(p=None), dict(t=None), dict(o=None)):
            assert call(desc(), **null) == RT_ERR_INVALID and r.L.rt_last_error(r.ctx).startswith(b"denoise atlas: NULL"), null
    assert (out == 77.0).all(), "a refused call wrote to the output"
    with pytest.raises(Exception):
        r.denoiseAtlas(atlas, points, texels, passes=4, **du.PARAMS)
    # the limits themselves are valid: step 4, step 1 with three passes, step 2 with two; n == 0 with NULL point arrays; the
    # output in place of the input on the host; float parameters are not validated - a NaN rejects every tap but the centre
    for step, passes in ((4, 1), (1, 3), (2, 2)):
        assert host(desc(step=step, passes=passes)) == 0
        want = du.denoise_model(atlas, points, texels, step=step, passes=passes, **du.PARAMS)[0]
        assert np.array_equal(du.words(out), du.words(want))
    assert host(desc(), p=None, t=None, n=0) == 0 and np.array_equal(du.words(out), du.words(atlas))
    same = atlas.copy()
    assert host(desc(step=1, passes=3), a=same.ctypes.data, o=same.ctypes.data) == 0
    assert np.array_equal(du.words(same), du.words(du.denoise_model(atlas, points, texels, **du.PARAMS)[0]))
    for odd in (dict(normal_cos=du.NAN), dict(normal_cos=1.5), dict(plane_eps=du.NAN), dict(max_dist=du.NAN), dict(plane_eps=-1.0)):
        kw = dict(du.PARAMS, passes=1, **odd)
        got = check(r, atlas, points, texels, kw, str(odd))
        centre_only = du.denoise_model(atlas, points[:0], texels[:0], **kw)[0].reshape(-1, 4).copy()
        flat = atlas.reshape(-1, 4)
        centre_only[texels] = (np.float32(0.140625) * flat[texels]) / np.float32(0.140625)
        assert np.array_equal(du.words(got), du.words(centre_only.reshape(8, 8, 4))), odd
