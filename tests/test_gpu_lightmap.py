"""The one-call lightmap on the GPU (rt_bake_atlas_lightmap / _device) against its definition by identity (include/mi355rt.h
"lightmaps"): with RT_LIGHTMAP_F32 the result is word for word rt_bake_atlas_irradiance, then rt_denoise_atlas with the points
of rt_bake_atlas_points, then rt_dilate_atlas - the slow route bakeAtlasIrradiance(..., denoise=..., dilate=...), which is
what it was before this call existed - and with another format it is the encode model (tests/encode_util.py) of that atlas.
Cornell, a 48 x 32 atlas under two layouts - two entries side by side, two rectangles that overlap - at depth 2 and 4 spp.

Parity must not pass on emptiness: that the filter changes texels and the gutter fills some is asserted on the slow route
before the new call is asked.  The slow route is computed once per layout and shared."""
import ctypes

import numpy as np
import pytest

import atlas_bake_util as au
import bake_util as bu
import denoise_util as du
import encode_util as eu
import parity_util as pu
import test_gpu_bake as tb

pytestmark = pytest.mark.gpu

RT_ERR_INVALID, RT_ERR_NOT_READY = -1, -3
WIDTH, HEIGHT, DEPTH, SPP = 48, 32, 2, 4
FILTER = dict(du.PARAMS, passes=2, step=1)
RADIUS = 3
BAKE = dict(t_max=5.0, pad_base=1000)
NONE4 = np.array([0, 0, 0, -1], np.float32).view(np.uint32)
LAYOUTS = ("two", "overlap")
_slow = {}


def entries_of(b, layout):
    n = au.instance_count(b)
    if layout == "two":
        return [(0, 0, 0, 24, 32), (1 % n, 24, 0, 24, 32)]
    return [(0, 0, 0, 30, 28), (1 % n, 19, 5, 29, 27)]          # the second rectangle ends at the atlas's corner


@pytest.fixture(scope="module")
def scene(W):
    b, m = tb._scene(W, "cornell")
    r = tb._renderer(W, b)
    yield r, b
    r.destroy()


def slow(scene, layout):
    """the slow route of a layout, once: {(filter, gutter): atlas}, the count, the gather's stats, the filled count with and
    without the filter, and the arguments"""
    if layout not in _slow:
        r, b = scene
        entries = entries_of(b, layout)
        uv = au.merged_grid_uv(b, [e[0] for e in entries])
        args = dict(BAKE, atlas_uv=uv)
        plain, n, st = r.bakeAtlasIrradiance(entries, WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, stats=True, **args)
        atlases = {(False, False): plain}
        atlases[(True, False)] = r.bakeAtlasIrradiance(entries, WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, denoise=FILTER, **args)
        atlases[(False, True)] = r.bakeAtlasIrradiance(entries, WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, dilate=RADIUS, **args)
        atlases[(True, True)] = r.bakeAtlasIrradiance(entries, WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, denoise=FILTER, dilate=RADIUS,
                                                       **args)
        filled = {f: r.dilateAtlas(atlases[(f, False)], RADIUS, filled=True)[1] for f in (False, True)}
        _slow[layout] = dict(entries=entries, args=args, atlases=atlases, n=n, stats=st, filled=filled)
    return _slow[layout]


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_slow_route_is_not_empty(scene, layout):
    s = slow(scene, layout)
    a = s["atlases"]
    covered = a[(False, False)]["hit_fraction"] >= 0
    changed = (du.words(a[(True, False)]) != du.words(a[(False, False)])).any(axis=2)
    gutter = a[(False, True)]["hit_fraction"] == -2
    print(layout, "covered", s["n"], "changed by the filter", int(changed.sum()), "filled", s["filled"], "lit",
          int((a[(False, False)]["rgb"] > 0).any(axis=2).sum()))
    assert s["n"] == covered.sum() and 0.1 * WIDTH * HEIGHT < s["n"] < 0.9 * WIDTH * HEIGHT
    assert changed.sum() >= 1 and not changed[~covered].any()
    assert s["filled"][False] == gutter.sum() >= 1 and s["filled"][True] == s["filled"][False]
    assert (a[(False, False)]["rgb"] > 0).any(), "a black bake would hide the colours"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_plain_f32_is_the_atlas_bake(scene, layout):
    from webgpu_raytracer_amd import renderer as R
    r, b = scene
    s = slow(scene, layout)
    got, n, filled, st = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, stats=True, **s["args"])
    assert got.shape == (HEIGHT, WIDTH) and got.dtype == R.IRRADIANCE_DTYPE
    assert np.array_equal(words(got), words(s["atlases"][(False, False)]))
    assert n == s["n"] and filled == 0
    for k in s["stats"]:
        if k != "kernel_ms":
            assert st[k] == s["stats"][k], (k, st[k], s["stats"][k])
    assert st["rays"] == n and st["samples"] == n * SPP
    assert {k: v for k, v in r.irradianceGatherStats().items() if k != "kernel_ms"} == \
        {k: v for k, v in st.items() if k != "kernel_ms"}


@pytest.mark.parametrize("gutter", (False, True))
@pytest.mark.parametrize("filtered", (False, True))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_f32_is_the_composition(scene, layout, filtered, gutter):
    r, b = scene
    s = slow(scene, layout)
    want = s["atlases"][(filtered, gutter)]
    got, n, filled, st = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, denoise=FILTER if filtered else None,
                                             dilate=RADIUS if gutter else 0, format="f32", stats=True, **s["args"])
    bad = np.argwhere((du.words(got) != du.words(want)).any(axis=2))
    assert bad.size == 0, (layout, filtered, gutter, len(bad), bad[:8].tolist())
    assert n == s["n"]
    assert filled == (s["filled"][filtered] if gutter else 0)
    plain = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, denoise=FILTER if filtered else None,
                                dilate=RADIUS if gutter else 0, **s["args"])       # without stats: the plain kernel
    assert np.array_equal(words(plain), words(want))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_f16_and_rgbe8_are_the_encode_model_of_the_f32_result(scene, layout):
    r, b = scene
    s = slow(scene, layout)
    for filtered, gutter in ((True, True), (False, False)):
        f32 = s["atlases"][(filtered, gutter)]
        kw = dict(denoise=FILTER if filtered else None, dilate=RADIUS if gutter else 0, **s["args"])
        half, n, filled, _ = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, format="f16", stats=True, **kw)
        assert half.shape == (HEIGHT, WIDTH, 4) and half.dtype == np.float16
        assert eu.same_f16(half.view(np.uint16), eu.encode_f16(f32))
        assert n == s["n"] and filled == (s["filled"][filtered] if gutter else 0)
        rgbe = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, format="rgbe", **kw)
        want = eu.encode_rgbe(f32).reshape(HEIGHT, WIDTH)
        assert rgbe.shape == (HEIGHT, WIDTH) and rgbe.dtype == np.uint32
        assert np.array_equal(rgbe, want), np.argwhere(rgbe != want)[:8].tolist()
        assert (want != 0).sum() > 50 and (want == 0).any()
        # coverage survives both formats
        w = f32["hit_fraction"]
        assert np.array_equal(half[:, :, 3] == -1, w == -1) and np.array_equal(half[:, :, 3] == -2, w == -2)
        assert not want[w == -1].any()


def test_the_device_output_form_equals_the_host_form(scene):
    import torch
    r, b = scene
    s = slow(scene, "overlap")
    texels = WIDTH * HEIGHT
    d_uv = torch.from_numpy(np.ascontiguousarray(s["args"]["atlas_uv"], np.float32)).to("cuda")
    for fmt, bytes_per in (("f32", 16), ("f16", 8), ("rgbe", 4)):
        kw = dict(denoise=FILTER, dilate=RADIUS, format=fmt)
        host = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, **kw, **s["args"])
        d_out = torch.full((texels * 4 + 4,), 0x55555555, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        n, filled = r.bakeAtlasLightmapDevice(s["entries"], WIDTH, HEIGHT, d_out.data_ptr(), texels * bytes_per, DEPTH, SPP, bu.SEED,
                                              atlas_uv_ptr=d_uv.data_ptr(), **kw, **BAKE)
        r.sync()
        got = d_out.cpu().numpy().view(np.uint32)
        used = texels * bytes_per // 4
        assert (n, filled) == (s["n"], s["filled"][True])
        assert np.array_equal(got[:used], words(host)), fmt
        assert (got[used:] == 0x55555555).all(), "words behind the encoded atlas were written"
    # the C entry with every optional output NULL: nothing but the count read waits for the device
    from webgpu_raytracer_amd import renderer as R
    d, rects = r._atlas_args(s["entries"], WIDTH, HEIGHT, BAKE["t_max"], BAKE["pad_base"])
    m = r._lightmap_desc(d, DEPTH, SPP, bu.SEED, FILTER, RADIUS, R.RT_LIGHTMAP_RGBE8)
    d_out = torch.zeros(texels, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert r.L.rt_bake_atlas_lightmap_device(r.ctx, ctypes.addressof(m), rects.ctypes.data, d_uv.data_ptr(), d_out.data_ptr(),
                                             texels * 4, None, None, None) == 0
    r.sync()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), eu.encode_rgbe(s["atlases"][(True, True)]))


def test_bake_lightmap_is_the_one_entry_atlas_form(scene):
    r, b = scene
    uv = bu.grid_uv(b, 0)
    kw = dict(denoise=FILTER, dilate=RADIUS, atlas_uv=uv, **BAKE)
    for fmt in ("f32", "rgbe"):
        one, n1, f1, _ = r.bakeLightmap(0, 33, 31, DEPTH, SPP, bu.SEED, format=fmt, stats=True, **kw)
        atlas, n2, f2, _ = r.bakeAtlasLightmap([(0, 0, 0, 33, 31)], 33, 31, DEPTH, SPP, bu.SEED, format=fmt, stats=True, **kw)
        assert np.array_equal(words(one), words(atlas)) and (n1, f1) == (n2, f2) and n1 > 0 and f1 > 0
    # ... which is the single-instance slow route, by identity (A)
    want = r.bakeIrradiance(0, 33, 31, DEPTH, SPP, bu.SEED, denoise=FILTER, dilate=RADIUS, atlas_uv=uv, **BAKE)
    assert np.array_equal(words(r.bakeLightmap(0, 33, 31, DEPTH, SPP, bu.SEED, **kw)), words(want))


def test_entries_that_cover_nothing(scene):
    r, b = scene
    s = slow(scene, "two")
    none = np.full_like(s["args"]["atlas_uv"], -1.0)
    texels = WIDTH * HEIGHT
    for filtered, gutter in ((True, True), (False, False)):
        kw = dict(denoise=FILTER if filtered else None, dilate=RADIUS if gutter else 0, atlas_uv=none, **BAKE)
        got, n, filled, st = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, stats=True, **kw)
        assert (n, filled) == (0, 0) and all(st[k] == 0 for k in st), st
        assert np.array_equal(words(got).reshape(-1, 4), np.tile(NONE4, (texels, 1)))
        half, n, filled, _ = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, format="f16", stats=True, **kw)
        assert (n, filled) == (0, 0)
        assert np.array_equal(half.view(np.uint16).reshape(-1, 4), np.tile(np.array([0, 0, 0, 0xbc00], np.uint16), (texels, 1)))
        rgbe, n, filled, _ = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, format="rgbe", stats=True, **kw)
        assert (n, filled) == (0, 0) and not rgbe.any()
    # ... and an ordinary one on the same context
    got = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, denoise=FILTER, dilate=RADIUS, **s["args"])
    assert np.array_equal(words(got), words(s["atlases"][(True, True)]))


def test_two_calls_give_the_same_words(scene):
    r, b = scene
    s = slow(scene, "overlap")
    for fmt in ("f32", "f16", "rgbe"):
        kw = dict(denoise=FILTER, dilate=RADIUS, format=fmt, **s["args"])
        a = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, **kw)
        # another size and another format in between: every staging array is re-used or grown
        r.bakeAtlasLightmap([(0, 0, 0, 61, 40)], 61, 40, DEPTH, SPP, bu.SEED + 1, dilate=5, format="f16", atlas_uv=s["args"]["atlas_uv"])
        c = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, **kw)
        assert np.array_equal(words(a), words(c)), fmt
    other = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED + 1, **s["args"])
    assert not np.array_equal(words(other), words(s["atlases"][(False, False)])), "the seed is used"


def test_lightmap_bakes_leave_the_render_alone(W):
    """Frames 1-4, lightmap bakes, frames 5-8 with lookahead 8 against the same frames without a bake: accumulation, presented
    image, counters, G-buffer and uniforms are equal; the radiance query's last stats are what they were before."""
    b, m = tb._scene(W, "cornell")
    W._build.build_rt()
    entries = entries_of(b, "overlap")
    uv = au.merged_grid_uv(b, [e[0] for e in entries])
    rays = np.zeros((64, 8), np.float32)
    rays[:, 0:3] = np.asarray(b.cameraData, np.float32)[0:3]
    rays[:, 3] = 1e30
    rays[:, 4:7] = (0.01 * np.arange(64)[:, None] - 0.3) * np.array([1, 0.5, 0], np.float32) + np.array([0, 0, 1], np.float32)

    def bakes(r):
        r.traceRadiance(rays, 4, 2, 3, stats=True)
        before = r.radianceQueryStats()
        for fmt in ("f32", "rgbe"):
            got, n, filled, _ = r.bakeAtlasLightmap(entries, WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, denoise=FILTER, dilate=RADIUS,
                                                    format=fmt, atlas_uv=uv, stats=True, **BAKE)
            assert n > 0 and filled > 0
        after = r.radianceQueryStats()
        assert {k: v for k, v in after.items() if k != "kernel_ms"} == {k: v for k, v in before.items() if k != "kernel_ms"}

    got = tb._render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), bakes)
    ref = tb._render(W, b, (1, 2, 3, 4), (5, 6, 7, 8), lambda r: None)
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), "accumulation"
    assert np.array_equal(got[1], ref[1]), "captureFrame"
    assert got[2] == ref[2], (got[2], ref[2])
    for a, w in zip(got[3], ref[3]):
        assert np.array_equal(pu.bits(a), pu.bits(w)), "G-buffer"
    assert np.array_equal(got[4], ref[4]), "uniforms"


def test_refusals(W, scene):
    import torch
    from webgpu_raytracer_amd import renderer as R
    r, b = scene
    s = slow(scene, "two")
    L, ctx = r.L, r.ctx
    n_inst = au.instance_count(b)
    n_verts = np.asarray(b.uvs).size // 2
    uv = np.ascontiguousarray(s["args"]["atlas_uv"], np.float32)
    out = np.full(8 * 8 * 4, 0x77777777, np.uint32)
    d_out = torch.full((8 * 8 * 4,), 0x77777777, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    keep = []

    def desc(width=8, height=8, pad_base=0, n_entries=1, spp=1, passes=0, step=1, radius=0, fmt=0, reserved=0):
        d = R.RtLightmapDesc(width, height, pad_base, 1e30, n_entries, 2, spp, 0, passes, step, 0.9, 0.02, 0.5, radius, fmt)
        d.reserved[0] = reserved
        return d

    def rect(inst=0, x=0, y=0, w=8, h=8, reserved=0):
        q = R.RtBakeRect(inst, x, y, w, h)
        q.reserved[0] = reserved
        return q

    def addr(o):
        keep.append(o)
        return ctypes.addressof(o) if o is not None else None

    def host(d, q, uv_ptr=None, n_uv=0, dst=out.ctypes.data, room=out.nbytes, c=ctx):
        return L.rt_bake_atlas_lightmap(c, addr(d), addr(q), uv_ptr, n_uv, dst, room, None, None, None)

    def dev(d, q, dst=d_out.data_ptr(), room=out.nbytes, c=ctx):
        return L.rt_bake_atlas_lightmap_device(c, addr(d), addr(q), None, dst, room, None, None, None)

    bad = [(None, rect()), (desc(), None), (desc(reserved=1), rect()), (desc(), rect(reserved=1)),
           (desc(fmt=3), rect()), (desc(fmt=0xffffffff), rect()),
           (desc(passes=4), rect()), (desc(passes=0xffffffff), rect()), (desc(passes=1, step=5), rect()),
           (desc(passes=2, step=3), rect()), (desc(passes=3, step=2), rect()), (desc(passes=1, step=0), rect()),
           (desc(passes=2, step=0x80000000), rect()),
           (desc(radius=25), rect()), (desc(radius=0xffffffff), rect()),
           (desc(n_entries=0), rect()), (desc(n_entries=65537), rect()), (desc(width=0), rect()), (desc(height=0), rect()),
           (desc(width=4097, height=4096), rect()), (desc(pad_base=(1 << 31) - 63), rect()),
           (desc(), rect(w=0)), (desc(), rect(x=1)), (desc(), rect(h=9)), (desc(), rect(x=0xfffffff0, w=32)),
           (desc(), rect(inst=n_inst)),
           (desc(spp=0), rect()), (desc(spp=65537), rect())]
    for d, q in bad:
        for call in (host, dev):
            assert call(d, q) == RT_ERR_INVALID, (call.__name__, d and (d.width, d.height, d.passes, d.step, d.format), q and q.inst)
            assert L.rt_last_error(ctx).startswith(b"lightmap:"), L.rt_last_error(ctx)
    # the output: NULL, or too small for the format by one byte
    assert host(desc(), rect(), dst=None) == RT_ERR_INVALID and L.rt_last_error(ctx).startswith(b"lightmap:")
    assert dev(desc(), rect(), dst=None) == RT_ERR_INVALID and L.rt_last_error(ctx).startswith(b"lightmap:")
    for fmt, bytes_per in ((0, 16), (1, 8), (2, 4)):
        for call in (host, dev):
            assert call(desc(fmt=fmt), rect(), room=64 * bytes_per - 1) == RT_ERR_INVALID, (call.__name__, fmt)
            assert L.rt_last_error(ctx).startswith(b"lightmap:")
    assert dev(desc(), rect(), dst=d_out.data_ptr() + 8) == RT_ERR_INVALID and L.rt_last_error(ctx).startswith(b"lightmap:")
    assert host(desc(), rect(), uv.ctypes.data, n_verts - 1) == RT_ERR_INVALID and L.rt_last_error(ctx).startswith(b"lightmap:")
    with pytest.raises(Exception):
        r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, denoise=dict(FILTER, passes=4), **s["args"])
    with pytest.raises(ValueError):
        r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, format="rgbm", **s["args"])
    with pytest.raises(TypeError):
        r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, denoise=dict(passes=1), **s["args"])
    r.sync()
    assert (out == 0x77777777).all() and (d_out.cpu().numpy().view(np.uint32) == 0x77777777).all(), "a refused call wrote"
    # without a scene: RT_ERR_NOT_READY under the same prefix
    fresh = W.WebGPURenderer(0)
    try:
        assert host(desc(), rect(), c=fresh.ctx) == RT_ERR_NOT_READY and L.rt_last_error(fresh.ctx).startswith(b"lightmap:")
        assert dev(desc(), rect(), c=fresh.ctx) == RT_ERR_NOT_READY and L.rt_last_error(fresh.ctx).startswith(b"lightmap:")
    finally:
        fresh.destroy()
    # the limits themselves are valid, and the context is as usable as before
    for d in (desc(passes=3, step=1, radius=24, fmt=2), desc(passes=1, step=4, fmt=1), desc(passes=2, step=2), desc(passes=0, step=99)):
        assert host(d, rect()) == 0, (d.passes, d.step)
    assert dev(desc(fmt=2), rect(), room=64 * 4) == 0
    got = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, denoise=FILTER, dilate=RADIUS, **s["args"])
    assert np.array_equal(words(got), words(s["atlases"][(True, True)]))
