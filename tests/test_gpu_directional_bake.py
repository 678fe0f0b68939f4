"""Directional atlas bakes on the GPU (rt_bake_atlas_directional, rt_bake_atlas_directional_lightmap) against their definition
by identity (include/mi355rt.h "directional lightmaps"): the bake is, layer by layer and bit for bit, the scatter of
rt_gather_directional on the points of rt_bake_atlas_points; the finished lightmap in f32 is word for word that bake, then
rt_denoise_atlas per layer, then rt_dilate_atlas per layer, and in f16 the encode model (tests/encode_util.py) of it.  Cornell,
a 48 x 32 atlas under the two layouts of tests/test_gpu_lightmap.py, depth 2, 4 spp.

Parity must not pass on emptiness: the coverage, a nonzero band-1 coefficient, that the filter changes texels and that the
gutter fills some are asserted on the slow route before the new calls are trusted.  The slow route is computed once per layout
and shared."""
import ctypes

import numpy as np
import pytest

import atlas_bake_util as au
import bake_util as bu
import denoise_util as du
import encode_util as eu
import test_gpu_bake as tb
from test_gpu_lightmap import BAKE, DEPTH, FILTER, HEIGHT, LAYOUTS, NONE4, RADIUS, SPP, WIDTH, entries_of

pytestmark = pytest.mark.gpu

RT_ERR_INVALID = -1
TEXELS = WIDTH * HEIGHT
_slow = {}


@pytest.fixture(scope="module")
def scene(W):
    b, m = tb._scene(W, "cornell")
    r = tb._renderer(W, b)
    yield r, b
    r.destroy()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


def slow(scene, layout):
    """the slow route of a layout, once: the points and texels, the gather on them scattered by numpy (`scatter`), and {(filter,
    gutter): four layers}: bakeAtlasDirectional, then denoiseAtlas per layer, then dilateAtlas per layer; the filled count of
    each layer with and without the filter"""
    if layout not in _slow:
        from webgpu_raytracer_amd import renderer as R
        r, b = scene
        entries = entries_of(b, layout)
        uv = au.merged_grid_uv(b, [e[0] for e in entries])
        args = dict(BAKE, atlas_uv=uv)
        points, texels = r.bakeAtlasPoints(entries, WIDTH, HEIGHT, **args)
        res, st = r.gatherDirectional(points, DEPTH, SPP, bu.SEED, stats=True)
        scatter = np.zeros((4, TEXELS), R.IRRADIANCE_DTYPE)
        scatter["hit_fraction"] = -1.0
        scatter.view(np.float32).reshape(4, TEXELS, 4)[:, texels, :] = np.moveaxis(res["layer"], 1, 0)
        scatter = scatter.reshape(4, HEIGHT, WIDTH)
        plain, n = r.bakeAtlasDirectional(entries, WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, **args)
        assert n == len(texels)
        layers = {(False, False): plain}
        layers[(True, False)] = np.stack([r.denoiseAtlas(plain[k], points, texels, **FILTER) for k in range(4)])
        filled = {}
        for f in (False, True):
            done = [r.dilateAtlas(layers[(f, False)][k], RADIUS, filled=True) for k in range(4)]
            layers[(f, True)] = np.stack([d[0] for d in done])
            filled[f] = [d[1] for d in done]
        for a in layers.values():
            a.setflags(write=False)
        scatter.setflags(write=False)
        _slow[layout] = dict(entries=entries, args=args, points=points, texels=texels, gather=res, stats=st, scatter=scatter,
                             layers=layers, filled=filled)
    return _slow[layout]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_slow_route_is_not_empty(scene, layout):
    s = slow(scene, layout)
    a = s["layers"]
    n = len(s["texels"])
    covered = a[(False, False)][0]["hit_fraction"] >= 0
    changed = [(du.words(a[(True, False)][k]) != du.words(a[(False, False)][k])).any(axis=2) for k in range(4)]
    band1 = a[(False, False)][1:]["rgb"]
    print(layout, "covered", n, "changed by the filter per layer", [int(c.sum()) for c in changed], "filled", s["filled"],
          "band-1 words that are not zero", int((band1 != 0).sum()), "negative", int((band1 < 0).sum()))
    assert n == covered.sum() and 0.1 * TEXELS < n < 0.9 * TEXELS
    assert (band1 != 0).any(), "a bake without band 1 would hide the directional part"
    assert (band1 < 0).any(), "band-1 coefficients are signed"
    assert (a[(False, False)][0]["rgb"] > 0).any()
    for k in range(4):
        assert changed[k].sum() >= 1 and not changed[k][~covered].any(), k
    assert s["filled"][False][0] >= 1 and len(set(s["filled"][False] + s["filled"][True])) == 1     # one count for all layers


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_bake_is_the_scatter_of_the_gather(scene, layout):
    from webgpu_raytracer_amd import renderer as R
    r, b = scene
    s = slow(scene, layout)
    want = s["scatter"]
    got, n, st = r.bakeAtlasDirectional(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, stats=True, **s["args"])
    assert got.shape == (4, HEIGHT, WIDTH) and got.dtype == R.IRRADIANCE_DTYPE and n == len(s["texels"])
    for k in range(4):
        bad = np.argwhere((du.words(got[k]) != du.words(want[k])).any(axis=2))
        assert bad.size == 0, (layout, k, len(bad), bad[:8].tolist())
    # uncovered texels are {0, 0, 0, -1} in all four layers; the fourth words of the four layers are equal
    flat = words(got).reshape(4, TEXELS, 4)
    uncovered = np.ones(TEXELS, bool)
    uncovered[s["texels"]] = False
    assert uncovered.any() and (flat[:, uncovered, :] == NONE4).all()
    assert (flat[:, :, 3] == flat[0, :, 3]).all()
    for k in s["stats"]:
        if k != "kernel_ms":
            assert st[k] == s["stats"][k], (k, st[k], s["stats"][k])
    assert st["rays"] == n and st["samples"] == n * SPP
    assert {k: v for k, v in r.directionalGatherStats().items() if k != "kernel_ms"} == \
        {k: v for k, v in st.items() if k != "kernel_ms"}
    plain, n2 = r.bakeAtlasDirectional(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, **s["args"])   # the plain kernel
    assert n2 == n and np.array_equal(words(plain), words(want))


@pytest.mark.parametrize("gutter", (False, True))
@pytest.mark.parametrize("filtered", (False, True))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_f32_is_the_composition(scene, layout, filtered, gutter):
    r, b = scene
    s = slow(scene, layout)
    want = s["layers"][(filtered, gutter)]
    got, n, filled, st = r.bakeAtlasDirectionalLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED,
                                                        denoise=FILTER if filtered else None, dilate=RADIUS if gutter else 0,
                                                        format="f32", stats=True, **s["args"])
    assert got.shape == (4, HEIGHT, WIDTH)
    for k in range(4):
        bad = np.argwhere((du.words(got[k]) != du.words(want[k])).any(axis=2))
        assert bad.size == 0, (layout, filtered, gutter, k, len(bad), bad[:8].tolist())
    assert n == len(s["texels"]) and st["rays"] == n
    assert filled == (s["filled"][filtered][0] if gutter else 0)
    plain, n2, filled2 = r.bakeAtlasDirectionalLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED,
                                                        denoise=FILTER if filtered else None, dilate=RADIUS if gutter else 0,
                                                        **s["args"])                  # without stats: the plain kernel
    assert np.array_equal(words(plain), words(want)) and (n2, filled2) == (n, filled)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_f16_is_the_encode_model_of_the_f32_result(scene, layout):
    r, b = scene
    s = slow(scene, layout)
    for filtered, gutter in ((True, True), (False, False)):
        f32 = s["layers"][(filtered, gutter)]
        kw = dict(denoise=FILTER if filtered else None, dilate=RADIUS if gutter else 0, **s["args"])
        half, n, filled = r.bakeAtlasDirectionalLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, format="f16", **kw)
        assert half.shape == (4, HEIGHT, WIDTH, 4) and half.dtype == np.float16
        for k in range(4):
            assert eu.same_f16(half[k].view(np.uint16), eu.encode_f16(f32[k])), k
            w = f32[k]["hit_fraction"]
            assert np.array_equal(half[k, :, :, 3] == -1, w == -1) and np.array_equal(half[k, :, :, 3] == -2, w == -2)
        assert (half[1:, :, :, :3] < 0).any(), "signed coefficients survive the half format"
        assert n == len(s["texels"]) and filled == (s["filled"][filtered][0] if gutter else 0)


def test_refusals(W, scene):
    from webgpu_raytracer_amd import renderer as R
    r, b = scene
    s = slow(scene, "two")
    L, ctx = r.L, r.ctx
    d, rects = r._atlas_args(s["entries"], WIDTH, HEIGHT, BAKE["t_max"], BAKE["pad_base"])
    uv = np.ascontiguousarray(s["args"]["atlas_uv"], np.float32)
    out = np.full(4 * TEXELS * 4, 0x77777777, np.uint32)

    def call(m, room=out.nbytes, dst=out.ctypes.data):
        return L.rt_bake_atlas_directional_lightmap(ctx, ctypes.addressof(m), rects.ctypes.data, uv.ctypes.data, uv.size // 2, dst,
                                                    room, None, None, None)

    rgbe = r._lightmap_desc(d, DEPTH, SPP, bu.SEED, FILTER, RADIUS, R.RT_LIGHTMAP_RGBE8)
    assert call(rgbe) == RT_ERR_INVALID and L.rt_last_error(ctx).startswith(b"directional lightmap:")
    for fmt, bytes_per in ((R.RT_LIGHTMAP_F32, 16), (R.RT_LIGHTMAP_F16, 8)):
        m = r._lightmap_desc(d, DEPTH, SPP, bu.SEED, FILTER, RADIUS, fmt)
        assert call(m, room=4 * TEXELS * bytes_per - 1) == RT_ERR_INVALID
        assert L.rt_last_error(ctx).startswith(b"directional lightmap: out_bytes")
    assert call(r._lightmap_desc(d, DEPTH, SPP, bu.SEED, dict(FILTER, passes=4), RADIUS, R.RT_LIGHTMAP_F32)) == RT_ERR_INVALID
    assert L.rt_last_error(ctx).startswith(b"directional lightmap:")
    assert call(r._lightmap_desc(d, DEPTH, SPP, bu.SEED, None, 0, R.RT_LIGHTMAP_F32), dst=None) == RT_ERR_INVALID
    assert L.rt_bake_atlas_directional(ctx, ctypes.addressof(d), rects.ctypes.data, uv.ctypes.data, uv.size // 2, DEPTH, 0, 0,
                                       out.ctypes.data, None, None) == RT_ERR_INVALID
    assert L.rt_last_error(ctx).startswith(b"bake directional:")
    with pytest.raises(W.RendererError, match="directional lightmap"):
        r.bakeAtlasDirectionalLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, format="rgbe", **s["args"])
    r.sync()
    assert (out == 0x77777777).all(), "a refused call wrote"
    # the smallest valid room is accepted, and the context is as usable as before
    m = r._lightmap_desc(d, DEPTH, SPP, bu.SEED, FILTER, RADIUS, R.RT_LIGHTMAP_F16)
    assert call(m, room=4 * TEXELS * 8) == 0
    assert (out[4 * TEXELS * 2:] == 0x77777777).all(), "words behind the four encoded layers were written"
    got, n, filled = r.bakeAtlasDirectionalLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, denoise=FILTER, dilate=RADIUS,
                                                    **s["args"])
    assert np.array_equal(words(got), words(s["layers"][(True, True)]))


def test_two_calls_give_the_same_words(scene):
    r, b = scene
    s = slow(scene, "overlap")
    for fmt in ("f32", "f16"):
        kw = dict(denoise=FILTER, dilate=RADIUS, format=fmt, **s["args"])
        a = r.bakeAtlasDirectionalLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, **kw)[0]
        # another size and another format in between: every staging array is re-used or grown
        r.bakeAtlasDirectionalLightmap([(0, 0, 0, 61, 40)], 61, 40, DEPTH, SPP, bu.SEED + 1, dilate=5, format="f16",
                                       atlas_uv=s["args"]["atlas_uv"])
        c = r.bakeAtlasDirectionalLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, **kw)[0]
        assert np.array_equal(words(a), words(c)), fmt
    other = r.bakeAtlasDirectional(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED + 1, **s["args"])[0]
    assert not np.array_equal(words(other), words(s["layers"][(False, False)])), "the seed is used"
    # the flat lightmap on the same context still gives its own words after directional bakes
    flat = r.bakeAtlasLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, denoise=FILTER, dilate=RADIUS, **s["args"])
    want = r.bakeAtlasIrradiance(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, denoise=FILTER, dilate=RADIUS, **s["args"])
    assert np.array_equal(words(flat), words(want))


def test_entries_that_cover_nothing(scene):
    r, b = scene
    s = slow(scene, "two")
    none = np.full_like(s["args"]["atlas_uv"], -1.0)
    got, n, st = r.bakeAtlasDirectional(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, stats=True, atlas_uv=none, **BAKE)
    assert n == 0 and all(st[k] == 0 for k in st), st
    assert np.array_equal(words(got).reshape(-1, 4), np.tile(NONE4, (4 * TEXELS, 1)))
    for filtered, gutter in ((True, True), (False, False)):
        kw = dict(denoise=FILTER if filtered else None, dilate=RADIUS if gutter else 0, atlas_uv=none, **BAKE)
        got, n, filled, st = r.bakeAtlasDirectionalLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, stats=True, **kw)
        assert (n, filled) == (0, 0) and all(st[k] == 0 for k in st), st
        assert np.array_equal(words(got).reshape(-1, 4), np.tile(NONE4, (4 * TEXELS, 1)))
        half, n, filled = r.bakeAtlasDirectionalLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, format="f16", **kw)
        assert (n, filled) == (0, 0)
        assert np.array_equal(half.view(np.uint16).reshape(-1, 4), np.tile(np.array([0, 0, 0, 0xbc00], np.uint16), (4 * TEXELS, 1)))
    # ... and an ordinary one on the same context
    got = r.bakeAtlasDirectionalLightmap(s["entries"], WIDTH, HEIGHT, DEPTH, SPP, bu.SEED, denoise=FILTER, dilate=RADIUS,
                                         **s["args"])[0]
    assert np.array_equal(words(got), words(s["layers"][(True, True)]))
