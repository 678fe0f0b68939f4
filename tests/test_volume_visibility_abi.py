"""Probe visibility maps (rt_bake_volume_visibility / rt_sample_volume_visible / rt_encode_volume_visibility, their device
forms and rt_volume_visibility_stats), the parts that need no GPU: the seven symbols are declared, exported and bound;
rt_volume_visibility_desc is the documented 32 bytes; the four kernels are in the library; every refusal returns
RT_ERR_INVALID with a "volume visibility:" message on a context-free call - the volume descriptor's own refusals keep their
"volume:" - and, where a device is present, on a context without a scene, where sampling and the export then work; the Node
addon carries the bindings."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_bake_volume_visibility", "rt_bake_volume_visibility_device", "rt_volume_visibility_stats",
           "rt_sample_volume_visible", "rt_sample_volume_visible_device", "rt_encode_volume_visibility",
           "rt_encode_volume_visibility_device")
RT_ERR_INVALID, RT_ERR_NOT_READY = -1, -3
PREFIX = b"volume visibility:"


def test_symbols_are_declared_exported_and_bound(W):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mi355rt.h")).read(), flags=re.S)
    W._build.build_rt()
    lib = ctypes.CDLL(W._build.RT_LIB)
    from webgpu_raytracer_amd import renderer
    L = renderer.load_library()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert hasattr(lib, s), s
        assert s in renderer.EXPORTED_SYMBOLS
        assert getattr(L, s).argtypes is not None
    for m in ("bakeVolumeVisibility", "bakeVolumeVisibilityDevice", "sampleVolumeVisible", "sampleVolumeVisibleDevice",
              "encodeVolumeVisibility", "volumeVisibilityStats"):
        assert callable(getattr(W.WebGPURenderer, m))
    assert "THE VISIBILITY RULE" in open(os.path.join(REPO, "include", "mi355rt.h")).read()
    blob = open(W._build.RT_LIB, "rb").read()
    for k in (b"k_visibility_rays", b"k_visibility_texels", b"k_volume_sample_visible", b"k_visibility_tiles"):
        assert k in blob, k


def test_descriptor_layout(W):
    from webgpu_raytracer_amd import renderer as R
    D = R.VOLUME_VISIBILITY_DESC_DTYPE
    assert D.itemsize == 32
    assert D.names == ("size", "spt", "max_distance", "normal_bias", "min_visibility", "crush_threshold", "flags", "reserved")
    assert [D.fields[k][1] for k in D.names] == [0, 4, 8, 12, 16, 20, 24, 28]
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    assert "static_assert(sizeof(rt_volume_visibility_desc) == 32" in layout
    assert re.search(r"#define RT_VOLUME_VIS_BACKFACE 1u", layout) and R.RT_VOLUME_VIS_BACKFACE == 1
    body = re.search(r"typedef struct rt_volume_visibility_desc \{(.*?)\} rt_volume_visibility_desc;", layout, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.strip() for d in body.split(";") if d.strip()] == [
        "uint32_t size", "uint32_t spt", "float max_distance", "float normal_bias", "float min_visibility",
        "float crush_threshold", "uint32_t flags", "uint32_t reserved"]
    d = R.volume_visibility_desc(16, 2.5, spt=7, normal_bias=0.125, min_visibility=0.25, crush_threshold=0.5, backface=True)
    assert np.frombuffer(d.tobytes(), np.uint32)[[0, 1, 6, 7]].tolist() == [16, 7, 1, 0]
    assert np.frombuffer(d.tobytes(), np.float32)[[2, 3, 4, 5]].tolist() == [2.5, 0.125, 0.25, 0.5]


def refused_descriptors(R):
    """(what, volume descriptor, visibility descriptor, the entries it is refused by: "all" or "bake")"""
    vol = R.volume_desc((0, 0, 0), (1, 1, 1), (2, 3, 4))

    def vis(**kw):
        v = R.volume_visibility_desc(8, 2.0, spt=4)
        for k, val in kw.items():
            v[k] = val
        return v
    out = []
    for size in (0, 1, 2, 3, 6, 12, 33, 64):
        out.append(("size %d" % size, vol, vis(size=size), "all"))
    for spt in (0, 65537):
        out.append(("spt %d" % spt, vol, vis(spt=spt), "bake"))
    for bad in (0.0, -1.0, np.nan, np.inf):
        out.append(("max_distance %r" % bad, vol, vis(max_distance=bad), "all"))
    for bad in (-0.5, np.nan, np.inf):
        out.append(("normal_bias %r" % bad, vol, vis(normal_bias=bad), "all"))
    for name in ("min_visibility", "crush_threshold"):
        for bad in (-0.25, 1.5, np.nan, np.inf):
            out.append(("%s %r" % (name, bad), vol, vis(**{name: bad}), "all"))
    for flags in (2, 3, 1 << 31):
        out.append(("flags %d" % flags, vol, vis(flags=flags), "all"))
    out.append(("reserved", vol, vis(reserved=1), "all"))
    big = R.volume_desc((0, 0, 0), (1, 1, 1), (1024, 1024, 2))             # 2^21 probes of 2^10 texels
    out.append(("n * size^2 == 2^31", big, vis(size=32), "all"))
    edge = R.volume_desc((0, 0, 0), (1, 1, 1), (1024, 1024, 1), pad_first=(1 << 30) + 1)   # 2^20 probes of 2^10 texels
    out.append(("pads", edge, vis(size=32), "bake"))
    return out


def check_refusals(R, L, ctx):
    buf = np.zeros(1 << 16, np.float32)                                    # stands for every array: a refusal comes first
    B = buf.ctypes.data
    for what, d, v, who in refused_descriptors(R):
        D, V = d.ctypes.data, v.ctypes.data
        bake = (lambda: L.rt_bake_volume_visibility(ctx, D, V, 0, B, None),
                lambda: L.rt_bake_volume_visibility_device(ctx, D, V, 0, B))
        rest = (lambda: L.rt_sample_volume_visible(ctx, D, V, B, B, B, 4, B),
                lambda: L.rt_sample_volume_visible_device(ctx, D, V, B, B, B, 4, B),
                lambda: L.rt_encode_volume_visibility(ctx, D, V, 0, B, B, 1 << 40),
                lambda: L.rt_encode_volume_visibility_device(ctx, D, V, 0, B, B + 1024, 1 << 40))
        for k, call in enumerate(bake + (rest if who == "all" else ())):
            assert call() == RT_ERR_INVALID, (what, k)
            assert L.rt_last_error(ctx).startswith(PREFIX), (what, k, L.rt_last_error(ctx))
    # the volume descriptor is checked first, by the volume's own check
    d = R.volume_desc((0, 0, 0), (1, 1, 1), (2, 3, 4))
    d["reserved"] = 1
    v = R.volume_visibility_desc(8, 2.0)
    v["size"] = 5
    assert L.rt_sample_volume_visible(ctx, d.ctypes.data, v.ctypes.data, B, B, B, 4, B) == RT_ERR_INVALID
    assert L.rt_last_error(ctx).startswith(b"volume: reserved")
    # arrays and formats, on good descriptors
    d = R.volume_desc((0, 0, 0), (1, 1, 1), (2, 3, 4))
    v = R.volume_visibility_desc(8, 2.0, spt=4)
    D, V = d.ctypes.data, v.ctypes.data
    A = (B + 15) & ~15                                                     # a 16-byte aligned address inside buf
    calls = [lambda: L.rt_bake_volume_visibility(ctx, D, V, 0, None, None),
             lambda: L.rt_bake_volume_visibility_device(ctx, D, V, 0, None),
             lambda: L.rt_bake_volume_visibility_device(ctx, D, V, 0, A + 8),
             lambda: L.rt_encode_volume_visibility(ctx, D, V, 0, None, A, 1 << 40),
             lambda: L.rt_encode_volume_visibility(ctx, D, V, 0, A, None, 1 << 40),
             lambda: L.rt_encode_volume_visibility(ctx, D, V, 2, A, A + 4096, 1 << 40),       # RGBE8
             lambda: L.rt_encode_volume_visibility(ctx, D, V, 3, A, A + 4096, 1 << 40),
             lambda: L.rt_encode_volume_visibility(ctx, D, V, 0, A, A + 4096, 24 * 100 * 8 - 1),
             lambda: L.rt_encode_volume_visibility_device(ctx, D, V, 0, A, A, 1 << 40),        # dev_out == dev_in
             lambda: L.rt_encode_volume_visibility_device(ctx, D, V, 0, A + 8, A + 4096, 1 << 40),
             lambda: L.rt_sample_volume_visible(ctx, D, V, A, A, A, 1 << 31, A),
             lambda: L.rt_sample_volume_visible_device(ctx, D, V, A, A, A, 1 << 31, A)]
    for k in range(4):
        arrays = [A, A, A, A]
        arrays[k] = None
        calls.append(lambda a=tuple(arrays): L.rt_sample_volume_visible(ctx, D, V, a[0], a[1], a[2], 4, a[3]))
        calls.append(lambda a=tuple(arrays): L.rt_sample_volume_visible_device(ctx, D, V, a[0], a[1], a[2], 4, a[3]))
        arrays[k] = A + 4
        calls.append(lambda a=tuple(arrays): L.rt_sample_volume_visible_device(ctx, D, V, a[0], a[1], a[2], 4, a[3]))
    for k, call in enumerate(calls):
        assert call() == RT_ERR_INVALID, k
        assert L.rt_last_error(ctx).startswith(PREFIX), (k, L.rt_last_error(ctx))
    # the accepted edges get past the descriptors: size 4 and 32, n * size^2 == 2^31 - 2^10, pad_first + texels == 2^31 - then
    # the NULL array is the refusal
    ok = R.volume_desc((0, 0, 0), (1, 1, 1), (1024, 1024, 1), pad_first=1 << 30)
    for size, spt in ((32, 65536), (4, 1)):
        v = R.volume_visibility_desc(size, 1e-30, spt=spt, min_visibility=1.0, crush_threshold=1.0, backface=True)
        assert L.rt_bake_volume_visibility(ctx, ok.ctypes.data, v.ctypes.data, 0, None, None) == RT_ERR_INVALID
        assert L.rt_last_error(ctx).startswith(PREFIX + b" NULL")


def test_refusals_without_a_context(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    check_refusals(R, L, None)
    # good arguments without a context are still refused, by code alone
    d = R.volume_desc((0, 0, 0), (1, 1, 1), (2, 3, 4))
    v = R.volume_visibility_desc(8, 2.0, spt=4)
    buf = np.zeros(1 << 16, np.float32)
    B = (buf.ctypes.data + 15) & ~15
    D, V = d.ctypes.data, v.ctypes.data
    assert L.rt_bake_volume_visibility(None, D, V, 0, B, None) == RT_ERR_INVALID
    assert L.rt_bake_volume_visibility_device(None, D, V, 0, B) == RT_ERR_INVALID
    assert L.rt_sample_volume_visible(None, D, V, B, B, B, 4, B) == RT_ERR_INVALID
    assert L.rt_sample_volume_visible(None, D, V, B, B, B, 0, B) == RT_ERR_INVALID
    assert L.rt_sample_volume_visible_device(None, D, V, B, B, B, 4, B) == RT_ERR_INVALID
    assert L.rt_encode_volume_visibility(None, D, V, 0, B, B + 4096, 1 << 40) == RT_ERR_INVALID
    assert L.rt_encode_volume_visibility_device(None, D, V, 0, B, B + 4096, 1 << 40) == RT_ERR_INVALID
    assert L.rt_volume_visibility_stats(None, B) == RT_ERR_INVALID
    assert L.rt_bake_volume_visibility(None, D, None, 0, B, None) == RT_ERR_INVALID
    assert L.rt_last_error(None).startswith(PREFIX + b" NULL descriptor")


def test_argument_rules_on_a_context_without_a_scene(W):
    """The refusals again with a context.  Sampling and the export need no scene; a bake without one is RT_ERR_NOT_READY; n ==
    0 points is RT_OK whatever the pointers.  Needs a device to make a context; without one the constructor's refusal is the
    result."""
    from webgpu_raytracer_amd import renderer as R
    import volume_visibility_util as vv
    L = R.load_library()
    if L.rt_device_count() == 0:
        with pytest.raises(W.RendererError):
            W.WebGPURenderer(0)
        return
    r = W.WebGPURenderer(0)
    try:
        check_refusals(R, L, r.ctx)
        d = R.volume_desc((0, 0, 0), (1, 1, 1), (2, 3, 4))
        v = R.volume_visibility_desc(8, 2.0, spt=4)
        D, V = d.ctypes.data, v.ctypes.data
        maps = vv.constant_maps(d, v, 100.0)
        assert L.rt_bake_volume_visibility(r.ctx, D, V, 0, maps.ctypes.data, None) == RT_ERR_NOT_READY
        assert L.rt_last_error(r.ctx).startswith(PREFIX + b" no scene")
        assert L.rt_sample_volume_visible(r.ctx, D, V, None, None, None, 0, None) == 0
        assert L.rt_sample_volume_visible_device(r.ctx, D, V, None, None, None, 0, None) == 0
        vol = np.zeros((24, 28), np.float32)
        vol[:, 0:3] = 1.0
        pts = np.zeros((4, 8), np.float32)
        pts[:, 6] = 1.0
        got = r.sampleVolumeVisible(d, v, vol, maps, pts)
        assert np.array_equal(got["hit_fraction"], np.ones(4, np.float32)) and (got["rgb"] > 0).all()
        tiles = r.encodeVolumeVisibility(d, v, maps, "f32")
        assert tiles.shape == (120, 20, 2) and (tiles[..., 0] == 100.0).all()
        with pytest.raises(W.RendererError, match="volume visibility: RT_LIGHTMAP_RGBE8"):
            r.encodeVolumeVisibility(d, v, maps, "rgbe")
        assert r.volumeVisibilityStats()["rays"] == 0
    finally:
        r.destroy()


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                    reason="node / node_api.h not present")
def test_node_addon_exports_the_bindings(W):
    W._build.build_scene()
    W._build.build_tex()
    W._build.build_rt()
    path = W._build.build_node_addon(force=True)
    assert path and os.path.exists(path)
    node_dir = os.path.dirname(path)
    js = ("const m=require('%s/index.js');console.log(typeof m.native.rtBakeVolumeVisibility,"
          "typeof m.native.rtSampleVolumeVisible,typeof m.native.rtEncodeVolumeVisibility,typeof m.WebGPURenderer.volumeVisibilityDesc,"
          "typeof m.WebGPURenderer.prototype.bakeVolumeVisibility,typeof m.WebGPURenderer.prototype.sampleVolumeVisible,"
          "typeof m.WebGPURenderer.prototype.encodeVolumeVisibility)" % node_dir)
    out = subprocess.run([shutil.which("node"), "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ["function"] * 7
    dts = open(os.path.join(node_dir, "index.d.ts")).read()
    for m in ("volumeVisibilityDesc(", "bakeVolumeVisibility(", "sampleVolumeVisible(", "encodeVolumeVisibility("):
        assert m in dts, m
    assert "--visibility" in open(os.path.join(node_dir, "bake_volume.js")).read()
