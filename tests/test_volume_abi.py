"""Irradiance volumes (rt_bake_volume / rt_sample_volume / rt_encode_volume and their device forms), the parts that need no
GPU: the six symbols are declared, exported and bound; rt_volume_desc is the documented 64 bytes; the four kernels are in the
library; every refusal of the descriptor returns RT_ERR_INVALID with a "volume:" message on a context-free call and - where a
device is present - on a context without a scene, where sampling and encoding then work; sh_hanning_window is its formula; the
Node addon carries the bindings."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_bake_volume", "rt_bake_volume_device", "rt_sample_volume", "rt_sample_volume_device", "rt_encode_volume",
           "rt_encode_volume_device")
RT_ERR_INVALID, RT_ERR_NOT_READY = -1, -3


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
    for m in ("bakeVolume", "bakeVolumeDevice", "sampleVolume", "sampleVolumeDevice", "encodeVolume"):
        assert callable(getattr(W.WebGPURenderer, m))
    assert "THE VOLUME RULE" in open(os.path.join(REPO, "include", "mi355rt.h")).read()
    blob = open(W._build.RT_LIB, "rb").read()
    for k in (b"k_volume_probes", b"k_volume_finish", b"k_volume_sample", b"k_volume_layers"):
        assert k in blob, k


def test_descriptor_layout(W):
    from webgpu_raytracer_amd import renderer as R
    D = R.VOLUME_DESC_DTYPE
    assert D.itemsize == 64
    assert D.names == ("origin", "nx", "step", "ny", "window", "nz", "t_max", "pad_first", "max_hit_fraction", "reserved")
    assert [D.fields[k][1] for k in D.names] == [0, 12, 16, 28, 32, 44, 48, 52, 56, 60]
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    assert "static_assert(sizeof(rt_volume_desc) == 64" in layout
    body = re.search(r"typedef struct rt_volume_desc \{(.*?)\} rt_volume_desc;", layout, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.strip() for d in body.split(";") if d.strip()] == [
        "float origin[3]", "uint32_t nx", "float step[3]", "uint32_t ny", "float window[3]", "uint32_t nz", "float t_max",
        "uint32_t pad_first", "float max_hit_fraction", "uint32_t reserved"]
    d = R.volume_desc((1, 2, 3), (0.5, 0.25, 2), (4, 5, 6), window=(1, 0.5, 0.25), t_max=9, pad_first=7, max_hit_fraction=0.5)
    words = np.frombuffer(d.tobytes(), np.float32)
    assert words[[0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 14]].tolist() == [1, 2, 3, 0.5, 0.25, 2, 1, 0.5, 0.25, 9, 0.5]
    assert np.frombuffer(d.tobytes(), np.uint32)[[3, 7, 11, 13, 15]].tolist() == [4, 5, 6, 7, 0]


def test_hanning_window_is_its_formula(W):
    from webgpu_raytracer_amd import renderer as R
    w = R.sh_hanning_window(3)
    assert w.dtype == np.float32 and w.shape == (3,)
    assert np.array_equal(w, np.array([(1 + np.cos(np.pi * l / 3)) / 2 for l in (0, 1, 2)], np.float32))
    assert w[0] == 1.0 and abs(float(w[1]) - 0.75) < 1e-7 and abs(float(w[2]) - 0.25) < 1e-7
    assert np.array_equal(R.sh_hanning_window(1e9), np.ones(3, np.float32))


def refused_descriptors(R):
    """(what, descriptor) of every refusal of the rule"""
    def desc(**kw):
        d = R.volume_desc((0, 0, 0), (1, 1, 1), (2, 3, 4))
        for k, v in kw.items():
            d[k] = v
        return d
    out = []
    for name in ("nx", "ny", "nz"):
        out += [(name + " 0", desc(**{name: 0})), (name + " 1025", desc(**{name: 1025}))]
    out.append(("n > 2^24", desc(nx=1024, ny=1024, nz=17)))
    out.append(("pads", desc(pad_first=(1 << 31) - 23)))
    for bad in (0.0, -1.0, np.nan, np.inf):
        for a in range(3):
            s = [1.0, 1.0, 1.0]
            s[a] = bad
            out.append(("step %r" % bad, desc(step=s)))
    for bad in (-0.5, np.nan, np.inf):
        for a in range(3):
            s = [1.0, 1.0, 1.0]
            s[a] = bad
            out.append(("window %r" % bad, desc(window=s)))
    out.append(("max_hit_fraction", desc(max_hit_fraction=np.nan)))
    out.append(("reserved", desc(reserved=1)))
    return out


def check_refusals(R, L, ctx):
    vol = np.zeros((24, 28), np.float32)
    pts = np.zeros((4, 8), np.float32)
    res = np.zeros((4, 4), np.float32)
    layers = np.zeros((7, 24, 4), np.float32)
    for what, d in refused_descriptors(R):
        calls = (lambda: L.rt_bake_volume(ctx, d.ctypes.data, 4, 1, 0, vol.ctypes.data, None),
                 lambda: L.rt_bake_volume_device(ctx, d.ctypes.data, 4, 1, 0, vol.ctypes.data),
                 lambda: L.rt_sample_volume(ctx, d.ctypes.data, vol.ctypes.data, pts.ctypes.data, 4, res.ctypes.data),
                 lambda: L.rt_sample_volume_device(ctx, d.ctypes.data, vol.ctypes.data, pts.ctypes.data, 4, res.ctypes.data),
                 lambda: L.rt_encode_volume(ctx, d.ctypes.data, 0, vol.ctypes.data, layers.ctypes.data, layers.nbytes),
                 lambda: L.rt_encode_volume_device(ctx, d.ctypes.data, 0, vol.ctypes.data, layers.ctypes.data, layers.nbytes))
        for k, call in enumerate(calls):
            assert call() == RT_ERR_INVALID, (what, k)
            assert L.rt_last_error(ctx).startswith(b"volume:"), (what, k, L.rt_last_error(ctx))
    # the accepted edges: 1024 on an axis, n == 2^24, pad_first + n == 2^31 and window 0 get past the descriptor (RGBE8 is the
    # next refusal, and it is the volume's own)
    ok = R.volume_desc((0, 0, 0), (1, 1, 1), (1024, 1024, 16), window=(0, 0, 0), pad_first=(1 << 31) - (1 << 24))
    assert L.rt_encode_volume(ctx, ok.ctypes.data, 2, vol.ctypes.data, layers.ctypes.data, layers.nbytes) == RT_ERR_INVALID
    assert L.rt_last_error(ctx).startswith(b"volume: RT_LIGHTMAP_RGBE8")
    assert L.rt_encode_volume(ctx, ok.ctypes.data, 3, vol.ctypes.data, layers.ctypes.data, layers.nbytes) == RT_ERR_INVALID
    assert L.rt_last_error(ctx).startswith(b"volume: format")


def test_refusals_without_a_context(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    check_refusals(R, L, None)
    # a good descriptor without a context is still refused, by code alone
    d = R.volume_desc((0, 0, 0), (1, 1, 1), (2, 3, 4))
    vol = np.zeros((24, 28), np.float32)
    assert L.rt_bake_volume(None, d.ctypes.data, 4, 1, 0, vol.ctypes.data, None) == RT_ERR_INVALID
    assert L.rt_sample_volume(None, d.ctypes.data, vol.ctypes.data, vol.ctypes.data, 0, vol.ctypes.data) == RT_ERR_INVALID
    assert L.rt_encode_volume(None, d.ctypes.data, 0, vol.ctypes.data, vol.ctypes.data, 1 << 20) == RT_ERR_INVALID
    assert L.rt_bake_volume(None, None, 4, 1, 0, vol.ctypes.data, None) == RT_ERR_INVALID


def test_argument_rules_on_a_context_without_a_scene(W):
    """The refusals again with a context, then the argument rules in the order the library checks them.  Sampling and encoding
    need no scene; a bake without one is RT_ERR_NOT_READY.  Needs a device to make a context; without one the constructor's
    refusal is the result."""
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    if L.rt_device_count() == 0:
        with pytest.raises(W.RendererError):
            W.WebGPURenderer(0)
        return
    r = W.WebGPURenderer(0)
    try:
        check_refusals(R, L, r.ctx)
        d = R.volume_desc((0, 0, 0), (1, 1, 1), (2, 3, 4))
        vol = np.zeros((24, 28), np.float32)
        vol[:, 0:3] = 1.0
        pts = np.zeros((4, 8), np.float32)
        pts[:, 6] = 1.0
        res = np.zeros((4, 4), np.float32)
        layers = np.zeros((7, 24, 4), np.float32)
        D, V, P, O = d.ctypes.data, vol.ctypes.data, pts.ctypes.data, res.ctypes.data

        def message():
            return L.rt_last_error(r.ctx)

        for spp in (0, 65537):
            assert L.rt_bake_volume(r.ctx, D, 4, spp, 0, V, None) == RT_ERR_INVALID and message().startswith(b"volume:")
            assert b"spp" in message()
            assert L.rt_bake_volume_device(r.ctx, D, 4, spp, 0, V) == RT_ERR_INVALID
        assert L.rt_bake_volume(r.ctx, D, 4, 1, 0, None, None) == RT_ERR_INVALID and message().startswith(b"volume: NULL")
        assert L.rt_bake_volume_device(r.ctx, D, 4, 1, 0, None) == RT_ERR_INVALID
        assert L.rt_bake_volume(r.ctx, D, 4, 1, 0, V, None) == RT_ERR_NOT_READY and message().startswith(b"volume: no scene")
        # sampling: n == 0 is RT_OK whatever the pointers, n >= 2^31 and NULL are refused, and no scene is needed
        assert L.rt_sample_volume(r.ctx, D, None, None, 0, None) == 0
        assert L.rt_sample_volume_device(r.ctx, D, None, None, 0, None) == 0
        assert L.rt_sample_volume(r.ctx, D, V, P, 1 << 31, O) == RT_ERR_INVALID and message().startswith(b"volume:")
        assert L.rt_sample_volume_device(r.ctx, D, V, P, 1 << 31, O) == RT_ERR_INVALID
        for a, b, c in ((None, P, O), (V, None, O), (V, P, None)):
            assert L.rt_sample_volume(r.ctx, D, a, b, 4, c) == RT_ERR_INVALID and message().startswith(b"volume: NULL")
            assert L.rt_sample_volume_device(r.ctx, D, a, b, 4, c) == RT_ERR_INVALID
        assert L.rt_sample_volume(r.ctx, D, V, P, 4, O) == 0
        assert np.array_equal(res[:, 3], np.ones(4, np.float32)) and (res[:, 0] > 0).all()
        # encoding: the capacity, NULL, and no scene needed
        assert L.rt_encode_volume(r.ctx, D, 0, V, layers.ctypes.data, layers.nbytes - 1) == RT_ERR_INVALID
        assert L.rt_encode_volume(r.ctx, D, 0, None, layers.ctypes.data, layers.nbytes) == RT_ERR_INVALID
        assert L.rt_encode_volume(r.ctx, D, 0, V, layers.ctypes.data, layers.nbytes) == 0
        assert np.array_equal(layers.reshape(7, 24, 4), vol.reshape(24, 7, 4).transpose(1, 0, 2))
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
    js = ("const m=require('%s/index.js');console.log(typeof m.native.rtBakeVolume,typeof m.native.rtSampleVolume,"
          "typeof m.native.rtEncodeVolume,typeof m.WebGPURenderer.prototype.bakeVolume,"
          "typeof m.WebGPURenderer.prototype.sampleVolume,typeof m.WebGPURenderer.prototype.encodeVolume)" % node_dir)
    out = subprocess.run([shutil.which("node"), "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ["function"] * 6
    assert os.path.exists(os.path.join(node_dir, "bake_volume.js"))
    dts = open(os.path.join(node_dir, "index.d.ts")).read()
    for m in ("bakeVolume(", "sampleVolume(", "encodeVolume("):
        assert m in dts, m
