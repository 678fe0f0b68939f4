"""Reflection probes (rt_capture_reflection / rt_filter_reflection / rt_bake_reflection, their device forms and
rt_reflection_stats), the parts that need no GPU: the seven symbols are declared, exported and bound; rt_reflection_desc is the
documented 32 bytes; the kernels are in the library; every refusal of the rule returns RT_ERR_INVALID with a "reflection:"
message on a context-free call and - where a device is present - on a context without a scene, where n == 0 is RT_OK and the
filter then works."""
import ctypes
import os
import re

import numpy as np
import pytest

import reflection_util as rf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_capture_reflection", "rt_capture_reflection_device", "rt_filter_reflection", "rt_filter_reflection_device",
           "rt_bake_reflection", "rt_bake_reflection_device", "rt_reflection_stats")
RT_ERR_INVALID, RT_ERR_NOT_READY = -1, -3


def test_symbols_are_declared_exported_and_bound(W):
    text = open(os.path.join(REPO, "include", "mi355rt.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    W._build.build_rt()
    lib = ctypes.CDLL(W._build.RT_LIB)
    from webgpu_raytracer_amd import renderer
    L = renderer.load_library()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert hasattr(lib, s), s
        assert s in renderer.EXPORTED_SYMBOLS
        assert getattr(L, s).argtypes is not None
    for m in ("captureReflection", "captureReflectionDevice", "filterReflection", "filterReflectionDevice", "bakeReflection",
              "bakeReflectionDevice", "encodeReflection", "reflectionStats"):
        assert callable(getattr(W.WebGPURenderer, m))
    for f in ("reflection_desc", "reflection_level_offsets", "octa_directions"):
        assert callable(getattr(renderer, f))
    assert "THE REFLECTION RULE" in text
    assert "RT_LIGHTMAP_RGBE8 included" in text                      # the export is rt_encode_atlas as it stands, and says so
    blob = open(W._build.RT_LIB, "rb").read()
    for k in (b"k_reflection_rays", b"k_reflection_texels", b"k_reflection_filter", b"k_reflection_copy"):
        assert k in blob, k


def test_descriptor_layout(W):
    from webgpu_raytracer_amd import renderer as R
    D = R.REFLECTION_DESC_DTYPE
    assert D.itemsize == 32
    assert D.names == ("size", "levels", "spt", "filter_samples", "reserved")
    assert [D.fields[k][1] for k in D.names] == [0, 4, 8, 12, 16]
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    assert "static_assert(sizeof(rt_reflection_desc) == 32" in layout
    assert "__builtin_offsetof(rt_reflection_desc, filter_samples) == 12" in layout
    body = re.search(r"typedef struct rt_reflection_desc \{(.*?)\} rt_reflection_desc;", layout, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.strip() for d in body.split(";") if d.strip()] == [
        "uint32_t size", "uint32_t levels", "uint32_t spt", "uint32_t filter_samples", "uint32_t reserved[4]"]
    d = R.reflection_desc(64, 4, spt=16, filter_samples=512)
    assert np.frombuffer(d.tobytes(), np.uint32).tolist() == [64, 4, 16, 512, 0, 0, 0, 0]
    assert R.reflection_level_offsets(64, 4).tolist() == [0, 4096, 5120, 5376, 5440]


CAPTURE, FILTER = 1, 2


def refused(R):
    """(what, descriptor, n, the parts that refuse it) of every refusal of the descriptor"""
    def desc(**kw):
        d = R.reflection_desc(16, 3, spt=2, filter_samples=128)
        for k, v in kw.items():
            d[k] = v
        return d
    both = CAPTURE | FILTER
    out = [("size %d" % s, desc(size=s), 1, both) for s in (0, 4, 7, 12, 24, 513, 1024)]
    out += [("levels %d" % l, desc(levels=l), 1, both) for l in (0, 1)]
    out += [("smallest level", desc(levels=4), 1, both), ("smallest level", desc(size=8, levels=3), 1, both),
            ("levels 40", desc(levels=40), 1, both)]
    out += [("spt %d" % s, desc(spt=s), 1, CAPTURE) for s in (0, 65537)]
    out += [("filter_samples %d" % k, desc(filter_samples=k), 1, FILTER) for k in (0, 32, 100, 4097, 4160)]
    for k in range(4):
        r = [0, 0, 0, 0]
        r[k] = 1
        out.append(("reserved[%d]" % k, desc(reserved=r), 1, both))
    chain = int(R.reflection_level_offsets(512, 2)[-1])
    out.append(("n * chain", desc(size=512, levels=2), ((1 << 31) + chain - 1) // chain, both))
    return out


def check_refusals(R, L, ctx):
    buf = np.zeros((2, 1024, 4), np.float32)
    probes = np.zeros((2, 8), np.float32)
    B, P = buf.ctypes.data, probes.ctypes.data
    for what, d, n, parts in refused(R):
        D = d.ctypes.data
        calls = [(CAPTURE, lambda: L.rt_capture_reflection(ctx, D, P, n, 4, 0, B, None)),
                 (CAPTURE, lambda: L.rt_capture_reflection_device(ctx, D, P, n, 4, 0, B)),
                 (FILTER, lambda: L.rt_filter_reflection(ctx, D, B, n, B)),
                 (FILTER, lambda: L.rt_filter_reflection_device(ctx, D, B, n, B)),
                 (CAPTURE | FILTER, lambda: L.rt_bake_reflection(ctx, D, P, n, 4, 0, B, None)),
                 (CAPTURE | FILTER, lambda: L.rt_bake_reflection_device(ctx, D, P, n, 4, 0, B))]
        for k, (part, call) in enumerate(calls):
            if not (part & parts):
                continue
            assert call() == RT_ERR_INVALID, (what, k)
            assert L.rt_last_error(ctx).startswith(b"reflection:"), (what, k, L.rt_last_error(ctx))
    assert L.rt_capture_reflection(ctx, None, P, 1, 4, 0, B, None) == RT_ERR_INVALID
    assert L.rt_last_error(ctx).startswith(b"reflection: NULL descriptor")


def test_refusals_without_a_context(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    check_refusals(R, L, None)
    # a good descriptor without a context is still refused, by code alone
    d = R.reflection_desc(16, 3, spt=2, filter_samples=128)
    buf = np.zeros((1, 1024, 4), np.float32)
    assert L.rt_filter_reflection(None, d.ctypes.data, buf.ctypes.data, 1, buf.ctypes.data) == RT_ERR_INVALID
    assert L.rt_bake_reflection(None, d.ctypes.data, buf.ctypes.data, 0, 4, 0, buf.ctypes.data, None) == RT_ERR_INVALID
    assert L.rt_reflection_stats(None, buf.ctypes.data) == RT_ERR_INVALID


def test_argument_rules_on_a_context_without_a_scene(W):
    """The refusals again with a context, then the argument rules in the order the library checks them: n == 0, NULL arrays,
    the pads of the host entries, no scene; the filter needs none and equals the model.  Needs a device to make a context;
    without one the constructor's refusal is the result."""
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    if L.rt_device_count() == 0:
        with pytest.raises(W.RendererError):
            W.WebGPURenderer(0)
        return
    r = W.WebGPURenderer(0)
    try:
        check_refusals(R, L, r.ctx)
        d = R.reflection_desc(16, 3, spt=2, filter_samples=128)
        D = d.ctypes.data
        chain = int(R.reflection_level_offsets(16, 3)[-1])
        maps = np.ones((2, 16, 16, 4), np.float32)
        chains = np.zeros((2, chain, 4), np.float32)
        probes = np.zeros((2, 8), np.float32)
        probes[:, 3] = 1e30
        M, C, P = maps.ctypes.data, chains.ctypes.data, probes.ctypes.data

        def message():
            return L.rt_last_error(r.ctx)

        st = R.RtRadianceStats()
        assert L.rt_capture_reflection(r.ctx, D, None, 0, 4, 0, None, ctypes.addressof(st)) == 0 and st.rays == 0
        assert L.rt_capture_reflection_device(r.ctx, D, None, 0, 4, 0, None) == 0
        assert L.rt_filter_reflection(r.ctx, D, None, 0, None) == 0 and L.rt_filter_reflection_device(r.ctx, D, None, 0, None) == 0
        assert L.rt_bake_reflection(r.ctx, D, None, 0, 4, 0, None, None) == 0
        assert L.rt_bake_reflection_device(r.ctx, D, None, 0, 4, 0, None) == 0
        assert r.reflectionStats()["rays"] == 0
        for a, b in ((None, M), (P, None)):
            assert L.rt_capture_reflection(r.ctx, D, a, 2, 4, 0, b, None) == RT_ERR_INVALID and message().startswith(b"reflection: NULL")
            assert L.rt_bake_reflection(r.ctx, D, a, 2, 4, 0, b, None) == RT_ERR_INVALID and message().startswith(b"reflection: NULL")
            assert L.rt_filter_reflection(r.ctx, D, a, 2, b) == RT_ERR_INVALID and message().startswith(b"reflection: NULL")
            assert L.rt_capture_reflection_device(r.ctx, D, a, 2, 4, 0, b) == RT_ERR_INVALID
            assert L.rt_filter_reflection_device(r.ctx, D, a, 2, b) == RT_ERR_INVALID
            assert L.rt_bake_reflection_device(r.ctx, D, a, 2, 4, 0, b) == RT_ERR_INVALID
        bad = probes.copy()
        bad.view(np.uint32)[1, 7] = (1 << 31) - 255                  # pad + 256 > 2^31; 2^31 - 256 is the accepted edge
        assert L.rt_capture_reflection(r.ctx, D, bad.ctypes.data, 2, 4, 0, M, None) == RT_ERR_INVALID
        assert message().startswith(b"reflection: probe 1: pad")
        assert L.rt_bake_reflection(r.ctx, D, bad.ctypes.data, 2, 4, 0, C, None) == RT_ERR_INVALID
        bad.view(np.uint32)[1, 7] = (1 << 31) - 256
        assert L.rt_capture_reflection(r.ctx, D, bad.ctypes.data, 2, 4, 0, M, None) == RT_ERR_NOT_READY
        assert L.rt_capture_reflection(r.ctx, D, P, 2, 4, 0, M, None) == RT_ERR_NOT_READY and message().startswith(b"reflection: no scene")
        assert L.rt_bake_reflection(r.ctx, D, P, 2, 4, 0, C, None) == RT_ERR_NOT_READY
        # the filter needs no scene
        maps = rf.special_maps(2, 16)
        got = r.filterReflection(d, maps)
        rf.check_words(got, rf.model_filter(rf.desc(16, 3, 2, 128), maps), "filter on an empty context", nan_as_class=True)
        assert np.array_equal(got[:, :256].view(np.uint32), maps.reshape(2, 256, 4).view(np.uint32))
    finally:
        r.destroy()
