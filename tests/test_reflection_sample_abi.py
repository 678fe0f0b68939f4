"""The reflection sampler (rt_sample_reflection, rt_sample_reflection_device), the parts that need no GPU: the two symbols are
declared, exported and bound; the three records are the documented 32 bytes, in the dtypes and in the static_asserts; the
kernels are in the library; the Node declarations exist; the documents say what was built; every refusal of the rule returns
RT_ERR_INVALID with a "reflection:" message on a context-free call and - where a device is present - on a context without a
scene, where n == 0 is RT_OK and the sampler then works and equals the model."""
import os
import re

import numpy as np
import pytest

import reflection_sample_util as rs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_sample_reflection", "rt_sample_reflection_device")
RT_OK, RT_ERR_INVALID = 0, -1


def _read(*path):
    with open(os.path.join(REPO, *path)) as f:
        return f.read()


def test_symbols_are_declared_exported_and_bound(W):
    import ctypes
    text = _read("include", "mi355rt.h")
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    W._build.build_rt()
    lib = ctypes.CDLL(W._build.RT_LIB)
    from webgpu_raytracer_amd import renderer
    L = renderer.load_library()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert hasattr(lib, s), s
        assert s in renderer.EXPORTED_SYMBOLS
        assert len(getattr(L, s).argtypes) == 9
    for m in ("sampleReflection", "sampleReflectionDevice"):
        assert callable(getattr(W.WebGPURenderer, m))
    for f in ("reflection_sample_desc", "reflection_queries"):
        assert callable(getattr(renderer, f))
    assert "THE REFLECTION SAMPLE RULE" in text
    blob = open(W._build.RT_LIB, "rb").read()
    for form in (b"Lb0", b"Lb1"):                                    # both instantiations, by their mangled names
        assert b"k_reflection_sampleI" + form + b"E" in blob, form


def test_record_layouts(W):
    from webgpu_raytracer_amd import renderer as R
    layout = _read("include", "mi355rt_layout.h")
    records = {
        "rt_reflection_sample_desc": (R.REFLECTION_SAMPLE_DESC_DTYPE, ("size", "levels", "flags", "reserved"), [0, 4, 8, 12],
                                      ["uint32_t size", "uint32_t levels", "uint32_t flags", "uint32_t reserved[5]"]),
        "rt_reflection_query": (R.REFLECTION_QUERY_DTYPE, ("position", "probe", "direction", "roughness"), [0, 12, 16, 28],
                                ["float position[3]", "uint32_t probe", "float direction[3]", "float roughness"]),
        "rt_reflection_box": (R.REFLECTION_BOX_DTYPE, ("lo", "unused0", "hi", "unused1"), [0, 12, 16, 28],
                              ["float lo[3]", "float unused0", "float hi[3]", "float unused1"]),
    }
    for name, (D, names, offsets, members) in records.items():
        assert D.itemsize == 32 and D.names == names and [D.fields[k][1] for k in names] == offsets, name
        assert "static_assert(sizeof(%s) == 32" % name in layout, name
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), layout, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        assert [d.strip() for d in body.split(";") if d.strip()] == members, name
    for text in ("__builtin_offsetof(rt_reflection_sample_desc, flags) == 8", "__builtin_offsetof(rt_reflection_sample_desc, reserved) == 12",
                 "__builtin_offsetof(rt_reflection_query, probe) == 12", "__builtin_offsetof(rt_reflection_query, roughness) == 28",
                 "__builtin_offsetof(rt_reflection_box, hi) == 16", "#define RT_REFLECTION_SAMPLE_PARALLAX 1u"):
        assert text in layout, text
    assert R.RT_REFLECTION_SAMPLE_PARALLAX == 1
    assert np.frombuffer(R.reflection_sample_desc(64, 4).tobytes(), np.uint32).tolist() == [64, 4, 0, 0, 0, 0, 0, 0]
    assert np.frombuffer(R.reflection_sample_desc(64, 4, parallax=True).tobytes(), np.uint32).tolist() == [64, 4, 1, 0, 0, 0, 0, 0]
    q = R.reflection_queries([1, 2, 3], [7, 0xffffffff], [[4, 5, 6], [0, 0, 1]], 0.5)
    assert q.view(np.float32).reshape(2, 8)[0].tolist() == [1, 2, 3, q.view(np.float32)[3], 4, 5, 6, 0.5]
    assert q.view(np.uint32).reshape(2, 8)[:, 3].tolist() == [7, 0xffffffff]
    # the reserved words of the bake's descriptor keep their meaning: none
    assert "uint32_t reserved[4];       /* 0 */" in layout


def test_the_documents_and_the_node_declarations(W):
    readme, integration, design = _read("README.md"), _read("INTEGRATION.md"), _read("DESIGN.md")
    assert "rt_sample_reflection" in readme and "sampleReflection" in readme
    assert "rt_sample_reflection" in integration and "(not built here)" not in integration
    assert "j = S - 1 - j" in integration and "i = S - 1 - i" in integration          # the seam fold, for bordered textures
    assert "### 4.1q" in design and "k_reflection_sample" in design
    not_built = design[design.index("### 4.1o"):design.index("### 4.1p")].split("**Not built:**")[1]
    for gone in ("a device sampler", "seam-aware", "parallax"):
        assert gone not in not_built, gone
    for stays in ("filtered importance sampling", "cube-map export", "BRDF-integration LUT"):
        assert stays in not_built, stays
    node = os.path.join(REPO, "webgpu-raytracer_amd", "node")
    dts, js, addon = _read(node, "index.d.ts"), _read(node, "index.js"), _read(node, "addon.c")
    for m in ("static reflectionSampleDesc(", "sampleReflection("):
        assert m in dts and m in js, m
    assert '{"rtSampleReflection", rtSampleReflection}' in addon and "native.rtSampleReflection(" in js


def refused(R):
    """(what, descriptor, n_probes, n) of every refusal that needs no array"""
    def desc(**kw):
        d = R.reflection_sample_desc(16, 3)
        for k, v in kw.items():
            d[k] = v
        return d
    out = [("size %d" % s, desc(size=s), 1, 1) for s in (0, 4, 7, 12, 24, 513, 1024)]
    out += [("levels %d" % l, desc(levels=l), 1, 1) for l in (0, 1)]
    out += [("smallest level", desc(levels=4), 1, 1), ("smallest level", desc(size=8, levels=3), 1, 1), ("levels 40", desc(levels=40), 1, 1)]
    out += [("flags %#x" % f, desc(flags=f), 1, 1) for f in (2, 3, 0x80000000)]
    for k in range(5):
        r = [0] * 5
        r[k] = 1
        out.append(("reserved[%d]" % k, desc(reserved=r), 1, 1))
    chain = int(R.reflection_level_offsets(512, 2)[-1])
    out.append(("n_probes 0", desc(), 0, 1))
    out.append(("n_probes * chain", desc(size=512, levels=2), ((1 << 31) + chain - 1) // chain, 1))
    out.append(("n 2^31", desc(), 1, 1 << 31))
    return out


def check_refusals(R, L, ctx):
    buf = np.zeros((512, 4), np.float32)                             # one chain of (16, 3) is 336 texels
    rec = np.zeros((2, 8), np.float32)
    B, P = buf.ctypes.data, rec.ctypes.data

    def calls(D, n_probes, n, chains=B, probes=P, boxes=P, queries=P, out=B):
        return [lambda: L.rt_sample_reflection(ctx, D, chains, n_probes, probes, boxes, queries, n, out),
                lambda: L.rt_sample_reflection_device(ctx, D, chains, n_probes, probes, boxes, queries, n, out)]

    def all_refuse(cs, what, message=b"reflection:"):
        for k, call in enumerate(cs):
            assert call() == RT_ERR_INVALID, (what, k)
            assert L.rt_last_error(ctx).startswith(message), (what, k, L.rt_last_error(ctx))

    for what, d, n_probes, n in refused(R):
        all_refuse(calls(d.ctypes.data, n_probes, n), what)
    all_refuse(calls(None, 1, 1), "NULL descriptor", b"reflection: NULL descriptor")
    # the descriptor comes first: a bad one is refused whatever else is wrong, and at n == 0 too
    bad = R.reflection_sample_desc(16, 1)
    all_refuse(calls(bad.ctypes.data, 0, 0, None, None, None, None, None), "bad descriptor, nothing else")
    # arrays: NULL, and for the device entry misaligned; probes and boxes only with the flag
    plain, par = R.reflection_sample_desc(16, 3), R.reflection_sample_desc(16, 3, parallax=True)
    for missing in ("chains", "queries", "out"):
        all_refuse(calls(plain.ctypes.data, 1, 1, **{missing: None}), missing, b"reflection: NULL array")
    for missing in ("probes", "boxes"):
        all_refuse(calls(par.ctypes.data, 1, 1, **{missing: None}), missing, b"reflection: NULL array")
    for off in ("chains", "queries", "out"):
        assert calls(plain.ctypes.data, 1, 1, **{off: B + 4})[1]() == RT_ERR_INVALID, off
        assert L.rt_last_error(ctx).startswith(b"reflection: device arrays must be 16-byte aligned"), off
    for off in ("probes", "boxes"):
        assert calls(par.ctypes.data, 1, 1, **{off: P + 8})[1]() == RT_ERR_INVALID, off
        assert L.rt_last_error(ctx).startswith(b"reflection: device arrays must be 16-byte aligned"), off


def test_refusals_without_a_context(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    check_refusals(R, L, None)
    # a good call without a context is still refused, by code alone
    d = R.reflection_sample_desc(16, 3)
    buf, rec = np.zeros((512, 4), np.float32), np.zeros((2, 8), np.float32)
    assert L.rt_sample_reflection(None, d.ctypes.data, buf.ctypes.data, 1, None, None, rec.ctypes.data, 1, buf.ctypes.data) == RT_ERR_INVALID
    assert L.rt_sample_reflection(None, d.ctypes.data, None, 1, None, None, None, 0, None) == RT_ERR_INVALID
    assert L.rt_sample_reflection_device(None, d.ctypes.data, None, 1, None, None, None, 0, None) == RT_ERR_INVALID


def test_argument_rules_on_a_context_without_a_scene(W):
    """The refusals again with a context; n == 0 is RT_OK whatever the arrays; and the sampler works with nothing uploaded
    and equals the model, with and without the flag - without it, with NULL probes and boxes.  Needs a device to make a
    context; without one the constructor's refusal is the result."""
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    if L.rt_device_count() == 0:
        with pytest.raises(W.RendererError):
            W.WebGPURenderer(0)
        return
    r = W.WebGPURenderer(0)
    try:
        check_refusals(R, L, r.ctx)
        plain, par = R.reflection_sample_desc(16, 3), R.reflection_sample_desc(16, 3, parallax=True)
        for d in (plain, par):
            assert L.rt_sample_reflection(r.ctx, d.ctypes.data, None, 0, None, None, None, 0, None) == RT_OK
            assert L.rt_sample_reflection_device(r.ctx, d.ctypes.data, None, 3, None, None, None, 0, None) == RT_OK
        chains = rs.hostile_chains(16, 3, 3)
        probes, boxes = rs.hostile_boxes(3)
        q = rs.hostile_queries(16, 3, 3)[:500]
        rs.check_words(r.sampleReflection(plain, chains, q), rs.model_sample(plain, chains, q), "empty context, plain")
        rs.check_words(r.sampleReflection(par, chains, q, probes, boxes), rs.model_sample(par, chains, q, probes, boxes),
                       "empty context, parallax")
        with pytest.raises(ValueError):
            r.sampleReflection(par, chains, q)                       # the binding asks for the probes and boxes itself
        with pytest.raises(ValueError):
            r.sampleReflection(plain, chains[:, :100], q)
    finally:
        r.destroy()
