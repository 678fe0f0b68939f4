"""Frame denoise (rt_denoise_frame / rt_denoise_frame_device / rt_set_present_denoise / rt_set_frame_denoise_form /
rt_frame_denoise_stats), the parts that need no GPU: the symbols are declared, exported and bound; the descriptor is the
documented 32 bytes with its fields where the header puts them; the limits; every refusal of a descriptor is made before the
context is looked at, with the error code and a message that begins "frame denoise:" (without a context, what
rt_last_error(NULL) returns); the recorder takes denoise=.  The refusals that need a context are in
tests/test_gpu_frame_denoise.py."""
import ctypes
import inspect
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_denoise_frame", "rt_denoise_frame_device", "rt_set_present_denoise", "rt_set_frame_denoise_form",
           "rt_frame_denoise_stats")
METHODS = ("denoiseFrame", "denoiseFrameDevice", "setPresentDenoise", "setFrameDenoiseForm", "frameDenoiseStats")
KERNELS = (b"k_frame_prepare", b"k_frame_pass_lds", b"k_frame_pass_direct", b"k_frame_finish")
RT_ERR_INVALID = -1


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
    for m in METHODS:
        assert callable(getattr(W.WebGPURenderer, m)), m
    blob = open(W._build.RT_LIB, "rb").read()
    for k in KERNELS:
        assert k in blob, k
    assert "THE FRAME DENOISE RULE" in open(os.path.join(REPO, "include", "mi355rt.h")).read()


def test_descriptor_layout(W):
    from webgpu_raytracer_amd import renderer as R
    D = R.RtFrameDenoiseDesc
    assert ctypes.sizeof(D) == 32 and R.FRAME_DENOISE_DESC_DTYPE.itemsize == 32
    want = [("passes", 0), ("step", 4), ("flags", 8), ("normal_cos", 12), ("plane_eps", 16), ("sigma_lum", 20), ("reserved", 24)]
    assert [(n, getattr(D, n).offset) for n, _ in D._fields_] == want
    assert [(n, R.FRAME_DENOISE_DESC_DTYPE.fields[n][1]) for n in R.FRAME_DENOISE_DESC_DTYPE.names] == want
    assert D.reserved.size == 8
    assert ctypes.sizeof(R.RtFrameDenoiseReport) == 48
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    assert "static_assert(sizeof(rt_frame_denoise_desc) == 32" in layout
    assert "static_assert(sizeof(rt_frame_denoise_report) == 48" in layout
    assert re.search(r"#define\s+RT_FRAME_DENOISE_MAX_STEP\s+16u", layout)
    assert re.search(r"#define\s+RT_FRAME_DENOISE_DEMODULATE\s+1u", layout)
    assert re.search(r"#define\s+RT_FRAME_DENOISE_SAME_INSTANCE\s+2u", layout)
    body = re.search(r"typedef struct rt_frame_denoise_desc \{(.*?)\} rt_frame_denoise_desc;", layout, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.strip() for d in body.split(";") if d.strip()] == [
        "uint32_t passes", "uint32_t step", "uint32_t flags", "float normal_cos", "float plane_eps", "float sigma_lum",
        "uint32_t reserved[2]"]
    assert (R.RT_FRAME_DENOISE_MAX_STEP, R.RT_FRAME_DENOISE_DEMODULATE, R.RT_FRAME_DENOISE_SAME_INSTANCE) == (16, 1, 2)
    # RT_TIMER_COUNT stays what callers size their arrays by
    assert re.search(r"RT_TIMER_COUNT = 6\b", open(os.path.join(REPO, "include", "mi355rt.h")).read())


def test_the_helpers_take_the_documented_arguments(W):
    from webgpu_raytracer_amd import renderer as R
    d = R.frame_denoise_desc(plane_eps=0.02)
    assert d.dtype == R.FRAME_DENOISE_DESC_DTYPE and d.shape == (1,)
    assert (int(d["passes"][0]), int(d["step"][0]), int(d["flags"][0])) == (4, 1, 1)
    assert int(R.frame_denoise_desc(2, 4, plane_eps=0.1, demodulate=False, same_instance=True)["flags"][0]) == 2
    p = inspect.signature(R.frame_denoise_desc).parameters
    assert p["plane_eps"].kind is inspect.Parameter.KEYWORD_ONLY and p["plane_eps"].default is inspect.Parameter.empty
    from webgpu_raytracer_amd import recorder
    p = inspect.signature(recorder.FrameLoop.__init__).parameters
    assert p["denoise"].default is None


def _bad_descriptors(R):
    ok = dict(plane_eps=0.02)
    out = {}
    for name, change in (("passes 0", dict(passes=0)), ("passes 6", dict(passes=6)), ("step 0", dict(step=0)),
                         ("step 17", dict(step=17, passes=1)), ("2 << 4", dict(step=2, passes=5)), ("16 << 1", dict(step=16, passes=2)),
                         ("flag 4", dict(flags=4)), ("flag 2^31", dict(flags=1 << 31)), ("reserved 0", dict(reserved=(1, 0))),
                         ("reserved 1", dict(reserved=(0, 7)))):
        d = R.frame_denoise_desc(**ok)
        for k, v in change.items():
            d[k] = v
        out[name] = d
    return out


def test_every_descriptor_refusal_is_made_before_the_context(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    out = np.zeros((4, 4, 4), np.float32)
    calls = {"rt_denoise_frame": lambda p: L.rt_denoise_frame(None, p, out.ctypes.data, out.nbytes),
             "rt_denoise_frame_device": lambda p: L.rt_denoise_frame_device(None, p, out.ctypes.data),
             "rt_set_present_denoise": lambda p: L.rt_set_present_denoise(None, p)}
    for name, d in _bad_descriptors(R).items():
        for fn, call in calls.items():
            L.rt_set_frame_denoise_form(None, 0)          # leaves another message behind, or none
            assert call(d.ctypes.data) == RT_ERR_INVALID, (name, fn)
            msg = L.rt_last_error(None)
            assert msg.startswith(b"frame denoise:"), (name, fn, msg)
    for fn in ("rt_denoise_frame", "rt_denoise_frame_device"):
        assert calls[fn](None) == RT_ERR_INVALID and L.rt_last_error(None) == b"frame denoise: NULL descriptor"
    for form in (-1, 3):
        assert L.rt_set_frame_denoise_form(None, form) == RT_ERR_INVALID
        assert L.rt_last_error(None).startswith(b"frame denoise: form must be")
    # the limits: every legal (step, passes) pair passes the descriptor check and is refused only for the missing context
    good = R.frame_denoise_desc(plane_eps=0.02)
    for step in range(1, 17):
        for passes in range(1, 6):
            good["step"], good["passes"] = step, passes
            legal = (step << (passes - 1)) <= 16
            L.rt_set_frame_denoise_form(None, 5)          # a known message to tell "no new message" from a refusal
            assert calls["rt_denoise_frame"](good.ctypes.data) == RT_ERR_INVALID
            assert L.rt_last_error(None).startswith(b"frame denoise: step <<") != legal, (step, passes)
    for fn, call in calls.items():
        assert call(R.frame_denoise_desc(plane_eps=0.02).ctypes.data) == RT_ERR_INVALID      # no context
    assert L.rt_set_present_denoise(None, None) == RT_ERR_INVALID
    assert L.rt_frame_denoise_stats(None, None) == RT_ERR_INVALID


def test_documents_state_the_feature():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "4.3b" in design and "k_frame_pass_lds" in design and "Not built" in design
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "rt_denoise_frame" in readme
    assert "setPresentDenoise" in open(os.path.join(REPO, "INTEGRATION.md")).read()
