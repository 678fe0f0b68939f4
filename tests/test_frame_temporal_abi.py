"""Frame temporal (rt_set_frame_temporal / rt_reset_frame_history / rt_read_frame_history), the parts that need no GPU: the
symbols are declared, exported and bound; the descriptor is the documented 32 bytes with its fields where the header puts them;
the report keeps its 48 bytes with the two new fields in the former padding; every refusal of a descriptor is made before the
context is looked at, with the error code and a message that begins "frame temporal:" (without a context, what
rt_last_error(NULL) returns); the recorder takes temporal= only beside denoise=; the documents state the feature.  The refusals
that need a context are in tests/test_gpu_frame_temporal.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_set_frame_temporal", "rt_reset_frame_history", "rt_read_frame_history")
METHODS = ("setFrameTemporal", "resetFrameHistory", "readFrameHistory")
RT_ERR_INVALID = -1


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
    for m in METHODS:
        assert callable(getattr(W.WebGPURenderer, m)), m
    assert b"k_frame_temporal" in open(W._build.RT_LIB, "rb").read()
    assert "THE FRAME TEMPORAL RULE" in text
    # the temporal half has left the "Not built" text of the frame denoise rule
    rule = text[text.index("THE FRAME DENOISE RULE"):text.index("int rt_denoise_frame(")]
    assert "Not built: temporal" not in rule and "Not built: separate treatment" in rule


def test_descriptor_and_report_layout(W):
    from webgpu_raytracer_amd import renderer as R
    D = R.RtFrameTemporalDesc
    assert ctypes.sizeof(D) == 32 and R.FRAME_TEMPORAL_DESC_DTYPE.itemsize == 32
    want = [("flags", 0), ("max_history", 4), ("var_history", 8), ("normal_cos", 12), ("plane_eps", 16), ("reserved", 20)]
    assert [(n, getattr(D, n).offset) for n, _ in D._fields_] == want
    assert [(n, R.FRAME_TEMPORAL_DESC_DTYPE.fields[n][1]) for n in R.FRAME_TEMPORAL_DESC_DTYPE.names] == want
    assert D.reserved.size == 12
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    assert "static_assert(sizeof(rt_frame_temporal_desc) == 32" in layout
    assert re.search(r"#define\s+RT_FRAME_TEMPORAL_MAX_HISTORY\s+256u", layout)
    assert re.search(r"#define\s+RT_FRAME_TEMPORAL_SAME_INSTANCE\s+1u", layout)
    body = re.search(r"typedef struct rt_frame_temporal_desc \{(.*?)\} rt_frame_temporal_desc;", layout, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.strip() for d in body.split(";") if d.strip()] == [
        "uint32_t flags", "uint32_t max_history", "uint32_t var_history", "float normal_cos", "float plane_eps",
        "uint32_t reserved[3]"]
    assert (R.RT_FRAME_TEMPORAL_MAX_HISTORY, R.RT_FRAME_TEMPORAL_SAME_INSTANCE) == (256, 1)
    # the report: 48 bytes still, every old field where it was, the new ones in the first pad byte and the first reserved word
    P = R.RtFrameDenoiseReport
    assert ctypes.sizeof(P) == 48
    assert "static_assert(sizeof(rt_frame_denoise_report) == 48" in layout
    offs = {n: getattr(P, n).offset for n, _ in P._fields_}
    assert (offs["prepare_ms"], offs["pass_ms"], offs["finish_ms"], offs["passes"], offs["form"], offs["cache_hit"]) == (0, 4, 24, 28, 32, 37)
    assert (offs["temporal"], offs["temporal_ms"]) == (38, 40)
    body = re.search(r"typedef struct rt_frame_denoise_report \{(.*?)\} rt_frame_denoise_report;", layout, flags=re.S).group(1)
    assert re.search(r"uint8_t temporal;", body) and re.search(r"float temporal_ms;", body)
    assert re.search(r"RT_TIMER_COUNT = 6\b", open(os.path.join(REPO, "include", "mi355rt.h")).read())


def test_the_helpers_take_the_documented_arguments(W):
    from webgpu_raytracer_amd import renderer as R
    d = R.frame_temporal_desc(plane_eps=0.02)
    assert d.dtype == R.FRAME_TEMPORAL_DESC_DTYPE and d.shape == (1,)
    assert (int(d["flags"][0]), int(d["max_history"][0]), int(d["var_history"][0])) == (0, 32, 4)
    assert abs(float(d["normal_cos"][0]) - 0.9) < 1e-6 and abs(float(d["plane_eps"][0]) - 0.02) < 1e-8
    assert int(R.frame_temporal_desc(8, 2, plane_eps=0.1, same_instance=True)["flags"][0]) == 1
    p = inspect.signature(R.frame_temporal_desc).parameters
    assert p["plane_eps"].kind is inspect.Parameter.KEYWORD_ONLY and p["plane_eps"].default is inspect.Parameter.empty
    with pytest.raises(TypeError):
        R.frame_temporal_desc()


class _Recorded:
    def __init__(self):
        self.calls = []

    def setPresentDenoise(self, d):
        self.calls.append(("setPresentDenoise", d))

    def setFrameTemporal(self, t):
        self.calls.append(("setFrameTemporal", t))


def test_the_recorder_takes_temporal_only_beside_denoise(W):
    from webgpu_raytracer_amd import recorder
    p = inspect.signature(recorder.FrameLoop.__init__).parameters
    assert p["temporal"].default is None and p["denoise"].default is None
    r = _Recorded()
    recorder.FrameLoop(r, None, 8, 8)
    assert r.calls == []
    d, t = dict(plane_eps=0.02), dict(plane_eps=0.02, max_history=8)
    recorder.FrameLoop(r, None, 8, 8, denoise=d, temporal=t)
    assert r.calls == [("setPresentDenoise", d), ("setFrameTemporal", t)]
    r = _Recorded()
    with pytest.raises(ValueError, match="temporal= needs denoise="):
        recorder.FrameLoop(r, None, 8, 8, temporal=t)
    assert r.calls == []


def test_every_descriptor_refusal_is_made_before_the_context(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    for name, change in (("flag 2", dict(flags=2)), ("flag 2^31", dict(flags=1 << 31)), ("reserved 0", dict(reserved=(1, 0, 0))),
                         ("reserved 1", dict(reserved=(0, 7, 0))), ("reserved 2", dict(reserved=(0, 0, 1 << 31))),
                         ("max_history 0", dict(max_history=0)), ("max_history 257", dict(max_history=257)),
                         ("max_history 2^32 - 1", dict(max_history=0xffffffff)), ("var_history 0", dict(var_history=0))):
        d = R.frame_temporal_desc(plane_eps=0.02)
        for k, v in change.items():
            d[k] = v
        L.rt_set_frame_denoise_form(None, 5)          # leaves another message behind
        assert L.rt_set_frame_temporal(None, d.ctypes.data) == RT_ERR_INVALID, name
        msg = L.rt_last_error(None)
        assert msg.startswith(b"frame temporal:"), (name, msg)
    # the limits pass the descriptor check and are refused only for the missing context: no new message
    for change in (dict(max_history=1), dict(max_history=256), dict(var_history=0xffffffff), dict(flags=1),
                   dict(normal_cos=float("nan"), plane_eps=float("nan"))):
        d = R.frame_temporal_desc(plane_eps=0.02)
        for k, v in change.items():
            d[k] = v
        L.rt_set_frame_denoise_form(None, 5)
        assert L.rt_set_frame_temporal(None, d.ctypes.data) == RT_ERR_INVALID
        assert L.rt_last_error(None).startswith(b"frame denoise: form must be"), change
    assert L.rt_set_frame_temporal(None, None) == RT_ERR_INVALID
    assert L.rt_reset_frame_history(None) == RT_ERR_INVALID
    n = ctypes.c_uint32(7)
    assert L.rt_read_frame_history(None, None, None, 0, ctypes.addressof(n)) == RT_ERR_INVALID and n.value == 7


def test_documents_state_the_feature():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "4.3c" in design and "k_frame_temporal" in design
    sec = design[design.index("4.3c"):]
    for word in ("Not built", "Expectation", "frame_temporal_rate.txt", "3 x 3 search", "clamping"):
        assert word in sec, word
    b = design[design.index("4.3b"):design.index("4.3c")]
    assert not re.search(r"Not built[^\n]*temporal reprojection", b)
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "rt_set_frame_temporal" in readme
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for word in ("setFrameTemporal", "resetFrameHistory", "readFrameHistory"):
        assert word in integration, word
    assert os.path.exists(os.path.join(REPO, "tools", "frame_temporal_time.py"))
