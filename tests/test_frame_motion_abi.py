"""Frame motion (RT_FRAME_TEMPORAL_MOTION, rt_set_frame_motion_ids, rt_read_frame_motion), the parts that need no GPU: the
symbols are declared, exported and bound; the flag has left the unknown bits of rt_set_frame_temporal; the refusals that need
no context carry their prefix; the report keeps its 48 bytes with the two new fields in what was left of its padding; the
scene library and the bridge hand out the TLAS builder's order; the documents state the feature.  The refusals that need a
context, the NOT_READY guard among them, are in tests/test_gpu_frame_motion.py."""
import ctypes
import inspect
import os
import re

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rt_set_frame_motion_ids", "rt_read_frame_motion")
METHODS = ("setFrameMotionIds", "readFrameMotion")
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
    code = open(W._build.RT_LIB, "rb").read()
    for k in (b"k_frame_motion", b"k_frame_motion_scatter", b"k_frame_temporal_motion"):
        assert k in code, k
    assert "THE FRAME MOTION RULE" in text and "RT_WORLD_INSTANCE_ORDER" in header
    # appended: the arrays before it keep their numbers
    enum = re.search(r"typedef enum rt_world_array \{(.*?)\}", header, flags=re.S).group(1)
    names = [n.strip().split("=")[0].strip() for n in enum.split(",") if n.strip()]
    assert names[-1] == "RT_WORLD_INSTANCE_ORDER" and names.index("RT_WORLD_DRAW_COMMANDS") == 8
    assert renderer.WebGPURenderer._WORLD_ARRAYS["instance_order"][0] == 9


def test_the_flag_is_no_longer_an_unknown_bit(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    assert R.RT_FRAME_TEMPORAL_MOTION == 2
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    assert re.search(r"#define\s+RT_FRAME_TEMPORAL_MOTION\s+2u", layout)
    d = R.frame_temporal_desc(plane_eps=0.02, motion=True, same_instance=True)
    assert int(d["flags"][0]) == 3 and int(R.frame_temporal_desc(plane_eps=0.02)["flags"][0]) == 0
    assert inspect.signature(R.frame_temporal_desc).parameters["motion"].default is False
    # without a context the flag is refused for the scene it needs - not as an unknown bit, which 4 still is
    for flags, want in ((2, b"frame temporal: RT_FRAME_TEMPORAL_MOTION needs an uploaded scene"), (3, b"frame temporal: RT_FRAME_TEMPORAL_MOTION"),
                        (4, b"frame temporal: unknown flag bit"), (6, b"frame temporal: unknown flag bit")):
        d = R.frame_temporal_desc(plane_eps=0.02)
        d["flags"] = flags
        L.rt_set_frame_denoise_form(None, 5)          # leaves another message behind
        assert L.rt_set_frame_temporal(None, d.ctypes.data) == RT_ERR_INVALID
        assert L.rt_last_error(None).startswith(want), (flags, L.rt_last_error(None))
    # the other checks of the descriptor still come first
    d = R.frame_temporal_desc(plane_eps=0.02, motion=True)
    d["max_history"] = 0
    assert L.rt_set_frame_temporal(None, d.ctypes.data) == RT_ERR_INVALID
    assert L.rt_last_error(None).startswith(b"frame temporal: max_history")


def test_the_ids_and_the_read_refuse_without_a_context(W):
    from webgpu_raytracer_amd import renderer as R
    L = R.load_library()
    ids = np.arange(3, dtype=np.uint32)
    L.rt_set_frame_denoise_form(None, 5)
    assert L.rt_set_frame_motion_ids(None, None, 3) == RT_ERR_INVALID
    assert L.rt_last_error(None).startswith(b"frame motion: NULL ids")
    L.rt_set_frame_denoise_form(None, 5)
    assert L.rt_set_frame_motion_ids(None, ids.ctypes.data, 3) == RT_ERR_INVALID
    assert L.rt_last_error(None).startswith(b"frame denoise: form must be"), "refused only for the missing context: no new message"
    out = np.zeros(8, np.float32)
    assert L.rt_read_frame_motion(None, out.ctypes.data, 1) == RT_ERR_INVALID


def test_the_report_stays_48_bytes(W):
    from webgpu_raytracer_amd import renderer as R
    P = R.RtFrameDenoiseReport
    assert ctypes.sizeof(P) == 48
    offs = {n: getattr(P, n).offset for n, _ in P._fields_}
    assert (offs["prepare_ms"], offs["pass_ms"], offs["finish_ms"], offs["passes"], offs["form"], offs["cache_hit"]) == (0, 4, 24, 28, 32, 37)
    assert (offs["temporal"], offs["temporal_ms"], offs["motion"], offs["motion_ms"]) == (38, 40, 39, 44)
    layout = open(os.path.join(REPO, "include", "mi355rt_layout.h")).read()
    assert "static_assert(sizeof(rt_frame_denoise_report) == 48" in layout
    body = re.search(r"typedef struct rt_frame_denoise_report \{(.*?)\} rt_frame_denoise_report;", layout, flags=re.S).group(1)
    assert re.search(r"uint8_t motion;", body) and re.search(r"float motion_ms;", body)
    assert "pad" not in re.sub(r"/\*.*?\*/", "", body, flags=re.S) and "reserved" not in re.sub(r"/\*.*?\*/", "", body, flags=re.S)


def test_the_bridge_hands_out_the_tlas_builders_order(W):
    b = W.WorldBridge()
    b.loadScene("instanced1000")
    order = b.instanceOrder
    n = len(b.instances) // 36
    assert order.dtype == np.uint32 and n > 1 and sorted(order.tolist()) == list(range(n))
    assert order.tolist() != list(range(n)), "the TLAS builder sorts: the order is not the identity"
    header = open(os.path.join(REPO, "include", "mi355scene.h")).read()
    assert re.search(r"const uint32_t\*\s+ms_world_instance_order\s*\(", header)
    # upload_scene passes it on, after the instances it belongs to
    calls = []

    class Recorder:
        def __getattr__(self, name):
            return lambda *a, **k: calls.append(name)

    W.upload_scene(Recorder(), b, 8, 8)
    assert "setFrameMotionIds" in calls and calls.index("setFrameMotionIds") > calls.index("updateBuffer")
    b.close()


def test_the_pixel_helper_inverts_the_camera(W):
    from webgpu_raytracer_amd import renderer as R
    import frame_denoise_util as fu
    u = fu.uniforms(8, 4, (0.01, -0.02))
    carry = np.zeros((4, 8, 8), np.float32)
    for y in range(4):
        for x in range(8):
            uu = (x + 0.5 + 0.01 * 8) / 8
            vv = 1.0 - (y + 0.5 - 0.02 * 4) / 4
            carry[y, x, :3] = np.array([-1 + 2 * uu, -1 + 2 * vv, -1.0]) * 3.0
    carry[..., 3:4].view(np.uint32)[:] = R.RT_FRAME_MOTION_MOVED
    carry[0, 0, 3:4].view(np.uint32)[:] = R.RT_FRAME_MOTION_UNTRACKED
    p = R.frame_motion_pixels(carry, u)
    assert p.shape == (4, 8, 2) and p.dtype == np.float64 and np.isnan(p[0, 0]).all()
    ys, xs = np.mgrid[0:4, 0:8]
    ok = ~np.isnan(p[..., 0])
    assert ok.sum() == 31 and np.abs(p[..., 0] - xs)[ok].max() < 1e-4 and np.abs(p[..., 1] - ys)[ok].max() < 1e-4


def test_documents_state_the_feature():
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "4.3d" in design
    sec = design[design.index("4.3d"):]
    for word in ("k_frame_motion", "Expectation", "Not built", "shading normal", "bytes per pixel"):
        assert word in sec, word
    readme = open(os.path.join(REPO, "README.md")).read()
    assert "RT_FRAME_TEMPORAL_MOTION" in readme
    integration = open(os.path.join(REPO, "INTEGRATION.md")).read()
    for word in ("setFrameMotionIds", "readFrameMotion", "instanceOrder"):
        assert word in integration, word
