"""The host's launch planner (csrc/launch_plan.h): which form of each kernel runs, how many threads a workgroup has, what it
stages in LDS and how much dynamic LDS the launch asks for, as functions of the scene's sizes and the context's knobs.  A
wrong answer there is a kernel that stages past its LDS allocation, or a scene that silently changes sides of a measured
line, so every row of tests/golden/launch_plan.json is evaluated through tests/model/launch_plan_check.cpp (host compiler
only, no GPU) and compared, field by field, with what the functions of rt_api.hip gave at the commit the table names, before
they moved into the planner.  The rows are sizes, not geometry: the bench scenes, the one-leaf test scenes, a size on each
line the planner draws and the smallest size over it, every knob off its default, and degenerate sizes.

The invariants below restate the byte sizes on their own, as the GPU tests of the one-leaf forms do: dyn is the wave blocks
plus exactly the arrays the plan stages, the workgroups a shape plans per CU fit the CU's LDS, and "all in LDS" is at most
64 KB."""
import ctypes
import json
import os

import pytest

import model_build

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "webgpu-raytracer_amd", "csrc")
SRC = os.path.join(HERE, "model", "launch_plan_check.cpp")
LIB = os.path.join(HERE, "model", "_build", "liblaunch_plan_check.so")

WAVE_QUEUE = 64 * 32 + 64 * 7 * 4 + 64 * 8     # RT_WORK_BYTES_PER_WAVE
PAIR_WAVE = WAVE_QUEUE + 7 * 64 * 8            # RT_PW_BYTES_PER_WAVE at RT_PW_STACK_K = 7
COL_PARK = 64 * 12                             # RT_PT_COL_BYTES_PER_WAVE

with open(os.path.join(HERE, "golden", "launch_plan.json")) as _f:
    TABLE = json.load(_f)
ROWS = TABLE["rows"]


@pytest.fixture(scope="module")
def planner():
    L = ctypes.CDLL(model_build.build(SRC, LIB, ["-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"]))
    L.lpc_fields.restype = ctypes.c_char_p
    L.lpc_eval.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    L.lpc_eval.restype = ctypes.c_int
    return L


def evaluate(L, row):
    inp = (ctypes.c_int64 * 14)(*(row["size"] + row["knobs"]))
    out = (ctypes.c_int64 * 128)()
    n = L.lpc_eval(inp, out)
    fields = L.lpc_fields().decode().split(",")
    assert n == len(fields)
    return dict(zip(fields, out[:n]))


def test_the_table_is_the_one_this_test_reads(planner):
    assert planner.lpc_fields().decode().split(",") == TABLE["fields"]
    assert TABLE["size_keys"] == ["n_nodes", "n_pairs", "n_tris", "n_inst", "n_verts", "n_lights", "n_tlas"]
    assert TABLE["knob_keys"] == ["lds_per_cu", "no_lds_staging", "treelet_cap", "walk", "wf_block", "wf_blocks_per_cu", "wf_rayreg"]
    assert TABLE["recorded_from"].startswith("95b3bdf")
    assert len({r["name"] for r in ROWS}) == len(ROWS) >= 100
    assert all(len(r["expect"]) == len(TABLE["fields"]) for r in ROWS)


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_plan_equals_the_recorded_one(planner, row):
    got = evaluate(planner, row)
    want = dict(zip(TABLE["fields"], row["expect"]))
    assert {k: (got[k], want[k]) for k in want if got[k] != want[k]} == {}


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_plan_invariants(planner, row):
    g = evaluate(planner, row)
    s = dict(zip(TABLE["size_keys"], row["size"]))
    k = dict(zip(TABLE["knob_keys"], row["knobs"]))
    n, p, t, i, v, l = (s[x] for x in ("n_nodes", "n_pairs", "n_tris", "n_inst", "n_verts", "n_lights"))
    tri_bytes = 48 * t
    node_inst_bytes = 64 * i + 16 * ((i + 3) // 4)
    shading_slots = 8 * t + 5 * t + v + (v + 1) // 2 + 9 * i + (l + 1) // 2 + 4 * l
    scene_bytes = 32 * n + tri_bytes + node_inst_bytes + 16 * shading_slots
    one_leaf_bytes = 32 * n + tri_bytes + node_inst_bytes + 16 * (8 * t + 2 * t + (l + 1) // 2 + 4 * l)

    for which in ("trace", "query"):
        f = lambda name: g["%s.%s" % (which, name)]
        waves = f("block") // 64
        if f("pairs"):
            staged = f("plan.stage_pairs") * 64 * p + f("plan.stage_tri") * tri_bytes + f("plan.stage_inst") * 96 * i
            assert f("dyn") == waves * PAIR_WAVE + staged
            all_staged = f("plan.stage_pairs") and f("plan.stage_tri") and f("plan.stage_inst")
        else:
            assert f("nplan.k_nodes") <= n
            staged = f("nplan.k_nodes") * 32 + f("nplan.stage_tri") * tri_bytes + f("nplan.stage_inst") * node_inst_bytes
            assert f("dyn") == waves * WAVE_QUEUE + staged
            all_staged = f("nplan.k_nodes") == n and f("nplan.stage_tri") and f("nplan.stage_inst")
        if f("trace_lds"):
            assert all_staged and f("block") == 256 and f("dyn") <= 64 * 1024 and g["fits_lds"]
        else:
            assert f("blocks_per_cu") >= 1
            assert f("dyn") * f("blocks_per_cu") <= k["lds_per_cu"]
        assert which == "trace" or f("block") == 256
        assert f("rq_form") == (3 + (not f("trace_lds")) if f("pairs") else (0 if f("trace_lds") else 1 + f("rayreg")))

    pp = lambda name: g["persistent_plan.%s" % name]
    if g["fits_lds"]:
        assert pp("dyn") == 4 * WAVE_QUEUE + scene_bytes <= 64 * 1024
        assert (pp("k_nodes"), pp("stage_tri"), pp("stage_inst")) == (n, 1, 1)
    else:
        assert pp("dyn") == 4 * WAVE_QUEUE + pp("k_nodes") * 32 + pp("stage_tri") * tri_bytes + pp("stage_inst") * node_inst_bytes
        assert pp("dyn") * 6 <= k["lds_per_cu"]
    assert g["one_leaf"] == (g["fits_lds"] and s["n_tlas"] == 1)

    for frames in (1, 2):
        for detailed in ("", ".detailed"):
            f = lambda name: g["persistent_shape.n%d%s.%s" % (frames, detailed, name)]
            assert (f("lds"), f("one_inst")) == (g["fits_lds"], g["one_leaf"])
            assert (f("plan.k_nodes"), f("plan.stage_tri"), f("plan.stage_inst")) == (pp("k_nodes"), pp("stage_tri"), pp("stage_inst"))
            assert f("waves") == (8 if f("wide") else 4)
            if f("wide"):
                assert f("one_inst") and frames > 1 and not detailed
                assert f("dyn") == 8 * (WAVE_QUEUE + COL_PARK) + one_leaf_bytes
                assert 3 * f("dyn") <= k["lds_per_cu"]
            elif f("one_inst"):
                assert f("dyn") == 4 * WAVE_QUEUE + one_leaf_bytes
            else:
                assert f("dyn") == pp("dyn")
            if f("lds"):
                assert f("dyn") <= 64 * 1024

    primary_bytes = 32 * n + tri_bytes + 64 * i + 128 * t
    if g["primary.lds"]:
        assert (g["primary.block"], g["primary.tiles_per_workgroup"], g["primary.dyn"]) == (256, 4, primary_bytes)
        assert primary_bytes <= 32 * 1024 and not k["no_lds_staging"]
    else:
        assert (g["primary.block"], g["primary.tiles_per_workgroup"], g["primary.dyn"]) == (64, 1, 0)
    if k["no_lds_staging"]:
        assert not g["fits_lds"] and g["trace.dyn"] == (g["trace.block"] // 64) * (PAIR_WAVE if g["trace.pairs"] else WAVE_QUEUE)


def test_planner_is_host_only():
    """launch_plan.h and lds_sizes.h compile without HIP: nothing of the runtime is included, directly or not."""
    for name in ("launch_plan.h", "lds_sizes.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "hip/" not in text and "__device__" not in text and "__global__" not in text, name
