"""The launch of k_primary_visibility once the LDS form of an unstriped dispatch of a one-leaf scene stages the scene once
per workgroup and walks `rounds` tiles per wave (csrc/launch_plan.h primary_shape and primary_grid_x; the tile of (workgroup,
round, wave) is rtk::primary_tile of csrc/lds_sizes.h, the very function the kernel calls).  Evaluated through
tests/model/primary_rounds_check.cpp, host compiler only.

For 1, 3, 4, 5, 31, 32, 33, 8 100 and 8 100 x 32 tiles, as one frame and as a batch, at 64 KB and 160 KB of LDS per CU, with
`rounds` chosen by the planner and forced to 1, 2, 3, 8 and 16: every tile index below n_tiles is given to exactly one
(workgroup, round, wave), and nothing at or above 4 * rounds * grid is given out (what lies between n_tiles and that bound
the kernel's `tile_id < n_tiles` retires).  The planner never leaves a grid of many rounds fewer workgroups than twelve times
what the chip keeps resident (eight 256-thread workgroups per CU), and takes the largest power of two under its cap that
does so; a scene that does not take the LDS form, one with more than one TLAS node and a striped rank have one round
whatever the knob says; and the two-argument call returns the four fields it always did."""
import ctypes
import os

import numpy as np
import pytest

import model_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "model", "primary_rounds_check.cpp")
LIB = os.path.join(HERE, "model", "_build", "libprimary_rounds_check.so")

# rows of tests/golden/launch_plan.json
CORNELL = [22, 10, 36, 1, 72, 2, 1]                       # one TLAS node, the LDS form, 7 104 bytes
RANDOM_7 = [94, 45, 105, 6, 315, 70, 11]                  # 11 TLAS nodes, the LDS form, 21 872 bytes
SPONZA_LIKE = [161846, 80922, 263176, 1, 136172, 8, 1]    # the global-memory form
TILE_COUNTS = [1, 3, 4, 5, 31, 32, 33, 8100, 8100 * 32]
LDS_PER_CU = [64 * 1024, 160 * 1024]
N_CUS = 256
RESIDENT = 8 * N_CUS                                      # 256-thread workgroups of 8 waves-per-SIMD code on the chip
FLOOR = 12 * RESIDENT                                     # the fewest workgroups the planner leaves a grid of many rounds
KEYS = ("lds", "block", "tiles_per_workgroup", "dyn", "rounds", "tiles", "grid_x")


@pytest.fixture(scope="module")
def planner():
    L = ctypes.CDLL(model_build.build(SRC, LIB, ["-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"]))
    L.prc_shape.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    L.prc_shape.restype = ctypes.c_int
    L.prc_tiles.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    L.prc_tiles.restype = None
    return L


def shape(L, size, lds_per_cu, own_tiles, n_frames, forced=0, no_lds=0, striped=0):
    """(the shape of the dispatch, the shape the two-argument call returns)"""
    inp = (ctypes.c_int64 * 14)(*(size + [lds_per_cu, no_lds, forced, N_CUS, own_tiles, n_frames, striped]))
    out = (ctypes.c_int64 * 16)()
    assert L.prc_shape(inp, out) == 13
    return dict(zip(KEYS, out[:7])), dict(zip(KEYS[:6], out[7:13]))


def covered(L, grid_x, rounds):
    t = np.zeros(4 * rounds * grid_x, np.uint32)
    L.prc_tiles(grid_x, rounds, t.ctypes.data)
    return t


@pytest.mark.parametrize("forced", [0, 1, 2, 3, 8, 16], ids=lambda f: "auto" if f == 0 else "rounds%d" % f)
@pytest.mark.parametrize("n_frames", [1, 2, 32])
@pytest.mark.parametrize("lds_per_cu", LDS_PER_CU)
@pytest.mark.parametrize("n_tiles", TILE_COUNTS)
def test_every_tile_is_cast_once(planner, n_tiles, lds_per_cu, n_frames, forced):
    s, _ = shape(planner, CORNELL, lds_per_cu, n_tiles, n_frames, forced)
    assert s["lds"] == 1 and s["block"] == 256 and s["tiles_per_workgroup"] == 4 and s["dyn"] == 7104
    rounds, grid = s["rounds"], s["grid_x"]
    assert s["tiles"] == (rounds > 1)                       # one round: the form of one tile per wave
    if forced:
        assert rounds == forced
    assert rounds >= 1 and (forced or rounds & (rounds - 1) == 0)   # the knob takes any count, the planner powers of two
    assert grid == -(-n_tiles // (4 * rounds))
    t = covered(planner, grid, rounds)
    assert int(t.max()) < 4 * rounds * grid
    counts = np.bincount(t, minlength=4 * rounds * grid)
    assert (counts[:n_tiles] == 1).all()                    # each tile below n_tiles exactly once ...
    assert (counts == 1).all()                              # ... and no index twice beyond them either
    assert 4 * rounds * (grid - 1) < n_tiles                # no workgroup without a tile


@pytest.mark.parametrize("n_frames", [1, 2, 4, 32, 64])
@pytest.mark.parametrize("lds_per_cu", LDS_PER_CU)
@pytest.mark.parametrize("n_tiles", TILE_COUNTS + [32400, FLOOR * 4, FLOOR * 8, FLOOR * 8 - 1])
def test_the_chip_stays_full(planner, n_tiles, lds_per_cu, n_frames):
    s, _ = shape(planner, CORNELL, lds_per_cu, n_tiles, n_frames)
    rounds, grid = s["rounds"], s["grid_x"]
    cap = shape(planner, CORNELL, lds_per_cu, 1 << 24, 64)[0]["rounds"]   # what a dispatch of any size gets at most
    assert 1 <= rounds <= cap <= 16
    if rounds > 1:
        assert grid * n_frames >= FLOOR, (rounds, grid)
    # the largest power of two under the cap that does so: twice as many rounds would not
    if rounds < cap:
        assert (n_tiles * n_frames) // (8 * rounds) < FLOOR


def test_a_single_1080p_frame_and_the_headline_batch(planner):
    one, _ = shape(planner, CORNELL, 160 * 1024, 32400, 1)   # 240 x 135 tiles
    assert one["rounds"] == 1 and one["tiles"] == 0 and one["grid_x"] == 8100
    quarter, _ = shape(planner, CORNELL, 160 * 1024, 8100, 1)
    assert quarter["rounds"] == 1 and quarter["grid_x"] == 2025   # 8 rounds would be 254 workgroups for 256 CUs
    batch, _ = shape(planner, CORNELL, 160 * 1024, 32400, 32)
    assert batch["rounds"] == 8 and batch["tiles"] == 1 and batch["grid_x"] == 1013
    assert [shape(planner, CORNELL, 160 * 1024, 32400, n)[0]["rounds"] for n in (2, 4, 8, 16, 64)] == [1, 1, 2, 4, 8]


@pytest.mark.parametrize("forced", [0, 2, 16])
@pytest.mark.parametrize("n_tiles", TILE_COUNTS)
@pytest.mark.parametrize("lds_per_cu", LDS_PER_CU)
def test_one_round_outside_the_form_of_many_tiles(planner, lds_per_cu, n_tiles, forced):
    for size, no_lds in ((SPONZA_LIKE, 0), (CORNELL, 1)):   # not the LDS form
        s, _ = shape(planner, size, lds_per_cu, n_tiles, 32, forced, no_lds)
        assert s == {"lds": 0, "block": 64, "tiles_per_workgroup": 1, "dyn": 0, "rounds": 1, "tiles": 0, "grid_x": n_tiles}
    grid = -(-n_tiles // 4)
    s, _ = shape(planner, RANDOM_7, lds_per_cu, n_tiles, 32, forced)   # the LDS form, a TLAS of more than one node
    assert s == {"lds": 1, "block": 256, "tiles_per_workgroup": 4, "dyn": 21872, "rounds": 1, "tiles": 0, "grid_x": grid}
    s, _ = shape(planner, CORNELL, lds_per_cu, n_tiles, 32, forced, striped=1)   # a striped rank
    assert s == {"lds": 1, "block": 256, "tiles_per_workgroup": 4, "dyn": 7104, "rounds": 1, "tiles": 0, "grid_x": grid}


@pytest.mark.parametrize("lds_per_cu", LDS_PER_CU)
def test_the_two_argument_call_is_todays(planner, lds_per_cu):
    four = KEYS[:4]
    for forced in (0, 16):
        for size, want in ((CORNELL, (1, 256, 4, 7104)), (RANDOM_7, (1, 256, 4, 21872)), (SPONZA_LIKE, (0, 64, 1, 0))):
            _, two = shape(planner, size, lds_per_cu, 8100, 32, forced)
            assert tuple(two[k] for k in four) == want
            if not forced:
                assert two["rounds"] == 1
