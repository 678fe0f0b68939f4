"""The one-leaf-TLAS LDS form in 512-thread workgroups (k_pathtrace_persistent_wide, csrc/k_pathtrace.hip.h).  The host takes
it for the product build when three workgroups, each with eight wave queues, eight waves' parked sample sums and one staged
copy of the scene, fit the CU's 160 KiB of LDS (rt_api.hip), and keeps the 256-thread form otherwise.  One-leaf scenes on
both sides of that line, batches, several samples per pixel, stripes and odd image shapes, against the oracle, bit for bit
(product build); the shape of each launch (rt_debug_pt_launch) shows which form the host took.  The host takes the wide form
for batched dispatches only (more than one frame), so a batch of 1 checks that it keeps the 256-thread form there."""
import numpy as np
import pytest

import parity_util as pu
import random_scene
from test_gpu_one_leaf_occupancy import dyn_lds
from test_gpu_product_build import RAYS, _check as check_product, _run

pytestmark = pytest.mark.gpu

LDS_PER_CU, WAVE_QUEUE, COL_PARK = pu.LDS_PER_CU, pu.WAVE_QUEUE, pu.COL_PARK
DEPTH, FRAMES = 8, (1, 2, 3)

# scene -> whether the host takes the wide form (random one-leaf scenes: (seed, triangles))
SCENES = {"cornell": True, (1, 30): True, (2, 50): False}


def _launch_is(r, wide, tickets):
    """The last persistent launch: the wide form at 3 workgroups per CU (6 waves per SIMD), else 256 threads; never more
    waves than tickets."""
    L = r.debugPtLaunch()
    assert L["threads"] == (512 if wide else 256), L
    if wide:
        assert L["per_cu"] == 3, L
    assert L["workgroups"] >= 1 and (L["workgroups"] - 1) * L["threads"] // 64 < tickets, L


def _bridge(W, name):
    b = pu.bridge_for(W, name) if name == "cornell" else random_scene.make(name[0], n_geoms=1, tris_per_geom=name[1],
                                                                           n_instances=1)
    assert len(b.tlas) // 8 == 1, "not a one-node TLAS"
    wide_dyn = dyn_lds(b) + 4 * WAVE_QUEUE + 8 * COL_PARK   # dyn_lds counts four wave queues
    assert (wide_dyn <= LDS_PER_CU // 3) == SCENES[name]
    return b


def _compare(W, oracle_lib, b, w, h, spp, frames, batch, stripes=None, wide=True):
    cpu = oracle_lib.OracleRenderer()
    if stripes:
        cpu.setStripes(*stripes)
    pu.drive(cpu, W, b, w, h, DEPTH, spp, frames, present=False)
    r = W.WebGPURenderer(0)
    try:
        if stripes:
            r.setStripes(*stripes)
        _run(W, r, b, w, h, DEPTH, spp, frames, batch, 1)
        tiles_x, tile_rows = (w + 7) // 8, (h + 7) // 8
        last_batch = len(frames) - (len(frames) - 1) // batch * batch
        _launch_is(r, wide and last_batch > 1, tiles_x * tile_rows * last_batch)
        if not stripes:
            check_product(r, cpu)
            return r.readAccum()
        # a rank's own rows (test_gpu_shapes.py test_stripes_at_odd_shapes)
        rows, rank, count = stripes
        owned = (np.arange(h) // rows) % count == rank
        part, want = r.readAccum(), cpu.readAccum()
        assert not part[~owned].any(), "rank %d wrote outside its rows" % rank
        assert np.array_equal(pu.bits(part[owned]), pu.bits(want[owned])), \
            pu.describe_mismatch("rank %d owned rows" % rank, part[owned], want[owned])
        gc, cc = r.getCounters(), cpu.getCounters()
        assert {k: gc[k] for k in RAYS} == {k: cc[k] for k in RAYS}
        return part
    finally:
        r.destroy()


@pytest.mark.parametrize("batch", [1, 2, 3])
@pytest.mark.parametrize("scene", sorted(SCENES, key=str))
def test_wide_form_batches(W, oracle_lib, scene, batch):
    _compare(W, oracle_lib, _bridge(W, scene), 64, 48, 1, FRAMES, batch, wide=SCENES[scene])
    if batch == 2:   # frames (1, 2) as one batch, then frame 3 alone: the last launch must be the wide form
        _compare(W, oracle_lib, _bridge(W, scene), 64, 48, 1, FRAMES[:2], batch, wide=SCENES[scene])


@pytest.mark.parametrize("scene", sorted(SCENES, key=str))
def test_wide_form_four_spp(W, oracle_lib, scene):
    _compare(W, oracle_lib, _bridge(W, scene), 40, 24, 4, (1, 2), 2, wide=SCENES[scene])


@pytest.mark.parametrize("w,h", [(1, 1), (65, 1), (9, 67)])
@pytest.mark.parametrize("batch", [1, 3])
def test_wide_form_odd_shapes(W, oracle_lib, w, h, batch):
    """1x1 is one ticket for a grid of eight waves; 9x67 is 18 tickets per frame: most waves get no tile or one."""
    _compare(W, oracle_lib, _bridge(W, "cornell"), w, h, 1, FRAMES, batch)


@pytest.mark.parametrize("rows", [1, 8])
def test_wide_form_three_ranks(W, oracle_lib, rows):
    b = _bridge(W, "cornell")
    w, h, count = 21, 67, 3
    total = None
    for rank in range(count):
        part = _compare(W, oracle_lib, b, w, h, 1, (1, 2), 2, stripes=(rows, rank, count))
        total = part if total is None else total + part
    full = oracle_lib.OracleRenderer()
    pu.drive(full, W, b, w, h, DEPTH, 1, (1, 2), present=False)
    assert np.array_equal(pu.bits(total), pu.bits(full.readAccum())), \
        pu.describe_mismatch("stripe sum", total, full.readAccum())
