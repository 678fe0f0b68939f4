"""The one-leaf-TLAS LDS form of the persistent kernel at the edge of its residency.  The product form is compiled for
RT_PT_ONE_INST_WAVES = 5 workgroups per CU (csrc/k_pathtrace.hip.h); the host sizes the grid with the occupancy query for
the launch's dynamic LDS (rt_api.hip), so a scene whose staged records leave room for fewer than five workgroups of the CU's
160 KiB simply gets fewer, and one that would allow more is held at five by registers.  One-leaf scenes on both sides of
the five-workgroup line, against the oracle, bit for bit (product build and counting build)."""
import pytest

import parity_util as pu
from parity_util import dyn_lds   # (tests that import it from here keep working)
import random_scene
from test_gpu_product_build import _check as check_product

pytestmark = pytest.mark.gpu

W_, H_, DEPTH, FRAMES = 64, 48, 8, (1, 2, 3)
LDS_PER_CU = pu.LDS_PER_CU
WAVE_QUEUES = 4 * pu.WAVE_QUEUE   # RT_WORK_BYTES_PER_WAVE x 4 waves


# (seed, triangles per geometry): workgroups per CU the LDS alone would allow
SCENES = {(1, 20): 6, (2, 50): 5, (2, 60): 4}


@pytest.mark.parametrize("counting", [False, True])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_one_leaf_lds_residency_parity(W, oracle_lib, scene, counting):
    b = random_scene.make(scene[0], n_geoms=1, tris_per_geom=scene[1], n_instances=1)
    assert len(b.tlas) // 8 == 1, "not a one-node TLAS"
    assert LDS_PER_CU // dyn_lds(b) == SCENES[scene]
    cpu = oracle_lib.OracleRenderer()
    pu.drive(cpu, W, b, W_, H_, DEPTH, 1, FRAMES, present=False)
    r = W.WebGPURenderer(0)
    try:
        r.setKernelVariant(1)          # the persistent kernel
        pu.drive(r, W, b, W_, H_, DEPTH, 1, FRAMES, present=False, detailed=counting)
        if counting:
            pu.assert_parity(r, cpu, check_output=False)
        else:
            check_product(r, cpu)
    finally:
        r.destroy()
