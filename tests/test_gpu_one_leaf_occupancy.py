"""The one-leaf-TLAS LDS form of the persistent kernel at the edge of its residency.  The product form is compiled for
RT_PT_ONE_INST_WAVES = 5 workgroups per CU (csrc/k_pathtrace.hip.h); the host sizes the grid with the occupancy query for
the launch's dynamic LDS (rt_api.hip), so a scene whose staged records leave room for fewer than five workgroups of the CU's
160 KiB simply gets fewer, and one that would allow more is held at five by registers.  One-leaf scenes on both sides of
the five-workgroup line, against the oracle, bit for bit (product build and counting build)."""
import pytest

import parity_util as pu
import random_scene
from test_gpu_product_build import _check as check_product

pytestmark = pytest.mark.gpu

W_, H_, DEPTH, FRAMES = 64, 48, 8, (1, 2, 3)
LDS_PER_CU = 160 * 1024
WAVE_QUEUES = 4 * (64 * 32 + 64 * 7 * 4 + 64 * 8)   # RT_WORK_BYTES_PER_WAVE x 4 waves


def dyn_lds(b):
    """Dynamic LDS of one workgroup (rt_api.hip: wave queues + scene_lds_slots x 16 bytes)."""
    n_nodes = (len(b.tlas) + len(b.blas)) // 8
    n_tris, n_inst = len(b.mesh_topology) // 20, len(b.instances) // 36
    n_verts, n_lights = len(b.vertices) // 4, len(b.lights) // 2
    slots = (2 * n_nodes + 3 * n_tris + 4 * n_inst + (n_inst + 3) // 4 + 8 * n_tris + 5 * n_tris + n_verts +
             (n_verts + 1) // 2 + 9 * n_inst + (n_lights + 1) // 2 + 4 * n_lights)
    return WAVE_QUEUES + 16 * slots


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
