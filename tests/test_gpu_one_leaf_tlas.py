"""The persistent kernel's LDS form on scenes whose TLAS is one node, a leaf (csrc/k_traverse.hip.h traverse<.., ONE_INST>:
the first node step tests the TLAS leaf, every later one runs without the TLAS half of the step).  Against the oracle,
bit for bit: accumulation, G-buffer, uniforms and all six counters of the counting build, and the product build."""
import pytest

import odd_bvh
import parity_util as pu
import random_scene
from test_gpu_product_build import _check as check_product

pytestmark = pytest.mark.gpu

W_, H_, DEPTH, FRAMES = 64, 48, 8, (1, 2, 3)
SCENES = ["cornell", "special", "random1", "random2", "random3", "tiny_trees", "empty_leaves"]


def _bridge(W, name):
    if name.startswith("random"):
        b = random_scene.make(int(name[-1]), n_instances=1)
    elif name in ("tiny_trees", "empty_leaves"):
        b = odd_bvh.make(3, ("tiny_trees",)) if name == "tiny_trees" else \
            odd_bvh.make(2, ("empty_leaves",), n_instances=1)
    else:
        b = pu.bridge_for(W, name)
    assert len(b.tlas) // 8 == 1, "not a one-node TLAS"
    return b


@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("counting", [True, False])
@pytest.mark.parametrize("scene", SCENES)
def test_one_leaf_tlas_parity(W, oracle_lib, scene, counting, spp):
    b = _bridge(W, scene)
    cpu = oracle_lib.OracleRenderer()
    pu.drive(cpu, W, b, W_, H_, DEPTH, spp, FRAMES, present=False)
    r = W.WebGPURenderer(0)
    try:
        r.setKernelVariant(1)          # the persistent kernel
        pu.drive(r, W, b, W_, H_, DEPTH, spp, FRAMES, present=False, detailed=counting)
        if counting:
            pu.assert_parity(r, cpu, check_output=False)
        else:
            check_product(r, cpu)
    finally:
        r.destroy()
