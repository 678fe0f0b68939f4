"""One context, the same kernels prepared for one dynamic-LDS size, then another, then the first again.  The host keeps one
prepared entry per kernel (rt_api.hip resident_blocks): a launch at another size sets the kernel's dynamic-LDS attribute
again, so going back to a size seen before must prepare again as well.  Scenes A (cornell) and B (a 20-triangle random
scene) are both one-leaf scenes that fit LDS: they take the same forms of the persistent kernel, the ray query and the
radiance query at different sizes.  One renderer and one oracle go through A, B, A; after each upload the frames (a batch
of two: the wide form; one alone: the 256-thread form) equal the oracle bit for bit, the ray queries equal the oracle's
traversal loop, the radiance query equals the radiance model, and what A gave the second time equals the first."""
import numpy as np
import pytest

import parity_util as pu
import radiance_util as ru
import random_scene
import ray_query_util as rq
from test_gpu_one_leaf_occupancy import dyn_lds
from test_gpu_product_build import _check as check_product

pytestmark = pytest.mark.gpu

W_, H_, DEPTH = 64, 48, 8
RD_DEPTH, RD_SPP = 4, 2
N_A, N_B = 320, 192      # rays_for + _random_rays: 512 rays per query


def _refs(W, oracle_lib, b):
    """The scene's rays and what the references say about them, computed once and left unchanged."""
    oracle = rq.oracle_for(W, oracle_lib, b)
    closest, shadow = rq.scene_rays(b, False, N_A, N_B), rq.scene_rays(b, True, N_A, N_B)
    assert closest.shape[0] == shadow.shape[0] == 512
    rad_rays = ru.with_pads(rq.to_rt_rays(closest))
    rad_ref, _ = ru.model_for(W, b).traceRadiance(rad_rays, RD_DEPTH, RD_SPP, ru.SEED)
    refs = dict(closest=closest, shadow=shadow, rad_rays=rad_rays, rad_ref=rad_ref,
                closest_ref=oracle.traceRays(closest)[0], shadow_ref=oracle.traceRays(shadow, any_hit=True)[0])
    for a in refs.values():
        a.setflags(write=False)
    return refs


def test_same_kernels_at_size_a_then_b_then_a(W, oracle_lib, gpu_renderer):
    a = pu.bridge_for(W, "cornell")
    b = random_scene.make(1, n_geoms=1, tris_per_geom=20, n_instances=1)
    for s in (a, b):
        assert len(s.tlas) // 8 == 1, "not a one-node TLAS"
    assert dyn_lds(a) != dyn_lds(b)
    refs = {"A": _refs(W, oracle_lib, a), "B": _refs(W, oracle_lib, b)}
    # parity must not pass on emptiness: the references' own hit and light counts on A's rays; B, 20 triangles in a box the
    # rays fill, is hit by few of them and is here for its size
    assert (refs["A"]["closest_ref"][:, 1] >= 0).sum() >= 50 and (refs["A"]["rad_ref"][:, :3].max(axis=1) > 0).sum() >= 50
    assert (refs["B"]["closest_ref"][:, 1] >= 0).any()
    gpu, cpu, steps = gpu_renderer, oracle_lib.OracleRenderer(), []
    for r in (gpu, cpu):
        r.buildPipeline(DEPTH, 1)
    gpu.setCounting(False)
    for step, (name, s) in enumerate((("A", a), ("B", b), ("A", a))):
        tag = "step %d, scene %s" % (step + 1, name)
        for r in (gpu, cpu):
            W.upload_scene(r, s, W_, H_)
            r.resetCounters()
        ref = refs[name]
        # frames 1 and 2 as a batch, frame 3 alone
        gpu.computeBatch([1, 2])
        wide = gpu.debugPtLaunch()
        gpu.compute(3)
        narrow = gpu.debugPtLaunch()
        for f in (1, 2, 3):
            cpu.compute(f)
        gpu.sync()
        print(tag, "batch", wide, "single frame", narrow)
        assert wide["threads"] == 512 and narrow["threads"] == 256, (tag, wide, narrow)
        check_product(gpu, cpu)
        # queries
        hits = gpu.traceRays(rq.to_rt_rays(ref["closest"]), t_min=rq.T_MIN)
        rq.check_closest(hits, ref["closest"], ref["closest_ref"], tag)
        occluded = gpu.traceRays(rq.to_rt_rays(ref["shadow"]), any_hit=True, t_min=rq.T_MIN)
        rq.check_any(occluded, ref["shadow_ref"], tag)
        rad = gpu.traceRadiance(ref["rad_rays"], RD_DEPTH, RD_SPP, ru.SEED)
        ru.check_against_model(rad, ref["rad_ref"], tag)
        steps.append(dict(wide=wide["dyn_lds"], narrow=narrow["dyn_lds"], hits=hits.view(np.uint32).copy(),
                          occluded=occluded.view(np.uint32).copy(), rad=ru.result_words(rad).copy()))
    for form in ("wide", "narrow"):
        assert steps[0][form] != steps[1][form], (form, steps[0][form], steps[1][form])
        assert steps[0][form] == steps[2][form], (form, steps[0][form], steps[2][form])
    for what in ("hits", "occluded", "rad"):
        assert np.array_equal(steps[0][what], steps[2][what]), what
