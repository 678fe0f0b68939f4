"""The reference model of the radiance queries (tests/model/radiance_model.cpp) tied to the oracle.  With gbuffer_depth0 = 1
the model's bounce loop, fed with the pinhole rays of the oracle's frame and the pixel index as RNG stream id, IS the
oracle's ray_color: every pixel's radiance equals the oracle's accumulation after compute(1) bit for bit, a second frame
added to the first equals the two-frame accumulator, and the per-ray counters sum to the oracle's.  No GPU.
(`mixed` has a thin lens, which draws from the RNG before the path: it is not a tie scene.)"""
import numpy as np
import pytest

import parity_util as pu
import radiance_util as ru
import random_scene


def _tie(W, oracle_lib, bridge, w, h, depth, spp, frames, tag, min_hit=0.2, min_lit=0.1):
    m = ru.ModelRenderer()
    m.buildPipeline(depth, spp)
    W.upload_scene(m, bridge, w, h)
    # the G-buffer pass alone (MAX_DEPTH = 0 shades nothing): its node and triangle visits are not the path tracer's
    g = ru.ModelRenderer()
    g.buildPipeline(0, spp)
    W.upload_scene(g, bridge, w, h)
    acc = None
    for f in range(1, frames + 1):
        m.resetCounters()
        g.resetCounters()
        m.compute(f)
        g.compute(f)
        rays = m.cameraRays()
        assert np.array_equal(rays.view(np.uint32)[:, 7], np.arange(w * h, dtype=np.uint32))
        out, counts = m.traceRadiance(rays, depth, spp, f, gbuffer_depth0=True)
        col = out[:, :3].reshape(h, w, 3)
        want = m.readAccum()
        if f == 1:
            acc = np.concatenate([col, np.ones((h, w, 1), np.float32)], axis=2)
        else:
            acc = acc + np.concatenate([col, np.ones((h, w, 1), np.float32)], axis=2)     # f32 adds, as accumulate does
        assert acc.dtype == np.float32
        bad = (ru.u32(acc) != ru.u32(want)).any(axis=2)
        assert not bad.any(), (tag, "frame", f, "pixels that differ", int(bad.sum()))
        total, primary = m.getCounters(), g.getCounters()
        assert primary["extension_rays"] == 0 and primary["shaded_hits"] == 0
        sums = dict(zip(ru.COUNT_NAMES, (int(x) for x in counts.sum(axis=0))))
        for name in ("extension_rays", "shadow_rays", "shaded_hits"):
            assert sums[name] == total[name], (tag, f, name)
        for name in ("nodes_visited", "tris_tested"):
            assert sums[name] == total[name] - primary[name], (tag, f, name)
        # so that the tie cannot pass on darkness
        _, _, depth_plane = m.readGBuffer()
        assert (depth_plane < 1.0).mean() >= min_hit and (col.max(axis=2) > 0).mean() >= min_lit, tag
        # t of a shaded pixel is the recomputed depth-0 distance, of a background pixel the ray's t_max
        hit = (depth_plane < 1.0).reshape(-1)
        assert np.all(out[~hit, 3] == np.float32(1e30)) and np.all(out[hit, 3] < np.float32(1e30))


@pytest.mark.parametrize("scene", ["cornell", "special", "viewer_diamond", "glass_blob"])
@pytest.mark.parametrize("shape", [(64, 48, 4, 2), (40, 24, 8, 1), (33, 17, 1, 3)])
def test_model_with_gbuffer_depth0_is_the_oracle(W, oracle_lib, scene, shape):
    w, h, depth, spp = shape
    _tie(W, oracle_lib, pu.bridge_for(W, scene), w, h, depth, spp, 1, (scene, shape))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_on_random_textured_scenes_two_frames(W, oracle_lib, seed):
    b = random_scene.make(seed, with_textures=True)
    # (a random scene's camera looks at a cloud of small objects in front of nothing: fewer pixels are covered)
    _tie(W, oracle_lib, b, 48, 32, 6, 2, 2, ("random", seed), min_hit=0.05, min_lit=0.02)


def test_traced_depth0_differs_only_in_the_depth0_surface(W, oracle_lib):
    """gbuffer_depth0 = 0 on the same camera rays: same hits and misses, t within rounding of the recomputed one, one more
    extension ray per ray (the first segment), and a picture close to the oracle's (the G-buffer quantises normal and
    albedo, so not equal)."""
    b = pu.bridge_for(W, "cornell")
    m = ru.ModelRenderer()
    m.buildPipeline(4, 2)
    W.upload_scene(m, b, 64, 48)
    m.compute(1)
    rays = m.cameraRays()
    a, ca = m.traceRadiance(rays, 4, 2, 1, gbuffer_depth0=True)
    t, ct = m.traceRadiance(rays, 4, 2, 1, gbuffer_depth0=False)
    hit_a, hit_t = a[:, 3] < 1e30, t[:, 3] < 1e30
    assert (hit_a != hit_t).mean() < 0.01         # the G-buffer clips at z_near / z_far, a query at RT_T_MIN / t_max
    both = hit_a & hit_t
    assert np.allclose(a[both, 3], t[both, 3], rtol=1e-4)
    assert np.all(ct[:, 0] >= 1)
    # a light seen directly is the exception: its emission is its albedo (material type 3), which the unorm8 G-buffer clamps
    # to 1; leave those pixels out of the comparison of the means
    topo = np.asarray(b.mesh_topology).view(np.float32).reshape(-1, 20)
    _, nid, _ = m.readGBuffer()
    tri = nid.reshape(-1, 4).view(np.uint32)[:, 2]
    keep = both & (topo[np.where(both, tri, 0), 7] < 2.5)
    assert keep.sum() > 0.4 * keep.size
    mean_a, mean_t = float(a[keep, :3].mean()), float(t[keep, :3].mean())
    print("mean radiance, G-buffer depth 0:", mean_a, "traced depth 0:", mean_t)
    assert abs(mean_a - mean_t) < 0.1 * mean_a
    # max_depth = 0: t reported, nothing shaded
    z, cz = m.traceRadiance(rays, 0, 2, 1)
    assert np.array_equal(ru.u32(z[:, 3]), ru.u32(t[:, 3])) and not z[:, :3].any()
    assert np.all(cz[:, 0] == 1) and not cz[:, 1:3].any()
