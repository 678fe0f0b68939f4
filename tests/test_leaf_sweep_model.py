"""The leaf sweep against the reference's stackless walk, ray by ray, on the host (tests/model/leaf_sweep_model.cpp: the slab
and triangle tests of csrc/k_traverse.hip.h over include/mi355rt_math.h; the leaf records of csrc/scene_facts.h walk_facts).

For a BLAS whose stored boxes nest, a walk over the leaves alone, each box against the bound the leaves before it left, must
reach and hit the leaves the node walk reaches and hits: closest distance (bits), triangle, occlusion, the set of hit leaves
and the number of triangle tests are compared for 10^5 rays per scene whose reciprocal direction and origin term are finite.
The argument fails for a ray with a zero or denormal direction component (1 / 0 = inf, 0 * inf = NaN, and fmin / fmax drop
the NaN): such rays must raise the guard's predicate, and one hand-made ray shows the two walks apart without it."""
import ctypes
import os

import numpy as np
import pytest

import model_build
import random_scene

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "model", "leaf_sweep_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libleaf_sweep_model.so")
N_RAYS = 100_000
f32, u32 = np.float32, np.uint32
T_MIN, T_MAX = f32(1e-3), f32(1e30)


@pytest.fixture(scope="module")
def model():
    flags = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"]
    L = ctypes.CDLL(model_build.build(SRC, LIB, flags))
    vp = ctypes.c_void_p
    L.lsm_reference.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp]
    L.lsm_reference.restype = None
    L.lsm_sweep.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp]
    L.lsm_sweep.restype = ctypes.c_int
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def both_walks(L, blas, tri_geom, rays, root=0, cap=64):
    """(reference rows, sweep rows, leaves): rows of {bits(t), triangle, occluded, triangle tests, hit leaves, guard}"""
    blas = np.ascontiguousarray(blas, f32).reshape(-1, 8)
    tri_geom = np.ascontiguousarray(tri_geom, f32)
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 8)
    ref = np.zeros((len(rays), 6), u32)
    swp = np.zeros((len(rays), 6), u32)
    L.lsm_reference(_ptr(blas), root, _ptr(tri_geom), _ptr(rays), len(rays), _ptr(ref))
    leaves = L.lsm_sweep(_ptr(blas), len(blas), root, cap, _ptr(tri_geom), _ptr(rays), len(rays), _ptr(swp))
    return ref, swp, leaves


def triangle_records(b):
    """{v0, e1, e2} per triangle, 12 words: what k_prepare_tris makes of the vertices and the topology"""
    pos = np.asarray(b.vertices, f32).reshape(-1, 4)[:, :3]
    idx = np.asarray(b.mesh_topology, u32).reshape(-1, 20)[:, :3].astype(np.int64)
    g = np.zeros((len(idx), 12), f32)
    g[:, 0:3] = pos[idx[:, 0]]
    g[:, 4:7] = pos[idx[:, 1]] - pos[idx[:, 0]]
    g[:, 8:11] = pos[idx[:, 2]] - pos[idx[:, 0]]
    return g


def surface_rays(b, n, seed):
    """n rays that start on the scene's triangles (a point drawn in a triangle, moved a little along a random direction so
    that the triangle itself is a candidate) and, for a fifth of them, well outside the scene, aimed into it."""
    rng = np.random.default_rng(seed)
    pos = np.asarray(b.vertices, f32).reshape(-1, 4)[:, :3].astype(np.float64)
    idx = np.asarray(b.mesh_topology, u32).reshape(-1, 20)[:, :3].astype(np.int64)
    t = rng.integers(0, len(idx), n)
    u, v = rng.random(n), rng.random(n)
    flip = u + v > 1
    u[flip], v[flip] = 1 - u[flip], 1 - v[flip]
    p = pos[idx[t, 0]] + u[:, None] * (pos[idx[t, 1]] - pos[idx[t, 0]]) + v[:, None] * (pos[idx[t, 2]] - pos[idx[t, 0]])
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = p + d * rng.choice([1e-4, -1e-2, 1e-2], n)[:, None]
    far = rng.random(n) < 0.2
    size = np.abs(pos).max()
    o[far] = p[far] - d[far] * rng.uniform(2, 6, far.sum())[:, None] * size
    rays = np.zeros((n, 8), f32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, T_MIN, d, T_MAX
    short = rng.random(n) < 0.3   # shadow-like rays: a bound inside the scene
    rays[short, 7] = rng.uniform(0.05, 2.0, short.sum()).astype(f32) * f32(size)
    return rays


def scene(W, name):
    if name == "cornell":
        b = W.WorldBridge()
        b.loadScene("cornell")
        return b
    return random_scene.make(name, n_geoms=1, tris_per_geom=30 + 5 * name, n_instances=1)


@pytest.mark.parametrize("name", ["cornell", 1, 2, 3, 5])
def test_the_sweep_equals_the_reference_walk_on_finite_rays(W, model, name):
    b = scene(W, name)
    rays = surface_rays(b, N_RAYS + N_RAYS // 8, 100 + (0 if name == "cornell" else name))
    ref, swp, leaves = both_walks(model, b.blas, triangle_records(b), rays)
    n_leaves = int(np.count_nonzero(np.asarray(b.blas, f32).view(u32).reshape(-1, 8)[:, 7]))
    assert leaves == n_leaves, "the scene's BLAS is not sweepable"
    finite = ref[:, 5] == 0
    assert int(finite.sum()) >= N_RAYS
    assert np.array_equal(ref[:, 5], swp[:, 5])
    for col, what in enumerate(("closest t (bits)", "triangle", "occluded", "triangle tests", "hit leaves")):
        bad = np.flatnonzero(finite & (ref[:, col] != swp[:, col]))
        assert bad.size == 0, "%s differs for %d rays, first %s: reference %s, sweep %s" % (
            what, bad.size, rays[bad[0]].tolist(), ref[bad[0]].tolist(), swp[bad[0]].tolist())
    # the rays are worth the comparison: hits, misses, occluded and open ones, more than one hit leaf
    hit = ref[finite, 1] != 0xffffffff
    assert 0.2 < hit.mean() < 0.999 and 0.1 < ref[finite, 2].mean() < 0.999
    hit_leaves = np.unpackbits(ref[finite, 4].copy().view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1)
    assert (hit_leaves >= 3).mean() > 0.05


def test_cornell_has_eleven_leaves(W, model):
    b = scene(W, "cornell")
    _, _, leaves = both_walks(model, b.blas, triangle_records(b), surface_rays(b, 8, 1))
    assert leaves == 11
    assert both_walks(model, b.blas, triangle_records(b), surface_rays(b, 8, 1), cap=10)[2] == -1


def test_zero_and_denormal_direction_components_raise_the_guard(W, model):
    b = scene(W, "cornell")
    rays = surface_rays(b, 6000, 7)
    finite = rays.copy()
    k = np.arange(len(rays))
    values = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39], f32)   # 1 / x overflows for every one of them
    rays[k, 4 + k % 3] = values[k % 6]
    ref, swp, _ = both_walks(model, b.blas, triangle_records(b), rays)
    assert (ref[:, 5] == 1).all() and (swp[:, 5] == 1).all()
    # ... and the smallest components whose reciprocal is finite do not
    finite[k, 4 + k % 3] = np.array([3e-39, -3e-39, 1e-38, -1e-38, 1e-30, -1e-30], f32)[k % 6]
    ref, swp, _ = both_walks(model, b.blas, triangle_records(b), finite)
    with np.errstate(over="ignore", invalid="ignore"):
        inv = f32(1) / finite[:, 4:7]
        want = ~(np.isfinite(inv).all(axis=1) & np.isfinite(finite[:, 0:3] * inv).all(axis=1))
    assert np.array_equal(ref[:, 5] != 0, want) and not want.all()
    ok = ~want
    assert np.array_equal(ref[ok, :5], swp[ok, :5])


def test_a_ray_the_two_walks_disagree_on_without_the_guard(model):
    """A root box [-1, 1]^3 over two leaves, [0, 1] x [-1, 1]^2 and [-1, 0] x [-1, 1]^2, one triangle each in the plane z = 0.
    The ray starts at x = 0.5 with d.x = 0: inv_d.x = inf, o_inv_d.x = inf.  Root: the x slab gives -inf - inf = -inf and
    inf - inf = NaN, fmin and fmax drop the NaN, the far side is -inf: a miss, and the reference never sees a leaf.  First
    leaf: its face at x = 0 gives 0 * inf = NaN on the near side too, both x terms drop out and the y and z slabs pass: the
    sweep tests the triangle and hits it.  The nesting argument needs finite operands; the guard's predicate is raised."""
    blas = np.zeros((3, 8), f32)
    w = blas.view(u32)
    blas[0, 0:3], blas[0, 4:7] = (-1, -1, -1), (1, 1, 1)
    blas[1, 0:3], blas[1, 4:7] = (0, -1, -1), (1, 1, 1)
    blas[2, 0:3], blas[2, 4:7] = (-1, -1, -1), (0, 1, 1)
    w[:, 3] = [3, 2, 3]
    w[:, 7] = [0, 0 << 3 | 1, 1 << 3 | 1]
    tri = np.zeros((2, 12), f32)
    tri[0, 0:3], tri[0, 4:7], tri[0, 8:11] = (0.1, -0.5, 0), (0.8, 0, 0), (0.4, 1.4, 0)
    tri[1, 0:3], tri[1, 4:7], tri[1, 8:11] = (-0.9, -0.5, 0), (0.8, 0, 0), (0.4, 1.4, 0)
    ray = np.array([[0.5, 0.1, -0.5, T_MIN, 0.0, 0.001, 1.0, T_MAX]], f32)
    ref, swp, leaves = both_walks(model, blas, tri, ray)
    assert leaves == 2
    assert ref[0, 5] == 1 and swp[0, 5] == 1                      # the guard sends this ray's wave to the node walk
    assert ref[0, 1] == 0xffffffff and ref[0, 2] == 0 and ref[0, 4] == 0
    assert swp[0, 1] == 0 and swp[0, 2] == 1 and swp[0, 4] == 1   # what the sweep would have answered
    # the same ray with a direction the reciprocal of which is finite: both walks hit the triangle
    ray[0, 4] = 1e-6
    ref, swp, _ = both_walks(model, blas, tri, ray)
    assert ref[0, 5] == 0 and np.array_equal(ref, swp) and ref[0, 1] == 0
