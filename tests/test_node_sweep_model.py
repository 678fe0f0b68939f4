"""The node sweep against the reference's stackless walk, ray by ray, on the host (tests/model/node_sweep_model.cpp: the node
records of csrc/scene_facts.h walk_facts, one word of state per ray, the slab and triangle tests of csrc/k_traverse.hip.h
over include/mi355rt_math.h).

The node sweep is the walk a wave of a sweep form takes when one of its rays has a non-finite reciprocal direction or origin
term (csrc/k_traverse.hip.h traverse_leaves).  On a canonical pre-order tree it visits, per ray, the reference's nodes in the
reference's order against the reference's bounds, so it must give the reference's closest distance (bits), triangle,
occlusion, hit leaves and number of triangle tests for EVERY ray: zero, negative-zero and denormal direction components,
origins on box faces, box faces at 0.  No ray is left out of a comparison here, and no mismatch is allowed."""
import ctypes
import os

import numpy as np
import pytest

import model_build
import sweep_trees
from test_leaf_sweep_model import T_MAX, T_MIN, surface_rays

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "model", "node_sweep_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libnode_sweep_model.so")
f32, u32 = np.float32, np.uint32
HOSTILE = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39], f32)   # 1 / x overflows for every one of them
COLUMNS = ("closest t (bits)", "triangle", "occluded", "triangle tests", "hit leaves", "non-finite operand")


@pytest.fixture(scope="module")
def model():
    flags = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"]
    L = ctypes.CDLL(model_build.build(SRC, LIB, flags))
    vp = ctypes.c_void_p
    L.lsm_reference.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp]
    L.lsm_reference.restype = None
    for fn in (L.lsm_sweep, L.nsm_sweep):
        fn.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp]
        fn.restype = ctypes.c_int
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def walks(L, blas, tri_geom, rays, cap=16):
    """(reference rows, node-sweep rows, leaf-sweep rows, nodes): rows as lsm_reference writes them"""
    blas = np.ascontiguousarray(blas, f32).reshape(-1, 8)
    tri_geom = np.ascontiguousarray(tri_geom, f32)
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 8)
    out = [np.zeros((len(rays), 6), u32) for _ in range(3)]
    L.lsm_reference(_ptr(blas), 0, _ptr(tri_geom), _ptr(rays), len(rays), _ptr(out[0]))
    nodes = L.nsm_sweep(_ptr(blas), len(blas), 0, cap, _ptr(tri_geom), _ptr(rays), len(rays), _ptr(out[1]))
    assert L.lsm_sweep(_ptr(blas), len(blas), 0, cap, _ptr(tri_geom), _ptr(rays), len(rays), _ptr(out[2])) >= 1
    return out[0], out[1], out[2], nodes


class Mesh:
    """Triangles (n, 3, 3) as the scene arrays surface_rays and the tree builder read, shifted so that box faces lie at 0:
    the lowest x and the highest y of the mesh and the lowest z of its middle triangle become 0 exactly (v - c in float32
    is 0 for v == c), and so does a face of every box that ends there, the root's among them."""
    def __init__(self, tri):
        tri = np.array(tri, f32)
        n = len(tri)
        shift = np.array([tri[:, :, 0].min(), tri[:, :, 1].max(), tri[n // 2, :, 2].min()], f32)
        self.tri = tri - shift
        self.vertices = np.concatenate([self.tri.reshape(-1, 3), np.ones((3 * n, 1), f32)], axis=1).reshape(-1)
        topo = np.zeros((n, 20), u32)
        topo[:, 0:3] = np.arange(3 * n).reshape(n, 3)
        self.mesh_topology = topo.reshape(-1)
        self.lo, self.hi = self.tri.min(axis=1), self.tri.max(axis=1)
        self.geom = np.zeros((n, 12), f32)
        self.geom[:, 0:3] = self.tri[:, 0]
        self.geom[:, 4:7] = self.tri[:, 1] - self.tri[:, 0]
        self.geom[:, 8:11] = self.tri[:, 2] - self.tri[:, 0]


def random_mesh(seed, n):
    rng = np.random.default_rng(seed)
    return Mesh(rng.uniform(-0.8, 0.8, (n, 1, 3)) + rng.normal(scale=0.18, size=(n, 3, 3)))


def hostile_rays(mesh, blas, n, seed):
    """n rays of surface_rays; three quarters of them get zero, negative-zero or denormal direction components (one, two or
    all three), and half of those, with a quarter of the rest, an origin whose coordinates on one to three axes lie on a box
    face of the tree, +-0 among them."""
    rng = np.random.default_rng(seed)
    rays = surface_rays(mesh, n, seed)
    k = np.arange(n)
    blas = np.asarray(blas, f32).reshape(-1, 8)
    for axis in range(3):
        bad_d = (k % 4 != 3) & (rng.random(n) < (0.6, 0.5, 0.4)[axis])
        rays[bad_d, 4 + axis] = HOSTILE[rng.integers(0, len(HOSTILE), bad_d.sum())]
        faces = np.concatenate([blas[:, axis], blas[:, 4 + axis], np.array([0.0, -0.0], f32)])
        on_face = (k % 2 == 0) & (rng.random(n) < 0.6)
        rays[on_face, axis] = faces[rng.integers(0, len(faces), on_face.sum())]
    return rays


def _compare(model, mesh, blas, rays, n_nodes):
    ref, node, leaf, nodes = walks(model, blas, mesh.geom, rays)
    assert nodes == n_nodes
    for col, what in enumerate(COLUMNS):
        bad = np.flatnonzero(ref[:, col] != node[:, col])
        assert bad.size == 0, "%s differs for %d of %d rays, first %s: reference %s, node sweep %s" % (
            what, bad.size, len(rays), rays[bad[0]].tolist(), ref[bad[0]].tolist(), node[bad[0]].tolist())
    return ref, leaf


def _worth_it(ref, rays):
    """the rays are worth the comparison: non-finite operands, hits and misses, occluded and open rays among them"""
    cold = ref[:, 5] == 1
    assert 0.5 < cold.mean() < 0.95
    # (few of them hit anything: a NaN slab term drops out of fmin / fmax, an infinite one usually ends the root's test)
    hit, occluded = ref[cold, 1] != 0xffffffff, ref[cold, 2] != 0
    assert min(hit.sum(), (~hit).sum(), occluded.sum(), (~occluded).sum()) >= 100
    assert ((rays[:, 0:3] == 0) & (rays[:, 4:7] == 0)).any()   # 0 * inf


@pytest.mark.parametrize("kind", ["one", "three", "triple", "full16"])
def test_the_node_sweep_equals_the_reference_walk_on_every_ray(model, kind):
    mesh = random_mesh(11, {"one": 5, "three": 9, "triple": 15, "full16": 30}[kind])
    blas = sweep_trees.build(mesh.lo, mesh.hi, 0, sweep_trees.shape(kind, len(mesh.tri)))
    assert (blas[:, 0:3] == 0).any() and (blas[:, 4:7] == 0).any()   # box faces at 0
    rays = hostile_rays(mesh, blas, 20_000, 5)
    ref, _ = _compare(model, mesh, blas, rays, sweep_trees.NODES[kind])
    _worth_it(ref, rays)


def test_the_node_sweep_equals_the_reference_walk_on_cornell(W, model):
    """tests/golden/cornell_blas.npz: the BLAS and the triangles of the headline scene as the host uploads them"""
    g = np.load(os.path.join(HERE, "golden", "cornell_blas.npz"))
    b = W.WorldBridge()
    b.loadScene("cornell")
    blas = np.asarray(g["blas"], f32).reshape(-1, 8)
    assert np.array_equal(blas.view(u32), np.asarray(b.blas, f32).view(u32).reshape(-1, 8))
    from test_leaf_sweep_model import triangle_records

    class M:
        geom = triangle_records(b)
        vertices, mesh_topology = b.vertices, b.mesh_topology
    assert (blas[:, 0:3] == 0).any()   # the box has walls at 0
    rays = hostile_rays(M, blas, 40_000, 9)
    ref, _ = _compare(model, M, blas, rays, 21)
    _worth_it(ref, rays)


@pytest.mark.parametrize("seed", range(12))
def test_the_node_sweep_equals_the_reference_walk_on_random_sweepable_trees(model, seed):
    rng = np.random.default_rng(300 + seed)
    mesh = random_mesh(400 + seed, int(rng.integers(1, 60)))
    s = sweep_trees.random_shape(rng, len(mesh.tri))
    blas = sweep_trees.build(mesh.lo, mesh.hi, 0, s)
    rays = hostile_rays(mesh, blas, 6_000, seed)
    _compare(model, mesh, blas, rays, len(blas))


def test_random_shapes_cover_wide_nodes_and_full_trees():
    shapes = []
    for seed in range(12):
        rng = np.random.default_rng(300 + seed)
        n = int(rng.integers(1, 60))
        shapes.append(sweep_trees.random_shape(rng, n))

    def widths(s):
        return [] if isinstance(s, int) else [len(s)] + [w for c in s for w in widths(c)]
    w = [x for s in shapes for x in widths(s)]
    assert 2 in w and 3 in w and 4 in w
    leaves = [len(sweep_trees.build(np.zeros((60, 3), f32), np.ones((60, 3), f32), 0, s)[:, 7].nonzero()[0]) for s in shapes]
    assert min(leaves) <= 3 and max(leaves) >= 12


def test_the_node_sweep_agrees_with_the_reference_where_the_leaf_sweep_does_not(model):
    """The hand-made ray of tests/test_leaf_sweep_model.py (test_a_ray_the_two_walks_disagree_on_without_the_guard): a root box
    [-1, 1]^3 over two leaves that meet at x = 0, a ray at x = 0.5 with d.x = 0.  The root's x slab is (-inf, NaN): a miss, and
    the reference never sees a leaf.  The leaf sweep, which does not test the root, hits the first leaf's triangle.  The node
    sweep tests the root, misses it and skips to the end of its subtree."""
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
    ref, node, leaf, nodes = walks(model, blas, tri, ray)
    assert nodes == 3
    assert ref[0, 5] == 1 and ref[0, 1] == 0xffffffff and ref[0, 2] == 0 and ref[0, 4] == 0
    assert np.array_equal(ref, node)
    assert leaf[0, 1] == 0 and leaf[0, 2] == 1 and leaf[0, 4] == 1   # what the leaf sweep would have answered
    ray[0, 4] = 1e-6   # a finite reciprocal: all three walks hit the triangle
    ref, node, leaf, _ = walks(model, blas, tri, ray)
    assert ref[0, 5] == 0 and ref[0, 1] == 0 and np.array_equal(ref, node) and np.array_equal(ref, leaf)
