"""What the host works out about the BLAS of a one-leaf scene (csrc/scene_facts.h walk_facts) and what the launch planner makes
of it (csrc/launch_plan.h persistent_shape).  The sweep forms of the wide path tracer test the BLAS leaves alone, which equals
the node walk only for a canonical pre-order tree of finite boxes that nest, stored word inside stored word; a tree wrongly
called sweepable is a wrong image.  Cornell's BLAS (tests/golden/cornell_blas.npz, written from WorldBridge) must give its
eleven leaves in walk order, bit for bit, and each clause of the condition is broken here on its own.
tests/model/walk_facts_check.cpp wraps the header; host compiler only, no GPU."""
import ctypes
import os

import numpy as np
import pytest

import model_build
import odd_bvh
import parity_util as pu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "webgpu-raytracer_amd", "csrc")
SRC = os.path.join(HERE, "model", "walk_facts_check.cpp")
LIB = os.path.join(HERE, "model", "_build", "libwalk_facts_check.so")
FIXTURE = os.path.join(HERE, "golden", "cornell_blas.npz")

UNKNOWN, NOT_SWEEPABLE, SWEEPABLE = 0, 1, 3   # known | sweepable << 1
CORNELL_LEAVES = [4, 6, 7, 8, 9, 12, 16, 17, 18, 19, 20]
CORNELL_COUNTS = [4, 4, 3, 4, 4, 6, 4, 2, 2, 1, 2]
f32, u32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def facts():
    flags = ["-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"]
    L = ctypes.CDLL(model_build.build(SRC, LIB, flags))
    L.wfc_max_nodes.restype = ctypes.c_uint64
    for name in ("wfc_max_records", "wfc_default_cap"):
        getattr(L, name).restype = ctypes.c_uint32
    L.wfc_divider.argtypes = [ctypes.c_uint32]
    L.wfc_divider.restype = ctypes.c_uint32
    L.wfc_eval.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    L.wfc_eval.restype = ctypes.c_int
    L.wfc_shape.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_int] * 3 + [ctypes.c_uint32, ctypes.c_int]
    L.wfc_shape.restype = ctypes.c_int
    return L


def evaluate(L, blas, root=0, cap=None):
    """(known | sweepable << 1, the leaf records as rows of 8 words)"""
    blas = np.ascontiguousarray(blas, dtype=f32).reshape(-1, 8)
    out = np.zeros((L.wfc_max_records(), 8), u32)
    got = L.wfc_eval(blas.ctypes.data_as(ctypes.c_void_p), len(blas), root, L.wfc_default_cap() if cap is None else cap,
                     out.ctypes.data_as(ctypes.c_void_p))
    return got & 3, out[:got >> 8]


def cornell():
    """(nodes as f32 rows, the same memory as u32 rows): a fresh copy of the fixture"""
    n = np.load(FIXTURE)["blas"].astype(f32).reshape(-1, 8).copy()
    return n, n.view(u32)


def parent_of(u, i):
    """the innermost inner node whose range [p + 1, skip[p]) holds node i (root 0)"""
    return max(p for p in range(i) if u[p, 7] == 0 and u[p, 3] > i)


def test_the_fixture_is_the_bridges_blas(W):
    b = W.WorldBridge()
    b.loadScene("cornell")
    z = np.load(FIXTURE)
    for name in ("blas", "tlas", "instances"):
        assert np.array_equal(np.asarray(getattr(b, name), f32).view(u32), z[name].view(u32)), name


def test_cornell_gives_its_eleven_leaves_in_order_bit_for_bit(facts):
    n, u = cornell()
    assert len(u) == 21 and np.flatnonzero(u[:, 7]).tolist() == CORNELL_LEAVES
    assert (u[CORNELL_LEAVES, 7] & 7).tolist() == CORNELL_COUNTS
    got, recs = evaluate(facts, n)
    assert got == SWEEPABLE and len(recs) == 11
    want = u[CORNELL_LEAVES].copy()
    want[:, 3] = [65536 // c + 1 for c in CORNELL_COUNTS]   # the skip word's place holds the count's divider
    assert np.array_equal(recs, want)


def test_the_divider_divides_every_item_number(facts):
    for count in range(1, 8):
        d = facts.wfc_divider(count)
        j = np.arange(64 * 7, dtype=np.uint64)
        assert d == 65536 // count + 1 and int(j[-1]) * d < 2 ** 32
        assert np.array_equal((j * d) >> 16, j // count), count


def test_a_child_box_one_ulp_outside_its_parent(facts):
    for leaf in (4, 12, 20):
        for word, towards in ((0, -np.inf), (1, -np.inf), (2, -np.inf), (4, np.inf), (5, np.inf), (6, np.inf)):
            n, u = cornell()
            p = parent_of(u, leaf)
            n[leaf, word] = np.nextafter(n[p, word], f32(towards))
            assert evaluate(facts, n)[0] == NOT_SWEEPABLE, (leaf, word)
            n[leaf, word] = n[p, word]   # on the parent's face: inside
            assert evaluate(facts, n)[0] == SWEEPABLE, (leaf, word)
    n, u = cornell()   # an inner node is a child too
    n[1, 4] = np.nextafter(n[0, 4], f32(np.inf))
    assert evaluate(facts, n)[0] == NOT_SWEEPABLE


def test_an_inverted_box(facts):
    n, u = cornell()
    assert n[6, 0] < n[6, 4]
    n[6, [0, 4]] = n[6, [4, 0]]
    assert evaluate(facts, n)[0] == NOT_SWEEPABLE
    n, u = cornell()   # lo == hi is a box
    n[19, 4] = n[19, 0]
    assert evaluate(facts, n)[0] == SWEEPABLE


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_a_word_that_is_not_finite(facts, value):
    for node, word in ((0, 0), (0, 6), (5, 1), (12, 2), (20, 4)):
        n, u = cornell()
        n[node, word] = value
        assert evaluate(facts, n)[0] == NOT_SWEEPABLE, (node, word)


def test_a_leaf_of_no_triangles(facts):
    n, u = cornell()
    u[9, 7] &= ~u32(7)   # first > 0, count 0: a legal leaf, which the node walk passes
    assert u[9, 7] != 0
    assert evaluate(facts, n)[0] == NOT_SWEEPABLE


def test_an_inner_node_with_one_child(facts):
    for x in (0, 1, 15):
        n, u = cornell()
        assert odd_bvh._make_single(u, x, 0, False)
        assert evaluate(facts, n)[0] == NOT_SWEEPABLE, x
    # every node reachable and every skip the end of a subtree, but node 0 has the one child 1: 0 -> 1 -> {2, 3}
    n, u = cornell()
    t = np.repeat(n[4:5], 4, axis=0)
    tu = t.view(u32)
    tu[:, 3] = [4, 4, 3, 4]
    tu[:2, 7] = 0
    assert evaluate(facts, t)[0] == NOT_SWEEPABLE
    assert evaluate(facts, t[1:].copy())[0] == NOT_SWEEPABLE   # (skips relative to another root)
    tu[1:, 3] -= 1
    assert evaluate(facts, t[1:].copy())[0] == SWEEPABLE     # the same three nodes as a tree of their own


def test_a_skip_that_goes_back(facts):
    for node, skip in ((6, 5), (6, 6), (10, 2), (20, 0)):
        n, u = cornell()
        u[node, 3] = skip
        assert evaluate(facts, n)[0] == NOT_SWEEPABLE, (node, skip)
    n, u = cornell()   # forward, but past the parent's end, or over nodes nothing else reaches
    u[4, 3] = 8
    assert evaluate(facts, n)[0] == NOT_SWEEPABLE
    n, u = cornell()
    u[0, 3] = 22    # the root's range ends behind the array
    assert evaluate(facts, n)[0] == NOT_SWEEPABLE


def test_one_leaf_over_the_cap(facts):
    n, u = cornell()
    assert facts.wfc_default_cap() == 16
    assert evaluate(facts, n, cap=11)[0] == SWEEPABLE
    assert evaluate(facts, n, cap=10)[0] == NOT_SWEEPABLE
    assert evaluate(facts, n, cap=1000)[0] == SWEEPABLE   # no cap above what the record buffer holds is honoured ...
    assert facts.wfc_max_records() == 64


def test_a_subtree_as_the_root(facts):
    n, u = cornell()
    # nodes 1 .. 9 are a tree of their own when skips are taken from node 1: the skips of Cornell's BLAS are relative to
    # node 0, so from root 1 every skip names one node further and the tree is not canonical
    assert evaluate(facts, n, root=1)[0] == NOT_SWEEPABLE
    sub = n[1:10].copy()
    sub.view(u32)[:, 3] -= 1
    got, recs = evaluate(facts, sub)
    assert got == SWEEPABLE and np.array_equal(recs[:, 7], u[[4, 6, 7, 8, 9], 7])
    got, recs = evaluate(facts, n[4:5].copy(), root=0)   # a root that is a leaf, with skip 5: not the end of a one-node tree
    assert got == NOT_SWEEPABLE
    one = n[4:5].copy()
    one.view(u32)[0, 3] = 1
    assert evaluate(facts, one)[0] == SWEEPABLE


def test_the_diamond_is_sweepable(W, facts):
    """The viewer scene's second instance is the 8-triangle octahedron: a BLAS of its own behind the floor's, named by its root."""
    b = pu.bridge_for(W, "viewer_diamond")
    n = np.asarray(b.blas, f32).reshape(-1, 8)
    u = n.view(u32)
    roots = np.asarray(b.instances, f32).view(u32).reshape(-1, 36)[:, 32].tolist()
    root = max(roots)
    assert root > 0 and root + u[root, 3] == len(u)
    leaves = root + np.flatnonzero(u[root:, 7])
    assert int((u[leaves, 7] & 7).sum()) == 8
    got, recs = evaluate(facts, n, root=root)
    assert got == SWEEPABLE and np.array_equal(recs[:, 7], u[leaves, 7])
    assert np.array_equal(recs[:, [0, 1, 2, 4, 5, 6]], u[leaves][:, [0, 1, 2, 4, 5, 6]])
    got, recs = evaluate(facts, n, root=min(roots))   # the floor's and the light's BLAS
    assert got == SWEEPABLE and int((recs[:, 7] & 7).sum()) == 12


def test_an_upload_the_host_does_not_scan(facts):
    n, u = cornell()
    assert facts.wfc_max_nodes() == 64 * 1024 // 32
    assert evaluate(facts, n, root=21)[0] == UNKNOWN
    assert facts.wfc_eval(None, 21, 0, 16, None) == UNKNOWN
    big = np.zeros((facts.wfc_max_nodes() + 1, 8), f32)
    assert evaluate(facts, big)[0] == UNKNOWN


# (nodes, triangles, vertices) of Cornell and of two random one-leaf scenes, one on each side of the wide form's LDS line
@pytest.mark.parametrize("size", [(22, 36, 72), (26, 30, 90), (28, 45, 135)])
def test_the_planner_takes_a_sweep_form_for_wide_launches_of_sweepable_scenes_only(facts, size):
    for frames in (1, 2, 32):
        for detailed in (0, 1):
            for plain in (0, 1):
                for walk in (UNKNOWN, NOT_SWEEPABLE, SWEEPABLE, 2):   # 2: sweepable without known
                    for leaves in (0, 1, 11, 16, 17):
                        for knob in (0, 1):
                            got = facts.wfc_shape(*size, frames, detailed, plain, walk, leaves, knob)
                            assert got >= 0, "the walk facts changed the launch shape"
                            wide = bool(got & 1)
                            assert wide == (frames > 1 and not detailed and size[1] < 45)
                            assert bool(got & 2) == (wide and plain == 1)
                            assert bool(got & 4) == (wide and walk == SWEEPABLE and 1 <= leaves <= 16 and knob == 1)


def test_walk_facts_are_host_only():
    text = open(os.path.join(CSRC, "scene_facts.h")).read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
