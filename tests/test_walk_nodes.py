"""The node records of a sweepable BLAS (csrc/scene_facts.h walk_facts, its node output): what the node sweep of
csrc/k_traverse.hip.h traverse_leaves reads when a wave cannot take the leaf sweep.  Every node of the root's subtree in
array order; a leaf's record is its leaf record; an inner node's holds a zero word and the end of its subtree as a position in
the array; the padding record behind either array, which a sweep reads ahead, is no node.  Host compiler only, no GPU; the
stand-alone program tests/model/walk_nodes_check.cpp runs the same trees, and trees that are not sweepable, under
AddressSanitizer and UndefinedBehaviorSanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import model_build
import sweep_trees
from test_node_sweep_model import model, random_mesh  # noqa: F401  (the model library is the fixture of that file)

HERE = os.path.dirname(os.path.abspath(__file__))
PROGRAM = os.path.join(HERE, "model", "walk_nodes_check.cpp")
f32, u32 = np.float32, np.uint32


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def records(L, blas, root=0, cap=16):
    """(leaf records, node records, padding record) as (n, 8) words, or None when the tree is not sweepable"""
    L.nsm_records.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 4
    L.nsm_records.restype = ctypes.c_int
    blas = np.ascontiguousarray(blas, f32).reshape(-1, 8)
    leaves, nodes = np.zeros((64, 8), u32), np.zeros((127, 8), u32)
    n_nodes, pad = np.zeros(1, u32), np.zeros(8, u32)
    n = L.nsm_records(_ptr(blas), len(blas), root, cap, _ptr(leaves), _ptr(nodes), _ptr(n_nodes), _ptr(pad))
    return None if n < 0 else (leaves[:n], nodes[:int(n_nodes[0])], pad)


def trees():
    """name -> (nodes, 8) float32: the four named shapes, random ones, and Cornell's"""
    out = {}
    for kind, n in (("one", 5), ("three", 9), ("triple", 15), ("full16", 30)):
        m = random_mesh(11, n)
        out[kind] = sweep_trees.build(m.lo, m.hi, 0, sweep_trees.shape(kind, n))
    for seed in range(8):
        rng = np.random.default_rng(300 + seed)
        m = random_mesh(400 + seed, int(rng.integers(1, 60)))
        out["random%d" % seed] = sweep_trees.build(m.lo, m.hi, 0, sweep_trees.random_shape(rng, len(m.tri)))
    out["cornell"] = np.asarray(np.load(os.path.join(HERE, "golden", "cornell_blas.npz"))["blas"], f32).reshape(-1, 8)
    return out


@pytest.mark.parametrize("name", sorted(trees()))
def test_node_records_are_the_tree_in_walk_order(model, name):  # noqa: F811
    blas = trees()[name]
    w = blas.view(u32)
    leaves, nodes, _ = records(model, blas)
    assert len(nodes) == len(blas) and len(leaves) == np.count_nonzero(w[:, 7])
    assert len(nodes) <= 2 * len(leaves) - 1 <= 31
    # the boxes, in array order, bit for bit
    assert np.array_equal(nodes[:, 0:3], w[:, 0:3]) and np.array_equal(nodes[:, 4:7], w[:, 4:7])
    inner = w[:, 7] == 0
    # an inner record: a zero word, and the end of its subtree (the node's own skip) as a position behind its two children
    assert not nodes[inner, 7].any() and np.array_equal(nodes[inner, 3], w[inner, 3])
    pos = np.arange(len(blas))
    assert (nodes[inner, 3] >= pos[inner] + 3).all() and (nodes[inner, 3] <= len(blas)).all()
    # a leaf record: the leaf array's, in the same order
    assert np.array_equal(nodes[~inner], leaves)
    assert np.array_equal(leaves[:, 7], w[~inner, 7]) and np.array_equal(leaves[:, 3], 65536 // (w[~inner, 7] & 7) + 1)


def test_three_children_and_the_root_that_is_a_leaf(model):  # noqa: F811
    t = trees()
    _, nodes, _ = records(model, t["triple"])
    assert nodes[:, 7].astype(bool).tolist() == [False, True, False, True, True, True, True]
    assert nodes[0, 3] == 7 and nodes[2, 3] == 6
    leaves, nodes, _ = records(model, t["one"])
    assert len(nodes) == 1 and nodes[0, 7] != 0 and np.array_equal(nodes, leaves)


def test_the_padding_record_is_no_node(model):  # noqa: F811
    """An inverted box no ray's slab test passes with finite operands, under a zero word (no leaf) whose subtree would end at
    position 0 (no inner node: that is before the record itself); walk_facts refuses such a node wherever it stands."""
    _, _, pad = records(model, trees()["three"])
    box = pad.view(f32)
    assert (box[0:3] > box[4:7]).all() and np.isfinite(box[[0, 1, 2, 4, 5, 6]]).all()
    assert pad[7] == 0 and pad[3] == 0
    blas = trees()["three"].copy()
    for at in range(3):
        bad = blas.copy()
        bad.view(u32)[at] = pad
        assert records(model, bad) is None


def test_a_tree_over_the_cap_has_no_records(model):  # noqa: F811
    assert records(model, trees()["full16"], cap=15) is None
    assert records(model, trees()["full16"], cap=16) is not None


def _comb(n_leaves):
    """a right comb: not sweepable at 16 leaves, and more nodes than a node array holds"""
    lo = np.zeros((n_leaves, 3), f32)
    hi = np.ones((n_leaves, 3), f32)
    s = 1
    for _ in range(n_leaves - 1):
        s = [1, s]
    return sweep_trees.build(lo, hi, 0, s)


def _single_chain(n):
    """n inner nodes of one child each over one leaf: nodes without end and no leaf to count"""
    blas = np.zeros((n + 1, 8), f32)
    blas[:, 4:7] = 1.0
    w = blas.view(u32)
    w[:, 3] = n + 1
    w[n, 7] = 1
    return blas


def _behind_junk(blas):
    """the tree as the second BLAS of its array: its root is node 1, its skips stay local to the root"""
    junk = np.full((1, 8), np.nan, f32)
    return np.concatenate([junk, blas])


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    named = trees()
    cases = [(named[k], 0, 16, True) for k in sorted(named)]
    cases += [(named["full16"], 0, 15, False), (named["full16"], 0, 64, True), (_behind_junk(named["full16"]), 1, 16, True),
              (_comb(17), 0, 16, False), (_comb(64), 0, 64, True), (_comb(65), 0, 64, False), (_comb(300), 0, 4096, False),
              (_single_chain(200), 0, 64, False), (_single_chain(2047), 0, 64, False), (named["three"], 3, 16, False)]
    path = tmp_path / "trees.bin"
    with open(path, "wb") as f:
        for blas, root, cap, _ in cases:
            f.write(np.array([len(blas), root, cap], u32).tobytes())
            f.write(np.ascontiguousarray(blas, f32).tobytes())
    exe = str(tmp_path / "walk_nodes_check")
    flags = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-I", os.path.join(os.path.dirname(HERE), "include")]
    model_build.build(PROGRAM, exe, flags, program=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    lines = r.stdout.split("\n")
    assert lines[len(cases)] == "ok"
    for (blas, root, cap, sweepable), line in zip(cases, lines):
        if not sweepable:
            assert line == "0 0 0"
        else:
            sub = blas[root:root + int(blas.view(u32)[root, 3])]
            assert line == "1 %d %d" % (np.count_nonzero(sub.view(u32)[:, 7]), len(sub))
