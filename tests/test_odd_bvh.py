"""Traversal on legal BVH arrays the builders never emit (tests/odd_bvh.py), on the host: the child-pair re-layout
(tests/pair_layout.py, restating csrc/k_pairs.hip.h) and the pair walk the kernels run (csrc/k_pairwalk.hip.h, compiled
by tests/model/pairwalk_model.cpp) against the oracle's literal loop — closest hit, occlusion bit and both counters of
every ray, at stacks of 64, 8, 2 and 1 entries.  A malformed layout can make a walk spin, so every walk runs in a child
process under a time limit and a stall fails the test.  No GPU (tests/test_gpu_odd_bvh.py runs the kernels)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import odd_bvh
import pair_layout

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
STACKS = (64, 8, 2, 1)
SEEDS = (1, 2, 3)
WALK_SECONDS = 240


def rays(n, seed, shadow):
    """rays_for (test_pairwalk_model.py) over a fixed box around the scene: a TLAS root box may be NaN or infinite here"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-3.0, 3.0, size=(n, 3)).astype(np.float32)
    o[: n // 4] = rng.uniform(-1.0, 1.0, size=(n // 4, 3)) + np.float32([0.0, 0.2, -4.2])   # some from the camera
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[: n // 4, 2] = np.abs(d[: n // 4, 2]) + 1.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[n // 4: n // 4 + n // 16, rng.integers(0, 3)] = 0.0   # some axis-parallel components (inf / NaN slabs)
    out = np.zeros((n, 8), np.float32)
    out[:, 0:3] = o
    out[:, 3] = 0.001
    out[:, 4:7] = d
    out[:, 7] = rng.uniform(0.5, 8.0, size=n).astype(np.float32) if shadow else 1e30
    return out


def compare_walks(b, n=1500, seed=7, stacks=STACKS):
    """the pair-walk model against the oracle's traceRays on `b`; returns a list of mismatch descriptions"""
    import ctypes
    import oracle_lib
    import webgpu_raytracer_amd as W
    from test_pairwalk_model import model_lib

    def p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    pairs, troot, inst_root = pair_layout.build(b.tlas, b.blas, b.instances)
    tri, inst_trav = pair_layout.traversal_records(b)
    L = model_lib()
    cpu = oracle_lib.OracleRenderer()
    cpu.buildPipeline(4, 1)
    W.upload_scene(cpu, b, 16, 16)
    bad = []
    for shadow in (False, True):
        rs = rays(n, seed + int(shadow), shadow)
        ref, ref_counts = cpu.traceRays(rs, any_hit=shadow)
        for k in stacks:
            out = np.zeros((n, 4), np.float32)
            counts = np.zeros((n, 2), np.uint64)
            stats = np.zeros(4, np.uint64)
            L.pwm_trace(p(pairs), p(troot), p(inst_trav), p(inst_root), p(tri), p(rs), n, int(shadow), k, 1, p(out), p(counts),
                        p(stats))
            if shadow:
                hit_bad = int((out[:, 3] != ref[:, 3]).sum())
            else:
                hit_bad = int((out[:, :3].view(np.uint32) != ref[:, :3].view(np.uint32)).any(axis=1).sum())
            cnt_bad = int((counts != ref_counts).any(axis=1).sum())
            if hit_bad or cnt_bad:
                bad.append("%s stack %d: %d hits, %d counter rows differ" % ("shadow" if shadow else "closest", k, hit_bad,
                                                                              cnt_bad))
    return bad


def _child(code):
    """run `code` in a fresh interpreter with the repository and tests/ importable; a stall is a failure"""
    prog = "import sys; sys.path[:0] = [%r, %r]\n" % (REPO, HERE) + code
    try:
        r = subprocess.run([sys.executable, "-s", "-c", prog], cwd=REPO, capture_output=True, text=True, timeout=WALK_SECONDS)
    except subprocess.TimeoutExpired:
        pytest.fail("the walk did not finish within %d s (a layout the walk cannot leave)" % WALK_SECONDS)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def built(W, oracle_lib):
    """the oracle, the scene library and the pair-walk model built once in this process; the children only load them"""
    from test_pairwalk_model import model_lib
    model_lib()
    return True


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", odd_bvh.CASES)
def test_pair_walk_equals_the_reference_loop_on_odd_arrays(built, case, seed):
    out = _child("import odd_bvh, test_odd_bvh as t\n"
                 "bad = t.compare_walks(odd_bvh.make(%d, %r))\n"
                 "print('MISMATCH' if bad else 'OK', bad)\n" % (seed, case))
    assert out.startswith("OK"), (case, seed, out)


@pytest.mark.parametrize("cases", [("empty_leaves", "loose_boxes", "single_child"),
                                   ("raw_fallback_words", "degenerate_boxes", "unreachable_gaps"),
                                   ("wide_leaves", "empty_leaves", "single_child", "unreachable_gaps"),
                                   ("deep_comb", "empty_leaves", "single_child"),
                                   ("tiny_trees", "degenerate_boxes"),
                                   ("empty_leaf_flush", "single_child", "loose_boxes")])
def test_pair_walk_on_combined_cases(built, cases):
    out = _child("import odd_bvh, test_odd_bvh as t\n"
                 "bad = t.compare_walks(odd_bvh.make(5, %r))\n"
                 "print('MISMATCH' if bad else 'OK', bad)\n" % (cases,))
    assert out.startswith("OK"), (cases, out)


def repro_single_child(b, rng, frac):
    """inner nodes X whose right child R is a leaf lose R: the skips in X's left subtree that named R name X's successor"""
    bl = np.array(b.blas, np.float32).reshape(-1, 8)
    u = bl.view(np.uint32)
    inst = np.asarray(b.instances, np.float32).reshape(-1, 36).view(np.uint32)
    done = 0
    for root in sorted(set(inst[:, 32].tolist())):
        size = int(u[root, 3])
        for x in range(root, root + size):
            if u[x, 7] != 0 or rng.random() > frac:
                continue
            l = x + 1
            r = root + int(u[l, 3])
            if r >= root + size or u[r, 7] == 0:
                continue
            sub = np.arange(l, r)
            m = root + u[sub, 3].astype(np.int64) == r
            u[sub[m], 3] = u[x, 3]
            done += 1
    b.blas = bl.reshape(-1)
    return done


def test_single_child_nodes_walk_as_the_reference(built):
    """The scenario that once gave wrong hits and counters at a 64-entry stack and a walk that never ended at a 1-entry
    stack: the pair layout turned a single-child node (its right child's slot names its own successor) into a bogus pair."""
    out = _child("import numpy as np, random_scene, odd_bvh, test_odd_bvh as t\n"
                 "b = random_scene.make(1, n_geoms=3, tris_per_geom=60, n_instances=5)\n"
                 "nd = t.repro_single_child(b, np.random.default_rng(1), 0.3)\n"
                 "assert nd == 11 and not odd_bvh.validate(b), nd\n"
                 "bad = t.compare_walks(b, n=2000, seed=1)\n"
                 "print('MISMATCH' if bad else 'OK', bad)\n")
    assert out.startswith("OK"), out


# ---------------------------------------------------------------------------------------- the generator itself
def _leaf_words(b):
    bu = np.asarray(b.blas, np.float32).reshape(-1, 8).view(np.uint32)
    return bu[:, 7][bu[:, 7] != 0]


def test_every_case_is_legal_and_has_its_feature():
    for seed in SEEDS:
        for case in odd_bvh.CASES:
            b = odd_bvh.make(seed, case)
            assert odd_bvh.validate(b) == []
            pair_layout.build(b.tlas, b.blas, b.instances)
            pair_layout.traversal_records(b)
        w = _leaf_words(odd_bvh.make(seed, "empty_leaves"))
        empty = ((w & 7) == 0) & ((w >> 3) > 0)
        assert 0.1 < empty.mean() < 0.6 and (empty[1:] & empty[:-1]).any()        # runs of adjacent empty leaves
        b = odd_bvh.make(seed, "wide_leaves")
        w = _leaf_words(b)
        assert {5, 6, 7} <= set((w & 7).tolist()) and {1, 2, 3, 4} & set((w & 7).tolist())
        assert ((w >> 3) + (w & 7) == len(b.mesh_topology) // 20).any()           # a leaf ends exactly at n_tris
        raw = odd_bvh.make(seed, "raw_fallback_words")
        assert not np.array_equal(_leaf_words(raw), _leaf_words(odd_bvh.make(seed, ())))
        b = odd_bvh.make(seed, "deep_comb")
        lv = odd_bvh.levels(b)
        assert len(lv) >= 3 and min(e - s for s, e in lv[1:3]) >= 2 * 300
        b = odd_bvh.make(seed, "unreachable_gaps")
        assert len(b.blas) > len(odd_bvh.make(seed, ()).blas)
        b = odd_bvh.make(seed, "single_child")
        assert b.single_child_nodes >= 3
        assert len(odd_bvh.make(seed, "tiny_trees").blas) // 8 <= 5 * 3
    assert len(odd_bvh.make(3, "tiny_trees").tlas) == 8                             # the TLAS is one leaf


def test_single_child_records_have_an_empty_slot():
    """pair_layout: a single-child node's record holds its one child on the left and the empty slot (word NONE, box
    +inf..+inf) on the right; no record names a node the reference walk cannot reach"""
    for seed in SEEDS:
        b = odd_bvh.make(seed, "single_child")
        pairs, troot, inst_root = pair_layout.build(b.tlas, b.blas, b.instances)
        pu = pairs.view(np.uint32)
        none = pu[:, 11] == pair_layout.NONE
        assert none.sum() >= b.single_child_nodes
        assert np.isposinf(pairs[none][:, [8, 9, 10, 12, 13, 14]]).all()
        assert (pu[none, 3] != pair_layout.NONE).all()


def test_empty_leaf_flush_scene_shape():
    """the race scene: empty and real leaves alternate in walk order and every empty leaf names a triangle that no real
    leaf holds (nearer than the grid)"""
    b = odd_bvh.make(1, "empty_leaf_flush")
    w = _leaf_words(b)
    kinds = (w & 7) == 0
    assert kinds[:-1:2].all() and not kinds[1::2].any()
    real = set((w[~kinds] >> 3).tolist())
    phantom = set((w[kinds] >> 3).tolist())
    assert max(phantom) not in real and len(w) > 300


def test_empty_leaf_flush_scene_visits_many_empty_leaves(built):
    """on the oracle: the camera rays of the race scene hit the grid and pass many empty leaves each (the phantom
    triangle those leaves name is never tested: a GPU image equal to the oracle's means no queued item leaked)"""
    import oracle_lib
    import webgpu_raytracer_amd as W
    import parity_util as pu
    b = odd_bvh.make(2, "empty_leaf_flush")
    cpu = oracle_lib.OracleRenderer()
    pu.drive(cpu, W, b, 64, 48, 6, 1, (1, 2, 3), present=False)
    c = cpu.getCounters()
    assert c["nodes_visited"] > 100 * c["primary_rays"]
    depth = cpu.readGBuffer()[2]
    assert (depth < 1.0).mean() > 0.4                           # a grid triangle fills half of every cell
