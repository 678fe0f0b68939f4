"""The meshes of tests/blas_cases.py on the CPU builder (ms_build_blas) — no GPU.  Two jobs:

 (a) the reference of tests/test_gpu_blas_builder.py is not taken as correct by definition on these inputs: every tree is
     checked with the builder-independent structure check of tests/test_bvh_independent.py (pre-order skips, leaves tile
     [0, n), boxes enclose what is below them, the right child ends where its parent ends), and for the trees with
     overflowed fallback leaves the true leaf ranges are recovered from the words (blas_cases.leaf_counts) and held to
     the same box rule;
 (b) every case keeps hitting the branch of csrc/bvh_build.hip.h it was made for: the shape of the CPU tree is asserted as
     inequalities against the host's launch formulas (blas_cases.guess_levels / guess_big_levels, rt_api.hip), so a later
     change of a generator or of a constant that takes a case off its branch fails here."""
import functools

import numpy as np
import pytest

import blas_cases as C
from test_bvh_independent import _nodes, check_blas_hierarchy, cpu_build_blas_raw


@functools.lru_cache(maxsize=None)
def _built(name):
    import webgpu_raytracer_amd as W
    W._build.build_scene()
    verts, tris = C.make(name)
    nodes, order = cpu_build_blas_raw(W, verts, tris)
    return verts, tris, nodes, order


def _shape(name):
    _, tris, nodes, _ = _built(name)
    return C.tree_shape(nodes, len(tris))


@pytest.mark.parametrize("name", list(C.CASES))
def test_cpu_tree_is_a_valid_hierarchy(W, name):
    verts, tris, nodes, order = _built(name)
    n = len(tris)
    assert sorted(order.tolist()) == list(range(n))                 # a permutation: every triangle in exactly one place
    assert np.isfinite(verts).all()
    tri_v = verts[tris[order].astype(np.int64)]                     # topology order = the builder's triangle order
    tmin, tmax = tri_v.min(axis=1), tri_v.max(axis=1)
    bmin, bmax, skip, data = _nodes(nodes)
    assert skip[0] == len(nodes)
    covered = check_blas_hierarchy(bmin, bmax, skip, data, 0, tmin, tmax, may_overflow=name in C.OVERFLOWED)
    if name not in C.OVERFLOWED:
        assert covered == (0, n)
        assert C.tree_shape(nodes, n).largest_leaf <= 4
        return
    assert covered is None, "listed as overflowed, but every leaf holds at most 7 triangles"
    # the true leaf ranges behind the overflowed words: they tile [0, n) and every leaf box encloses its triangles
    ranges = C.leaf_counts(nodes, n)
    leaves = np.flatnonzero(data != 0)
    assert len(ranges) == len(leaves) and ranges[0][0] == 0 and ranges[-1][0] + ranges[-1][1] == n
    for k, (first, count) in zip(leaves, ranges):
        assert int(data[k]) == (first << 3) | count
        assert (bmin[k] <= tmin[first:first + count].min(axis=0)).all() and (bmax[k] >= tmax[first:first + count].max(axis=0)).all()
    assert max(c for _, c in ranges) > 7


def test_tree_shape_and_leaf_counts_on_the_hand_derived_tree():
    """six_along_x of tests/golden/blas_kat.json: root over 6, leaves of 4 and 2 (derivation in test_bvh_independent.py)"""
    from test_bvh_independent import KAT
    s = C.tree_shape(KAT["six_along_x"]["nodes"], 6)
    assert s == C.Shape(2, 0, [1, 2], 4, [6, 4])
    assert C.leaf_counts(KAT["six_along_x"]["nodes"], 6) == [(0, 4), (4, 2)]
    # an overflowed word: 9 triangles after 3 -> (3 << 3) | 9 = 25, which decodes to first 3, count 1
    a = np.zeros((3, 8), np.float32)
    a.view(np.uint32)[:, 3] = (3, 2, 3)
    a.view(np.uint32)[:, 7] = (0, 3, (3 << 3) | 9)
    assert C.leaf_counts(a, 12) == [(0, 3), (3, 9)]
    assert (C.guess_levels(6000), C.guess_big_levels(6000), C.guess_big_levels(4096), C.guess_big_levels(40000)) == (19, 4, 0, 7)


@pytest.mark.parametrize("name", ["skew_6000_s1", "skew_6000_s2", "skew_6000_s3", "skew_16384_s1", "skew_16384_s2",
                                  "skew_40000_s1", "skew_40000_s2"])
def test_skewed_meshes_outlive_both_guesses(W, name):
    """A node above kBig on a level >= guess_big_levels + 3: levels guess .. guess + 2 run it in k_level<256, false>, the
    next in k_level<64, false>; and a tree deeper than guess_levels (what that does and does not mean for the number of
    launches: test_sequences_launch_too_few_levels_and_build_again)."""
    n = len(_built(name)[1])
    s = _shape(name)
    assert s.big_levels >= C.guess_big_levels(n) + 4, s
    assert s.depth > C.guess_levels(n), s


@pytest.mark.parametrize("seed", [1, 2])
def test_balanced_mesh_after_a_skewed_one_has_two_nodes_per_workgroup(W, seed):
    """With the large-node levels learnt from skew(40000), scatter(40000) runs k_level<256, true> (grid <= 1 024) on a
    level of more than 1 024 nodes none of which is large; and the level count learnt from scatter is too small for skew."""
    sc, sk = _shape("scatter_40000_s%d" % seed), _shape("skew_40000_s%d" % (3 - seed))
    assert any(sc.level_nodes[d] > 1024 and sc.level_max_tris[d] <= C.K_BIG for d in range(min(sk.big_levels, sc.depth))), (sc, sk)
    assert sc.depth + 2 < sk.depth
    assert sc.big_levels + 3 < sk.big_levels      # levels the skewed mesh's large nodes spend in the generic kernels next time


@pytest.mark.parametrize("name", ["overflow_4000_s1", "overflow_4200_s1", "overflow_8192_s1", "identical_5000"])
def test_unsplittable_meshes_are_one_leaf(W, name):
    verts, tris, nodes, order = _built(name)
    assert len(nodes) == 1
    assert int(nodes.view(np.uint32)[0, 7]) == len(tris)            # (0 << 3) | count, unmasked
    if name.startswith("overflow"):                                  # ... because the area of the root box is inf
        d = (nodes[0, 4:7] - nodes[0, 0:3]).astype(np.float32)
        with np.errstate(over="ignore"):
            assert np.isinf(np.float32(2) * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]))
        assert np.isfinite(nodes[0, :3]).all() and np.isfinite(nodes[0, 4:7]).all()


def test_clump_ends_in_a_large_fallback_leaf_below_the_root(W):
    verts, tris, nodes, order = _built("clump_4500_1500_s1")
    n = len(tris)
    ranges = C.leaf_counts(nodes, n)
    data = nodes.view(np.uint32)[:, 7]
    big = [(f, c) for f, c in ranges if c > C.K_BIG]
    assert len(big) == 1 and ((big[0][0] << 3) | big[0][1]) in data.tolist()
    assert len(nodes) > 1 and data[0] == 0                           # ... below an inner root
    # it sits on a level the first build does not run the large-node kernels on
    bmin, bmax, skip, _ = _nodes(nodes)
    k = int(np.flatnonzero(data == ((big[0][0] << 3) | big[0][1]))[0])
    depth = sum(1 for i in range(k) if data[i] == 0 and skip[i] > k)
    assert depth >= C.guess_big_levels(n)


def _device_levels(name, big_launched):
    _, tris, nodes, _ = _built(name)
    return C.device_levels(nodes, len(tris), big_launched)


def test_sequences_launch_too_few_levels_and_build_again(W):
    """What makes a build run again is not the depth of the tree but the levels the DEVICE puts nodes on
    (blas_cases.device_levels): nodes of at most 64 triangles are finished inside k_level<64, false>.  A single build of
    skew(n) therefore fits guess_levels(n) although its tree is deeper; the learnt-level sequences of
    tests/test_gpu_blas_builder.py are what reach the relaunch, once or twice (levels -> 2 levels + 8)."""
    for name in ("skew_6000_s1", "skew_16384_s1", "skew_40000_s1"):
        n = len(_built(name)[1])
        assert _shape(name).depth > C.guess_levels(n) >= _device_levels(name, C.guess_big_levels(n))
    # (a) balanced, then skewed, at 40 000: the skewed mesh is launched with the balanced one's levels + 2 and large-node levels
    sc, sk = _shape("scatter_40000_s1"), _shape("skew_40000_s1")
    learnt = _device_levels("scatter_40000_s1", C.guess_big_levels(40000)) + 2
    assert learnt < _device_levels("skew_40000_s1", sc.big_levels) <= 2 * learnt + 8
    # (c), (d) one leaf, then a balanced mesh: 1 + 2 = 3 levels, then 14
    for one, many in (("identical_5000", "scatter_5000_s1"), ("overflow_8192_s1", "scatter_8192_s1")):
        assert _shape(one).depth == 1
        assert 3 < _device_levels(many, 1) <= 14
    # (e) one leaf, then a skewed mesh: 3 levels, 14, 36
    assert _shape("identical_6000").depth == 1 and 14 < _device_levels("skew_6000_s1", 1) <= 36


@pytest.mark.parametrize("name", ["lattice_16384_s1", "lattice_10000_s2"])
def test_lattice_has_ties_signed_zeros_and_large_nodes(W, name):
    verts, tris, nodes, order = _built(name)
    cells = np.unique(verts[tris[:, 0].astype(np.int64)].view(np.uint32).reshape(-1, 3) & 0x7fffffff, axis=0)
    assert len(cells) <= 512 and len(tris) > C.K_BIG                 # dozens of coincident triangles per cell
    zero = verts == 0
    assert np.signbit(verts[zero]).any() and not np.signbit(verts[zero]).all()
    assert (verts[:, 0] < 0).any() and (verts[:, 0] > 0).any()
    assert max(c for _, c in C.leaf_counts(nodes, len(tris))) > 7
