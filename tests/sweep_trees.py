"""Sweepable BLASes of a given shape over a run of triangles — test infrastructure of the node sweep
(csrc/k_traverse.hip.h traverse_leaves, csrc/scene_facts.h walk_facts).

A shape is a nested list: an int is a leaf of that many triangles (1-7), a list an inner node of its children (two or more).
Triangles are taken in order, every box is the tight float32 box of what lies under it, so every child's stored box lies in
its parent's, bit for bit, and the array is in canonical pre-order: what walk_facts calls sweepable.

  one      the root is a leaf (1 node)
  three    a root over two leaves (3 nodes)
  triple   a root of three children, the middle one an inner node of three leaves (7 nodes)
  full16   a complete binary tree of 16 leaves (31 nodes: the most a sweep of 16 leaves has)
"""
import numpy as np

import odd_bvh
import random_scene


def _spread(n, k):
    """n triangles over k leaves, as evenly as they go"""
    assert k <= n <= 7 * k, (n, k)
    return [n // k + (1 if i < n % k else 0) for i in range(k)]


def _full(sizes):
    return sizes[0] if len(sizes) == 1 else [_full(sizes[:len(sizes) // 2]), _full(sizes[len(sizes) // 2:])]


def shape(kind, n):
    """the shape `kind` over n triangles"""
    if kind == "one":
        assert 1 <= n <= 7
        return n
    if kind == "three":
        return _spread(n, 2)
    if kind == "triple":
        s = _spread(n, 5)
        return [s[0], [s[1], s[2], s[3]], s[4]]
    if kind == "full16":
        return _full(_spread(n, 16))
    raise ValueError(kind)


# triangles per geometry that random_scene.make is asked for (it draws 0.5 .. 1.5 times as many)
TRIS = {"one": 4, "three": 6, "triple": 12, "full16": 22}
NODES = {"one": 1, "three": 3, "triple": 7, "full16": 31}


def random_shape(rng, n):
    """a random shape of at most 16 leaves over n triangles, inner nodes of two to four children"""
    leaves = int(rng.integers(max(1, -(-n // 7)), min(16, n) + 1))
    sizes = _spread(n, leaves)

    def rec(s):
        if len(s) == 1:
            return s[0]
        kids = int(rng.integers(2, min(4, len(s)) + 1))
        cuts = np.sort(rng.choice(np.arange(1, len(s)), kids - 1, replace=False)).tolist()
        return [rec(s[a:e]) for a, e in zip([0] + cuts, cuts + [len(s)])]
    return rec(sizes)


def count(s):
    return s if isinstance(s, int) else sum(count(c) for c in s)


def build(lo, hi, first, s):
    """rows [min, max, skip local to the root, data] of the shape `s` over the triangles from `first` on, whose boxes are
    lo[t], hi[t]; -> (nodes, 8) float32"""
    nodes = []

    def rec(s, at):
        idx = len(nodes)
        nodes.append(None)
        n = count(s)
        mn, mx = lo[at:at + n].min(axis=0), hi[at:at + n].max(axis=0)
        if isinstance(s, int):
            assert 1 <= s <= 7
            nodes[idx] = [mn, mx, 0, (at << 3) | s]
        else:
            assert len(s) >= 2
            nodes[idx] = [mn, mx, 0, 0]
            for c in s:
                rec(c, at)
                at += count(c)
        nodes[idx][2] = len(nodes)

    rec(s, first)
    return random_scene._pack(nodes).reshape(-1, 8)


def scene(kind, seed=0):
    """a one-instance, one-geometry random scene whose BLAS is the shape `kind` over its triangles"""
    b = random_scene.make(100 + seed, n_geoms=1, tris_per_geom=TRIS[kind], n_instances=1)
    lo, hi = odd_bvh._tri_boxes(b)
    blas = build(lo, hi, 0, shape(kind, len(lo)))
    assert len(blas) == NODES[kind]
    b.blas = blas.reshape(-1)
    bad = odd_bvh.validate(b)
    assert not bad, bad
    return b
