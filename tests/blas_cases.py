"""Meshes that drive the GPU BLAS builder (csrc/bvh_build.hip.h) into the branches random vertices in a cube never reach,
and a reader of the tree shape that proves a mesh still does so: skewed splits that keep a node above kBig = 4 096
triangles alive far below the levels the host schedules the large-node kernels on, large nodes that cannot split, many
exactly equal centroids / costs / +-0 bounds, ranges around the kChunk = 2 048 chunking.  numpy only; every coordinate is
finite (the reference defines nothing for NaN / inf vertices).  tests/test_blas_cases.py holds every case to the shape it
was made for on the CPU builder, tests/test_gpu_blas_builder.py holds the GPU builder to the CPU builder on them.

Every generator returns (verts (n_verts, 3) float32, tris (n_tris, 3) uint32)."""
import collections

import numpy as np

f32 = np.float32
K_BIG = 4096       # bvh_build.hip.h kBig: nodes above this many triangles are worked on by the k_big_* kernels
K_CHUNK = 2048     # ... kChunk: in chunks of this many positions


def _ceil_log2(v):
    return max(int(v) - 1, 0).bit_length()


def guess_levels(n):
    """rt_api.hip blas_guess_levels: the tree levels launched for a mesh never built before"""
    return min(1024, _ceil_log2(max(n // 4, 1)) + 8)


def guess_big_levels(n):
    """rt_api.hip blas_guess_big_levels: ... of which the first so many run the large-node kernels"""
    return _ceil_log2((n + K_BIG - 1) // K_BIG) + 3 if n > K_BIG else 0


def tri_at(x, rng):
    """One "small" triangle per entry of x: y, z = 0.01 * rng.random(), s = 0.001 * x (all float32), vertices (x, y, z),
    (x + s, y + s, z), (x, y, z + s) — its size follows its place on x, so geometric spacing stays geometric."""
    x = np.asarray(x, f32).reshape(-1)
    n = len(x)
    y = f32(0.01) * rng.random(n, dtype=f32)
    z = f32(0.01) * rng.random(n, dtype=f32)
    s = f32(0.001) * x
    v = np.empty((n, 3, 3), f32)
    v[:, 0] = np.stack([x, y, z], 1)
    v[:, 1] = np.stack([x + s, y + s, z], 1)
    v[:, 2] = np.stack([x, y, z + s], 1)
    return v.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def _geometric(n, e_lo, e_hi, seed):
    rng = np.random.default_rng(seed)
    e = np.linspace(e_lo, e_hi, n)
    rng.shuffle(e)
    return tri_at(np.exp2(e).astype(f32), rng)


def skew(n, seed):
    """x = 2^e, e = linspace(-60, 20, n) shuffled: with 16 bins over the node's extent almost every centroid falls into
    bin 0, every level peels a few hundred triangles off, and a node above kBig survives many levels."""
    return _geometric(n, -60.0, 20.0, seed)


def overflow(n, seed):
    """skew with exponents -120 .. 120: the area of the root box is inf in f32, every SAH cost is inf, no candidate is
    valid and the mesh becomes ONE fallback leaf."""
    return _geometric(n, -120.0, 120.0, seed)


def scatter(n, seed):
    """centres uniform in the unit cube, the other two vertices within 0.003 of the centre: a balanced tree, leaves <= 4"""
    rng = np.random.default_rng(seed)
    c = rng.random((n, 3), dtype=f32)
    v = np.empty((n, 3, 3), f32)
    v[:, 0] = c
    v[:, 1] = c + (rng.random((n, 3), dtype=f32) * f32(2) - f32(1)) * f32(0.003)
    v[:, 2] = c + (rng.random((n, 3), dtype=f32) * f32(2) - f32(1)) * f32(0.003)
    return v.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def identical(n):
    """n copies of one triangle: nothing can split them"""
    verts = np.array([[0.25, 0.5, 0.125], [0.75, 1.0, 0.125], [0.25, 0.5, 0.625]], f32)
    return verts, np.tile(np.array([0, 1, 2], np.uint32), (n, 1))


def clump(n_same, n_spread, seed):
    """n_same coincident small triangles shuffled among n_spread small triangles spread along x (1 .. 2): the coincident
    ones end up, levels below the root, as one node that cannot split — a fallback leaf far above kBig when n_same is"""
    rng = np.random.default_rng(seed)
    sv, _ = tri_at(np.linspace(1.0, 2.0, n_spread).astype(f32), rng)
    one, _ = tri_at(np.array([1.4], f32), rng)
    v = np.concatenate([np.tile(one.reshape(1, 3, 3), (n_same, 1, 1)), sv.reshape(-1, 3, 3)])
    v = v[rng.permutation(len(v))]
    return v.reshape(-1, 3), np.arange(3 * len(v), dtype=np.uint32).reshape(-1, 3)


def lattice(n, seed):
    """Quantized coordinates: triangle origins on an 8 x 8 x 8 lattice of pitch 0.5 that straddles zero on x, box edges
    exactly 0.5 — dozens of coincident triangles per cell, exactly equal centroids and SAH costs — and a third of the zero
    coordinates written as -0.0 (min / max of +-0 is decided by the key order, not by the visiting order)."""
    rng = np.random.default_rng(seed)
    o = rng.integers(0, 8, (n, 3)).astype(f32) * f32(0.5)
    o[:, 0] -= f32(2.0)
    v = np.empty((n, 3, 3), f32)
    v[:, 0] = o
    v[:, 1] = o + np.array([0.5, 0.5, 0.0], f32)
    v[:, 2] = o + np.array([0.0, 0.0, 0.5], f32)
    v = v.reshape(-1, 3)
    zeros = np.flatnonzero(v.reshape(-1) == 0)
    v.reshape(-1)[zeros[::3]] = f32(-0.0)
    return v, np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


# scatter at these sizes: a root that is an exact multiple of kChunk, one whose last chunk holds 1 position, 2 047 positions
CHUNK_EDGES = (8191, 8192, 8193, 12289)


def chunk_edges(seed=5):
    return [scatter(n, seed) for n in CHUNK_EDGES]


# name -> (generator, arguments); a tree with fallback leaves above 7 triangles is listed in OVERFLOWED
CASES = collections.OrderedDict([
    ("skew_6000_s1", (skew, (6000, 1))), ("skew_6000_s2", (skew, (6000, 2))), ("skew_6000_s3", (skew, (6000, 3))),
    ("skew_16384_s1", (skew, (16384, 1))), ("skew_16384_s2", (skew, (16384, 2))),
    ("skew_40000_s1", (skew, (40000, 1))), ("skew_40000_s2", (skew, (40000, 2))),
    ("scatter_40000_s1", (scatter, (40000, 1))), ("scatter_40000_s2", (scatter, (40000, 2))),
    ("scatter_5000_s1", (scatter, (5000, 1))), ("scatter_8192_s1", (scatter, (8192, 1))), ("scatter_65_s1", (scatter, (65, 1))),
    ("overflow_4000_s1", (overflow, (4000, 1))), ("overflow_4200_s1", (overflow, (4200, 1))), ("overflow_8192_s1", (overflow, (8192, 1))),
    ("identical_5000", (identical, (5000,))), ("identical_6000", (identical, (6000,))),
    ("clump_4500_1500_s1", (clump, (4500, 1500, 1))),
    ("lattice_16384_s1", (lattice, (16384, 1))), ("lattice_10000_s2", (lattice, (10000, 2))),
] + [("chunk_edge_%d" % n, (scatter, (n, 5))) for n in CHUNK_EDGES])
OVERFLOWED = {"overflow_4000_s1", "overflow_4200_s1", "overflow_8192_s1", "identical_5000", "identical_6000", "clump_4500_1500_s1",
              "lattice_16384_s1", "lattice_10000_s2"}


def make(name):
    fn, args = CASES[name]
    return fn(*args)


def as_arrays(nodes):
    """(n, 8) float32 rows {min, skip} {max, data} from cpu_build_blas's list of dicts (or from such rows)"""
    if isinstance(nodes, np.ndarray):
        return np.ascontiguousarray(nodes, f32).reshape(-1, 8)
    a = np.zeros((len(nodes), 8), f32)
    u = a.view(np.uint32)
    for i, nd in enumerate(nodes):
        a[i, 0:3], a[i, 4:7] = nd["min"], nd["max"]
        u[i, 3], u[i, 7] = nd["skip"], nd["data"]
    return a


Shape = collections.namedtuple("Shape", "depth big_levels level_nodes largest_leaf level_max_tris")


def tree_shape(nodes, n_tris):
    """The shape of ONE BLAS from its pre-order node array (skip relative to the BLAS root, as cpu_build_blas returns it;
    leaf starts may carry a common topology offset): depth (levels, a single leaf is 1), big_levels (the deepest level
    holding a node above kBig triangles, + 1; 0 when there is none — what Ctl::big_levels / rt_build_blas_levels >> 16
    report), the node count of every level, the largest leaf, and the most triangles under one node per level.

    The triangle count under a node comes from the leaf tiling — the differences of the sorted leaf starts, the last
    leaf ending at n_tris — never from `data & 7`.  That is meaningful ONLY for trees without overflowed fallback leaves:
    there a word is `first << 3 | count` with an UNMASKED count (blas.rs:111-115; see UNREACHABLE in
    tests/test_bvh_independent.py), `data >> 3` is no longer the start, and the counts read here are garbage
    (leaf_counts below recovers them for such trees)."""
    leaf, skip, depth_of, tris_under, cnt = _per_node(nodes, n_tris)
    depth = int(depth_of.max()) + 1
    level_nodes = np.bincount(depth_of, minlength=depth).tolist()
    level_max = np.zeros(depth, np.int64)
    np.maximum.at(level_max, depth_of, tris_under)
    big = np.flatnonzero(level_max > K_BIG)
    return Shape(depth, int(big[-1]) + 1 if len(big) else 0, level_nodes, int(cnt.max()), level_max.tolist())


def _per_node(nodes, n_tris):
    a = as_arrays(nodes)
    u = a.view(np.uint32)
    skip, data = u[:, 3].astype(np.int64), u[:, 7].astype(np.int64)
    n = int(skip[0])
    skip, data = skip[:n], data[:n]
    leaf = data != 0
    start = data[leaf] >> 3
    o = np.argsort(start, kind="stable")
    ends = np.append(start[o][1:], start[o][0] + n_tris)
    cnt = np.zeros(int(leaf.sum()), np.int64)
    cnt[o] = ends - start[o]
    under = np.zeros(n + 1, np.int64)                     # prefix sums of the leaf counts in pre-order
    per_node = np.zeros(n, np.int64)
    per_node[leaf] = cnt
    under[1:] = np.cumsum(per_node)
    tris_under = under[skip] - under[np.arange(n)]
    depth_of = np.zeros(n, np.int64)
    for i in range(n):                                     # pre-order: a parent comes before its children
        if not leaf[i]:
            depth_of[i + 1] = depth_of[i] + 1
            depth_of[skip[i + 1]] = depth_of[i] + 1
    return leaf, skip, depth_of, tris_under, cnt


def device_levels(nodes, n_tris, big_launched):
    """The levels the GPU build of this tree puts nodes on (Ctl::cnt, the low half of rt_build_blas_levels) when the first
    `big_launched` levels run the large-node kernels: from level big_launched + 3 on the host launches k_level<64, false>
    (rt_api.hip blas_enqueue), where a node of at most kSubtree = 64 triangles is finished by its wave (k_subtree) and
    hands nothing to the next level.  That is why this is smaller than the depth of the tree, and it — not the depth — is
    what has to exceed the launched level count for a build to run again.  Same caveat as tree_shape."""
    leaf, skip, depth_of, tris_under, _ = _per_node(nodes, n_tris)
    in_wave = np.zeros(len(leaf), bool)                    # made inside a k_subtree call: on no level of the device
    for i in range(len(leaf)):
        if not leaf[i]:
            done = in_wave[i] or (tris_under[i] <= 64 and depth_of[i] >= big_launched + 3)
            in_wave[i + 1] = in_wave[skip[i + 1]] = done
    return int(depth_of[~in_wave].max()) + 1


def leaf_counts(nodes, n_tris, max_steps=2000000):
    """The true (first, count) of every leaf of a BLAS-local node array (first leaf at 0), in pre-order, also where counts
    overflowed the 3-bit field: leaves tile
    [0, n_tris) in pre-order, so with p = the triangles before a leaf its word is (p << 3) | count — the low three bits are
    count & 7, the rest is p | (count >> 3), which leaves count >> 3 open on the bits p has set.  Those are searched (the
    smallest count first) under the condition that every later word fits too and the last leaf ends at n_tris.  Raises
    ValueError when no assignment exists."""
    a = as_arrays(nodes)
    data = a.view(np.uint32)[:, 7].astype(np.int64)
    words = data[data != 0].tolist()

    def candidates(word, p):
        lo, hi = word & 7, word >> 3
        if p & ~hi:
            return
        need, free = hi & ~p, hi & p
        s = 0
        while True:                                        # the submasks of `free` in ascending order
            c = ((need | s) << 3) | lo
            if 1 <= c <= n_tris - p:
                yield c
            if s == free:
                return
            s = (s - free) & free

    out, iters, p, k, steps = [], [], 0, 0, 0
    while k < len(words):
        if len(iters) == k:
            iters.append(candidates(words[k], p))
        c = next(iters[k], None)
        steps += 1
        if steps > max_steps:
            raise ValueError("leaf words: search did not finish")
        if c is None:                                      # no count fits here: the previous leaf takes its next one
            iters.pop()
            if not out:
                raise ValueError("leaf words do not tile [0, %d)" % n_tris)
            p, _ = out.pop()
            k -= 1
            continue
        if k == len(words) - 1 and p + c != n_tris:
            continue
        out.append((p, c))
        p += c
        k += 1
    return out
