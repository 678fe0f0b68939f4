"""Legal BVH arrays that the builders never emit — test infrastructure.

The scene compiler (blas.rs / tlas.rs restated) and random_scene._build_bvh emit tidy trees only: tight boxes, a proper
binary pre-order, leaves of 1-7 triangles, no gaps between BLASes.  rt_upload_bvh takes any arrays, k_validate_scene
(csrc/k_validate.hip.h) accepts every array whose indices stay in range, and the reference's stackless walk renders all
of them.  Every case here writes such an array and returns a random_scene.Bridge, the duck-typed bridge parity_util.drive
and upload_scene take:

  empty_leaves        ~30 % of BLAS leaves rewritten to count 0 with first > 0, runs of adjacent ones included
  empty_leaf_flush    a scene built for the item-queue race of a count-0 leaf (see _empty_leaf_flush)
  wide_leaves         leaves of 5, 6 and 7 beside leaves of 1-4 in walk order; one leaf ends exactly at n_tris
  raw_fallback_words  leaf words with an unmasked count >= 8 (first << 3 | count, as blas.rs writes them): they decode to
                      another (first, count) and leave triangles unreachable; the decoded range stays in bounds
  loose_boxes         TLAS and BLAS boxes shrunk, grown or shifted: parents need not enclose children, leaves may cut
                      off parts of their triangles
  degenerate_boxes    zero extent on 1-3 axes, inverted boxes, +-inf bounds, NaN in one coordinate, TLAS and BLAS
  tiny_trees          single-node BLASes (the root is a leaf); a TLAS that is one leaf, or many instances of one BLAS
  deep_comb           left and right combs >= 300 deep: the pair walk goes stackless at every stack size
  unreachable_gaps    node ranges between BLASes that no instance names, filled with junk skip / data words
  single_child        inner nodes with one child (the right child made unreachable): at a BLAS root, deep inside, at
                      the last inner node of a BLAS, and in the TLAS

make(seed, cases) builds the base scene (random_scene.make unless a case makes its own) and applies the cases in
order; every result is checked against `validate`, a numpy restatement of k_validate_scene's rules, so a scene the
GPU refuses is a failure, never an expected outcome.
"""
import numpy as np

import random_scene

CASES = ("empty_leaves", "empty_leaf_flush", "wide_leaves", "raw_fallback_words", "loose_boxes", "degenerate_boxes",
         "tiny_trees", "deep_comb", "unreachable_gaps", "single_child")
BASE_CASES = ("empty_leaf_flush", "tiny_trees", "deep_comb")   # cases that build their own scene (first in a combination)


# ---------------------------------------------------------------------------------------------------------- arrays
def _nodes(a):
    n = np.array(a, np.float32).reshape(-1, 8)
    return n, n.view(np.uint32)


def _inst(b):
    i = np.array(b.instances, np.float32).reshape(-1, 36)
    return i, i.view(np.uint32)


def _roots(b):
    return sorted(set(_inst(b)[1][:, 32].tolist()))


def _geoms(b):
    """per geometry id: (first triangle, triangle count) from the topology rows (random_scene keeps them contiguous)"""
    topo = np.asarray(b.mesh_topology, np.uint32).reshape(-1, 20)
    out = {}
    for g in np.unique(topo[:, 3]):
        idx = np.flatnonzero(topo[:, 3] == g)
        out[int(g)] = (int(idx[0]), len(idx))
    return out


def _tri_boxes(b):
    pos = np.asarray(b.vertices, np.float32).reshape(-1, 4)[:, :3]
    topo = np.asarray(b.mesh_topology, np.uint32).reshape(-1, 20)
    v = pos[topo[:, 0:3].astype(np.int64)]
    return v.min(axis=1), v.max(axis=1)


def validate(b):
    """k_validate_scene restated: the list of problems (empty = the GPU accepts the scene)."""
    tl, tu = _nodes(b.tlas)
    bl, bu = _nodes(b.blas)
    n_tlas, n_nodes = len(tl), len(tl) + len(bl)
    n_verts = len(b.vertices) // 4
    topo = np.asarray(b.mesh_topology, np.uint32).reshape(-1, 20)
    n_tris = len(topo)
    inst = _inst(b)[1]
    n_inst = len(inst)
    bad = []
    if (topo[:, 0:3] >= n_verts).any():
        bad.append("triangles")
    for i in range(n_tlas):
        skip, data = int(tu[i, 3]), int(tu[i, 7])
        ok = i < skip <= n_tlas
        ok = ok and ((data >> 3) < n_inst if data else i + 1 < n_tlas)
        if not ok:
            bad.append("TLAS node %d" % i)
    roots = _roots(b)
    for g in range(len(bl)):
        below = [r for r in roots if r <= g]
        if not below:
            continue
        root = below[-1]
        if root >= len(bl):
            continue
        size, local = int(bu[root, 3]), g - root
        if local >= size:
            continue
        skip, data = int(bu[g, 3]), int(bu[g, 7])
        ok = local < skip <= size
        ok = ok and ((data >> 3) + (data & 7) <= n_tris if data else local + 1 < size)
        if not ok:
            bad.append("BLAS node %d" % g)
    for k in range(n_inst):
        off = int(inst[k, 32])
        ok = n_tlas + off < n_nodes
        if ok:
            size = int(bu[off, 3])
            ok = size >= 1 and n_tlas + off + size <= n_nodes
        if not ok:
            bad.append("instance %d" % k)
    lights = np.asarray(b.lights, np.uint32).reshape(-1, 2)
    if len(lights) and ((lights[:, 0] >= n_inst).any() or (lights[:, 1] >= n_tris).any()):
        bad.append("lights")
    return bad


def levels(b):
    """(start, end) absolute node ranges of the TLAS and of every BLAS an instance names (TLAS ++ BLAS numbering)"""
    tl, tu = _nodes(b.tlas)
    bl, bu = _nodes(b.blas)
    out = [(0, int(tu[0, 3]))]
    for r in _roots(b):
        out.append((len(tl) + r, len(tl) + r + int(bu[r, 3])))
    return out


# ------------------------------------------------------------------------------------------------ tree building
def _tree(lo_box, hi_box, first, count, split, leaf_word):
    """pre-order stackless nodes over triangles [first, first + count): split(lo, n, depth) -> None (leaf) or the size of
    the left part.  Returns rows [min, max, local skip, data] with tight boxes."""
    nodes = []

    def rec(lo, n, depth):
        idx = len(nodes)
        nodes.append(None)
        mn, mx = lo_box[lo:lo + n].min(axis=0), hi_box[lo:lo + n].max(axis=0)
        k = split(lo, n, depth)
        if k is None:
            nodes[idx] = [mn, mx, 0, leaf_word(lo, n)]
        else:
            nodes[idx] = [mn, mx, 0, 0]
            rec(lo, k, depth + 1)
            rec(lo + k, n - k, depth + 1)
        nodes[idx][2] = len(nodes)

    rec(first, count, 0)
    return random_scene._pack(nodes).reshape(-1, 8)


def _rebuild_blas(b, split_for):
    """every geometry's BLAS rebuilt over its own triangles in topology order; split_for(g) -> split function.
    Returns {geometry: BLAS offset}."""
    lo, hi = _tri_boxes(b)
    blocks, offs, off = [], {}, 0
    for g, (first, count) in sorted(_geoms(b).items()):
        blk = _tree(lo, hi, first, count, split_for(g), lambda f, n: (f << 3) | n)
        blocks.append(blk)
        offs[g] = off
        off += len(blk)
    b.blas = np.concatenate(blocks).reshape(-1)
    inst, iu = _inst(b)
    iu[:, 32] = [offs[int(g)] for g in iu[:, 34]]
    b.instances = inst.reshape(-1)
    return offs


def _use_geometry(b, k, g, offs):
    """instance k walks geometry g's BLAS from now on; every TLAS box becomes one generous box around the scene"""
    inst, iu = _inst(b)
    iu[k, 32], iu[k, 34] = offs[g], g
    b.instances = inst.reshape(-1)
    tl = _nodes(b.tlas)[0]
    tl[:, 0:3] = -8.0
    tl[:, 4:7] = 8.0
    b.tlas = tl.reshape(-1)


def _leaves(u):
    return np.flatnonzero(u[:, 7] != 0)


def _reachable(u, start, end, absolute):
    """nodes the reference's stackless walk can reach in the level [start, end) (every box hit)"""
    stack = [start]
    out = set()
    while stack:
        i = stack.pop()
        if i >= end or i in out:
            continue
        out.add(i)
        skip = int(u[i, 3]) + (0 if absolute else start)
        stack.append(skip)
        if u[i, 7] == 0:
            stack.append(i + 1)
    return out


# ------------------------------------------------------------------------------------------------------- cases
def empty_leaves(b, rng):
    bl, bu = _nodes(b.blas)
    run = False
    for i in _leaves(bu):
        run = rng.random() < (0.6 if run else 0.2)
        if run and (bu[i, 7] >> 3) > 0:
            bu[i, 7] &= ~np.uint32(7)
    b.blas = bl.reshape(-1)
    return b


def wide_leaves(b, rng):
    sizes = [5, 1, 6, 2, 7, 3, 4]
    geoms = _geoms(b)

    def split_for(g):
        first, count = geoms[g]
        cuts, at, k = [first], first, 0       # leaf runs of the sizes in turn, then a tree over the runs
        while at < first + count:
            at = min(at + sizes[k % len(sizes)], first + count)
            cuts.append(at)
            k += 1

        def split(lo, n, depth):
            inside = [c for c in cuts if lo < c < lo + n]
            return inside[len(inside) // 2] - lo if inside else None
        return split
    offs = _rebuild_blas(b, split_for)
    # the last geometry holds the last triangles: an instance walks its BLAS, so one leaf ends exactly at n_tris
    last = max(offs)
    if last not in _inst(b)[1][:, 34]:
        _use_geometry(b, 0, last, offs)
    return b


def raw_fallback_words(b, rng):
    bl, bu = _nodes(b.blas)
    n_tris = len(b.mesh_topology) // 20
    done = 0
    for i in _leaves(bu):
        if rng.random() > 0.35:
            continue
        first, count = int(bu[i, 7] >> 3), int(bu[i, 7] & 7)
        raw = int(rng.integers(8, 16))          # count field as blas.rs writes a fallback leaf: it spills into first
        word = (first << 3) + raw
        if (word >> 3) + (word & 7) <= n_tris and word & 7:
            bu[i, 7] = word
            done += 1
    b.blas = bl.reshape(-1)
    return b


def _perturb(a, rng, frac):
    n, u = _nodes(a)
    sel = rng.random(len(n)) < frac
    c = (n[:, 0:3] + n[:, 4:7]) / 2
    e = (n[:, 4:7] - n[:, 0:3]) / 2 * rng.uniform(0.2, 1.8, (len(n), 1)).astype(np.float32)
    c = c + (rng.normal(size=c.shape) * 0.15 * (np.abs(e) + 0.05)).astype(np.float32)
    n[sel, 0:3] = (c - e)[sel]
    n[sel, 4:7] = (c + e)[sel]
    return n.reshape(-1)


def loose_boxes(b, rng):
    b.blas = _perturb(b.blas, rng, 0.35)
    b.tlas = _perturb(b.tlas, rng, 0.35)
    return b


def _degenerate(a, rng, frac):
    n, u = _nodes(a)
    for i in np.flatnonzero(rng.random(len(n)) < frac):
        kind = int(rng.integers(0, 5))
        if kind == 0:                                   # zero extent on 1, 2 or 3 axes
            ax = rng.choice(3, size=int(rng.integers(1, 4)), replace=False)
            n[i, 4 + ax] = n[i, ax]
        elif kind == 1:                                 # inverted: min > max
            n[i, 0:3], n[i, 4:7] = n[i, 4:7].copy(), n[i, 0:3].copy()
        elif kind == 2:                                 # infinite on one axis
            ax = int(rng.integers(0, 3))
            n[i, ax], n[i, 4 + ax] = -np.inf, np.inf
        elif kind == 3:                                 # a bound at +-inf the wrong way round
            ax = int(rng.integers(0, 3))
            n[i, ax if rng.random() < 0.5 else 4 + ax] = np.inf if rng.random() < 0.5 else -np.inf
        else:                                           # NaN in one coordinate
            n[i, int(rng.choice([0, 1, 2, 4, 5, 6]))] = np.nan
    return n.reshape(-1)


def degenerate_boxes(b, rng):
    b.blas = _degenerate(b.blas, rng, 0.15)
    tl = _degenerate(b.tlas, rng, 0.25).reshape(-1, 8)
    tl[0] = _nodes(b.tlas)[0][0]                        # the TLAS root stays whole: the rays still get in
    b.tlas = tl.reshape(-1)
    return b


def _tiny_trees(seed, rng):
    """variant seed % 3: one instance (the TLAS is a single leaf) of a single-leaf BLAS; 24 instances of one single-leaf
    BLAS; five instances of three geometries, some single-leaf, some not"""
    variant = seed % 3
    b = random_scene.make(seed, n_geoms=(1, 1, 3)[variant], tris_per_geom=(5, 5, 9)[variant],
                          n_instances=(1, 24, 5)[variant])
    _rebuild_blas(b, lambda g: (lambda lo, n, depth: None if n <= 7 else n - 7))
    return b


def _comb(b, rng):
    def split_for(g):
        if g % 2 == 0:
            return lambda lo, n, depth: None if n == 1 else n - 1     # left comb: inner spine on the left, leaves right
        return lambda lo, n, depth: None if n == 1 else 1             # right comb: leaves left, inner spine right
    return _rebuild_blas(b, split_for)


def _deep_comb(seed, rng):
    b = random_scene.make(seed, n_geoms=2, tris_per_geom=640, n_instances=3)
    offs = _comb(b, rng)
    _use_geometry(b, 0, 0, offs)                        # both combs walked
    _use_geometry(b, 1, 1, offs)
    return b


def unreachable_gaps(b, rng):
    bl, bu = _nodes(b.blas)
    inst, iu = _inst(b)
    blocks, shift, out_len = [], {}, 0
    starts = sorted(set(_roots(b)) | {0})
    # split the array at every BLAS root and in front of each put a junk range no instance names
    cuts = starts + [len(bl)]
    for k in range(len(cuts) - 1):
        a, e = cuts[k], cuts[k + 1]
        gap = int(rng.integers(1, 9))
        junk = rng.normal(size=(gap, 8)).astype(np.float32)
        ju = junk.view(np.uint32)
        here = out_len + np.arange(gap)
        choice = rng.integers(0, 4, size=(gap, 2))
        for j in range(gap):
            for col, c in ((3, choice[j, 0]), (7, choice[j, 1])):
                ju[j, col] = (0, 0xFFFFFFFF, max(int(here[j]) - 3, 0), 1)[c]   # zero, all ones, backwards, tiny
        junk[rng.random(gap) < 0.3, 1] = np.nan
        blocks.append(junk)
        out_len += gap
        shift[a] = out_len
        blocks.append(bl[a:e])
        out_len += e - a
    tail = rng.normal(size=(3, 8)).astype(np.float32)
    tail.view(np.uint32)[:, 3] = 0
    tail.view(np.uint32)[:, 7] = 0
    blocks.append(tail)
    iu[:, 32] = [shift[int(o)] for o in iu[:, 32]]
    b.blas = np.concatenate(blocks).reshape(-1)
    b.instances = inst.reshape(-1)
    return b


def _make_single(u, x, start, absolute):
    """inner node x loses its right child: the skips in its left subtree that named the right child name x's successor"""
    if u[x, 7] != 0:
        return False
    base = 0 if absolute else start
    l = x + 1
    tx = base + int(u[x, 3])
    r = base + int(u[l, 3])
    if r >= tx:
        return False
    sub = np.arange(l, r)
    m = base + u[sub, 3].astype(np.int64) == r
    u[sub[m], 3] = u[x, 3]
    return True


def single_child(b, rng, frac=0.15):
    """returns the bridge; b.single_child_nodes counts the nodes made single-child that a walk can still reach"""
    done = 0
    bl, bu = _nodes(b.blas)
    tl, tu = _nodes(b.tlas)
    for root in _roots(b):
        size = int(bu[root, 3])
        end = root + size
        inner = [x for x in range(root, end) if bu[x, 7] == 0]
        if not inner:
            continue
        spine, x = [], root                              # the right spine: its last inner node is the last of the BLAS
        while bu[x, 7] == 0:
            spine.append(x)
            x = root + int(bu[x + 1, 3])
            if x >= end:
                break
        picks = {root, spine[-1]} | {x for x in inner if rng.random() < frac}
        for x in sorted(picks, reverse=True):            # deepest first: a pick inside an earlier one stays a tree
            reach = _reachable(bu, root, end, False)
            if x in reach and _make_single(bu, x, root, False):
                done += 1
    n_tlas = int(tu[0, 3])
    for x in sorted({0} | {x for x in range(n_tlas) if tu[x, 7] == 0 and rng.random() < 0.3}, reverse=True):
        if x in _reachable(tu, 0, n_tlas, True) and _make_single(tu, x, 0, True):
            done += 1
    b.blas = bl.reshape(-1)
    b.tlas = tl.reshape(-1)
    b.single_child_nodes = done
    return b


def _empty_leaf_flush(seed, rng):
    """A scene built to show the item-queue race of a count-0 leaf if the hardware ever lets the wrong store win.

    One instance, one BLAS in front of the camera.  Real triangles tile the plane z = 0 in a 16 x 12 grid, one per
    cell.  In walk order the BLAS alternates an EMPTY leaf (count 0, box around a few neighbouring cells) and the REAL
    leaf of one cell (count 1: the triangle its rays hit), so the lanes of a primary-ray wave, spread over several
    cells, wait at empty and at real leaves in the same flushes.  Every empty leaf's `first` names a huge triangle at
    z = -2, nearer than anything a camera ray really hits and reachable through no real leaf: a leaked item changes the
    hit, the G-buffer and the image.  A light triangle above the grid has a real leaf of its own."""
    gx, gy = 16, 12
    x0, x1, y0, y1 = -3.0, 3.0, -2.4, 2.8
    cw, ch = (x1 - x0) / gx, (y1 - y0) / gy
    tris = []
    for j in range(gy):
        for i in range(gx):
            ax, ay = x0 + i * cw, y0 + j * ch
            jit = rng.uniform(-0.05, 0.05, 2) * (cw, ch)
            tris.append([[ax, ay, 0.0], [ax + cw * 1.02 + jit[0], ay, 0.02 * (i % 3)], [ax, ay + ch * 1.02 + jit[1], 0.0]])
    big = len(tris)
    tris.append([[-40.0, -40.0, -2.0], [40.0, -40.0, -2.0], [0.0, 40.0, -2.0]])       # the phantom: never in a real leaf
    light = len(tris)
    tris.append([[-1.0, 3.5, -1.0], [1.0, 3.5, -1.0], [0.0, 3.5, 1.0]])
    tri = np.array(tris, np.float32)
    nt = len(tri)
    verts = np.concatenate([tri.reshape(-1, 3), np.ones((nt * 3, 1), np.float32)], axis=1)
    normals = np.zeros((nt * 3, 4), np.float32)
    normals[:, 2] = -1.0
    uvs = rng.uniform(0, 1, (nt * 3, 2)).astype(np.float32)
    topo = np.zeros((nt, 20), np.uint32)
    tf = topo.view(np.float32)
    topo[:, 0:3] = np.arange(nt * 3).reshape(nt, 3)
    tf[:, 4:7] = rng.uniform(0.3, 0.9, (nt, 3))
    tf[:, 7] = 0.0
    tf[:, 9] = 1.0
    tf[:, 10] = 1.5
    tf[:, 12:16] = -1.0
    tf[:, 19] = -1.0
    tf[light, 7] = 3.0
    tf[light, 4:7] = 6.0
    lo, hi = tri.min(axis=1) - 1e-4, tri.max(axis=1) + 1e-4
    # leaf sequence in walk order: (box lo, box hi, word)
    seq = []
    cells = list(range(gx * gy))
    for c in cells:
        nb = [k for k in (c - 1, c, c + 1, c + gx) if 0 <= k < gx * gy]
        first = big if rng.random() < 0.9 else int(rng.integers(1, big))
        seq.append((lo[nb].min(axis=0) - (0, 0, 3.0), hi[nb].max(axis=0), first << 3))
        seq.append((lo[c], hi[c], (c << 3) | 1))
    seq.append((lo[light], hi[light], (light << 3) | 1))
    nodes = []

    def rec(a, e):
        idx = len(nodes)
        nodes.append(None)
        if e - a == 1:
            nodes[idx] = [seq[a][0], seq[a][1], 0, seq[a][2]]
        else:
            m = (a + e) // 2
            nodes[idx] = [np.min([s[0] for s in seq[a:e]], axis=0), np.max([s[1] for s in seq[a:e]], axis=0), 0, 0]
            rec(a, m)
            rec(m, e)
        nodes[idx][2] = len(nodes)

    rec(0, len(seq))
    blas = random_scene._pack(nodes)
    inst = np.zeros(36, np.float32)
    inst[0:16] = np.eye(4, dtype=np.float32).reshape(-1)
    inst[16:32] = np.eye(4, dtype=np.float32).reshape(-1)
    inst.view(np.uint32)[32:36] = [0, 0, 0, 0]
    wlo, whi = np.array(nodes[0][0]) - 1e-3, np.array(nodes[0][1]) + 1e-3
    tlas = random_scene._pack([[wlo, whi, 1, (0 << 3) | 1]])
    cam = random_scene.make(seed, n_geoms=1, tris_per_geom=4, n_instances=1).cameraData
    return random_scene.Bridge(vertices=verts.reshape(-1), normals=normals.reshape(-1), uvs=uvs.reshape(-1),
                               mesh_topology=topo.reshape(-1), tlas=tlas, blas=blas, instances=inst,
                               lights=np.array([0, light], np.uint32), draw_commands=np.array([nt * 3, 1, 0, 0], np.uint32),
                               cameraData=cam, textures=None)


_MUTATORS = {"empty_leaves": empty_leaves, "wide_leaves": wide_leaves, "raw_fallback_words": raw_fallback_words,
             "loose_boxes": loose_boxes, "degenerate_boxes": degenerate_boxes, "unreachable_gaps": unreachable_gaps,
             "single_child": single_child}
_BASES = {"empty_leaf_flush": _empty_leaf_flush, "tiny_trees": _tiny_trees, "deep_comb": _deep_comb}


def make(seed, cases, **base_kw):
    """the scene of `cases` (a name or a sequence of names, applied in order) for `seed`; asserted legal"""
    cases = (cases,) if isinstance(cases, str) else tuple(cases)
    rng = np.random.default_rng(1000 + seed)
    bases = [c for c in cases if c in _BASES]
    assert len(bases) <= 1, cases
    if bases:
        b = _BASES[bases[0]](seed, rng)
    else:
        kw = dict(n_geoms=3, tris_per_geom=50, n_instances=5)
        kw.update(base_kw)
        b = random_scene.make(seed, **kw)
    for c in cases:
        if c in _MUTATORS:
            b = _MUTATORS[c](b, rng)
    bad = validate(b)
    assert not bad, (cases, seed, bad[:5])
    b.cases = cases
    return b
