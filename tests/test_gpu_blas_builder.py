"""The GPU BLAS builder (csrc/bvh_build.hip.h behind rt_build_blas and rt_world_update) against the scene compiler's CPU
builder on the meshes of tests/blas_cases.py — node array and triangle order bit for bit, no tolerance anywhere.  What
each mesh is for, and the proof on the CPU tree that it still gets there, is in tests/test_blas_cases.py:

 1. nodes above kBig in the GENERIC level kernels (k_level<256, false>, k_level<64, false>): skew_* built once (the guessed
    large-node levels end 4+ levels above the last large node), skew after scatter in the sequences, clump's fallback leaf;
 2. more than one node per workgroup in k_level<256, true>: scatter(40000) after skew(40000) (2 048 small nodes on level 11,
    grid 1 024, the large-node levels learnt from the skewed mesh);
 3. learnt level counts that are wrong for the next mesh: the sequences, the world path, the skinned mesh that changes shape;
 4. large nodes that cannot split: overflow_* (every SAH cost inf), identical_*, clump;
 5. ties: lattice_* (coincident triangles, equal centroids and costs, +-0 bounds inside large nodes).
The hand-derived arrays of tests/golden/blas_kat.json are applied to the GPU builder as they are to the CPU builder."""
import functools

import numpy as np
import pytest

import blas_cases as C
import gltf_util as G
from test_bvh_independent import KAT, cpu_build_blas_raw, mesh_from_boxes
from test_gpu_world_update import _same

f32 = np.float32


@functools.lru_cache(maxsize=None)
def _ref(name):
    """mesh and CPU answer of one case, computed once for every test that uses it"""
    import webgpu_raytracer_amd as W
    W._build.build_scene()
    verts, tris = C.make(name)
    nodes, order = cpu_build_blas_raw(W, verts, tris)
    for a in (verts, tris, nodes, order):
        a.setflags(write=False)
    return verts, tris, nodes, order


def _gpu_build(r, verts, tris):
    verts = np.asarray(verts, f32)
    v4 = np.concatenate([verts, np.ones((len(verts), 1), f32)], 1)
    return r.buildBlas(v4, np.asarray(tris, np.uint32).reshape(-1))


def _equal(tag, got, want):
    """bitwise, with the first differing word on a mismatch"""
    for what, g, w in (("nodes", got[0], want[0]), ("order", got[1], want[1])):
        g = np.ascontiguousarray(g).view(np.uint32).reshape(-1)
        w = np.ascontiguousarray(w).view(np.uint32).reshape(-1)
        assert g.shape == w.shape, (tag, what, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError("%s %s: %d of %d words differ, first at %d (want %08x got %08x)"
                                 % (tag, what, len(bad), len(w), bad[0], w[bad[0]], g[bad[0]]))


def _levels(r):
    v = r.L.rt_build_blas_levels(r.ctx)
    return v & 0xffff, v >> 16          # levels the device put nodes on, levels that held a node above 4 096 triangles


def _check_levels(r, name, big_launched):
    if not name.startswith(("skew", "scatter", "chunk_edge")):
        return                            # tree_shape reads nothing meaningful from overflowed leaf words
    _, tris, nodes, _ = _ref(name)
    levels, big = _levels(r)
    print("%s: device levels %d, large-node levels %d (launched with %d)" % (name, levels, big, big_launched))
    assert big == C.tree_shape(nodes, len(tris)).big_levels, name
    assert levels == C.device_levels(nodes, len(tris), big_launched), name


def _as_dicts(nodes):
    u = nodes.view(np.uint32)
    return [{"min": nodes[i, 0:3].tolist(), "skip": int(u[i, 3]), "max": nodes[i, 4:7].tolist(), "data": int(u[i, 7])}
            for i in range(len(nodes))]


@pytest.mark.gpu
def test_gpu_builder_gives_the_hand_derived_arrays(W):
    """The arrays worked out by hand from blas.rs (derivations in tests/test_bvh_independent.py), NOT the CPU builder's."""
    r = W.WebGPURenderer(0)
    for case, boxes, want_order in (("six_along_x", [(x, 0, 0, 1, 1, 1) for x in (8, 0, 15, 1, 10, 13)], [2, 0, 4, 5, 3, 1]),
                                    ("axis_rule", [(0, y, z, 2, 1, 1) for (y, z) in ((0, 0), (0, 7), (2, 3), (2, 5), (1, 1))], [2, 3, 4, 0, 1])):
        nodes, order = _gpu_build(r, *mesh_from_boxes(boxes))
        assert order.tolist() == KAT[case]["order"] == want_order
        assert _as_dicts(nodes) == KAT[case]["nodes"]
    nodes, order = _gpu_build(r, *mesh_from_boxes([(0, 0, 0, 1, 1, 1), (4, 0, 0, 1, 1, 1), (9, 0, 0, 1, 1, 1)]))
    assert order.tolist() == [0, 1, 2]
    assert _as_dicts(nodes) == [{"min": [0.0, 0.0, 0.0], "skip": 1, "max": [10.0, 1.0, 1.0], "data": 3}]
    flat, order = _gpu_build(r, [(0, 0, 0), (1, 0, 0), (0, 0, 1)], [(0, 1, 2)])      # size.y = 0 < 1e-5 -> +-0.5e-5
    half = float(f32(1e-5) * f32(0.5))
    assert order.tolist() == [0]
    assert _as_dicts(flat) == [{"min": [0.0, -half, 0.0], "skip": 1, "max": [1.0, half, 1.0], "data": 1}]
    r.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(C.CASES))
def test_single_build_on_a_fresh_renderer(W, name):
    """Guessed level counts (blas_guess_levels / blas_guess_big_levels).  For the skewed and the balanced meshes the counters
    the build reports are those of the CPU tree: the large-node levels (a skewed mesh has them 4+ levels past the guess,
    i.e. its large nodes went through both generic level kernels) and the levels the device put nodes on."""
    verts, tris, want_nodes, want_order = _ref(name)
    r = W.WebGPURenderer(0)
    got = _gpu_build(r, verts, tris)
    _equal(name, got, (want_nodes, want_order))
    _check_levels(r, name, C.guess_big_levels(len(tris)))
    r.destroy()


SEQUENCES = {
    "a_balanced_skewed_40000": ["scatter_40000_s1", "skew_40000_s1", "scatter_40000_s2", "skew_40000_s2"],
    "b_skewed_lattice_16384": ["skew_16384_s1", "lattice_16384_s1", "skew_16384_s1"],
    "c_one_leaf_balanced_5000": ["identical_5000", "scatter_5000_s1", "identical_5000"],
    "d_overflow_balanced_8192": ["overflow_8192_s1", "scatter_8192_s1"],
    "e_one_leaf_skewed_6000": ["identical_6000", "skew_6000_s1"],
}


@pytest.mark.gpu
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
def test_sequences_at_one_size_on_one_renderer(W, seq):
    """Learnt level counts: rt_build_blas launches the previous build's levels + 2 and its large-node levels whenever n_tris
    is unchanged — too few of both after a balanced or an unsplittable mesh (the build runs again; large nodes on generic
    levels), too many after a skewed one (k_big_* on levels without a large node, k_level<256, true> with two nodes per
    workgroup, many empty levels).  EVERY build equals its CPU answer."""
    r = W.WebGPURenderer(0)
    big_launched = None
    for k, name in enumerate(SEQUENCES[seq]):
        verts, tris, want_nodes, want_order = _ref(name)
        if big_launched is None:
            big_launched = C.guess_big_levels(len(tris))
        got = _gpu_build(r, verts, tris)
        _equal("%s[%d] %s" % (seq, k, name), got, (want_nodes, want_order))
        _check_levels(r, name, big_launched)
        big_launched = _levels(r)[1]
    r.destroy()


def _static_glb(meshes):
    """one mesh / node per (verts, tris), in this order"""
    b = G.GltfBuilder()
    for verts, tris in meshes:
        acc = {"POSITION": b.accessor(np.asarray(verts, f32), G.F32, "VEC3", minmax=True)}
        b.doc["meshes"].append({"primitives": [{"attributes": acc, "indices": b.accessor(np.asarray(tris, np.uint32).reshape(-1), G.U32, "SCALAR")}]})
        b.doc["nodes"].append({"mesh": len(b.doc["meshes"]) - 1})
    b.doc["scenes"][0]["nodes"] = list(range(len(meshes)))
    return b.glb()


@pytest.mark.gpu
def test_world_update_with_awkward_geometries(W):
    """blas_enqueue inside rt_world_update: node_base chaining and non-zero topo_start (a large geometry after small ones,
    small ones after a large one, overflowed leaf words that get the topology offset added), the per-geometry level
    counts and their relaunch loop; then, with the static cache off, rebuilds with the learnt counts."""
    one = (np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1]], f32), np.array([[0, 1, 2]], np.uint32))
    glb = _static_glb([_ref("skew_16384_s1")[:2], _ref("lattice_10000_s2")[:2], _ref("identical_5000")[:2],
                       _ref("clump_4500_1500_s1")[:2], one, _ref("scatter_65_s1")[:2]])
    r = W.WebGPURenderer(0)
    cpu_b, dev_b = W.WorldBridge(), W.WorldBridge()
    dev_b.setDeviceUpdater(r)
    cpu_b.loadScene("viewer", glbData=glb)
    dev_b.loadScene("viewer", glbData=glb)
    for t in (0.0, 0.1, 0.2):
        if t == 0.1:
            r.setWorldStaticCache(False)
        cpu_b.update(t)
        dev_b.update(t)
        assert dev_b.deviceResident, dev_b.deviceWarning
        _same(r, cpu_b, "awkward world t=%g" % t)
    inst = np.asarray(cpu_b.instances).reshape(-1, 36)
    assert len(inst) == 1 + 6                                   # the room + one instance per mesh
    r.destroy()


SKIN_E, SKIN_S = 80.0, 90.0       # x grows by 1 + 2^e, e = 0 .. SKIN_E, at joint scale 2^SKIN_S


def shape_changing_skinned_glb(n_tris=16384, seed=7):
    """Two joints, per-triangle weights (w0, w1) = (1 - w1, 2^(e - SKIN_S)), e = linspace(0, SKIN_E) shuffled — the exponent is in
    the weight.  Joint 0 stays the identity, joint 1 is scaled on x by a factor animated 1 -> 2^SKIN_S -> 1 over t = 0, 1, 2
    (weights are used as given, without renormalisation: k_skin, the scene compiler's skinning loop).  At scale 1 the blend is
    (w0 + w1) * identity: the mesh is scatter(n_tris).  At scale 2^SKIN_S a vertex's x becomes x * (w0 + w1 * 2^SKIN_S) ~
    x * (1 + 2^e): geometrically spaced along x like blas_cases.skew."""
    rng = np.random.default_rng(seed)
    verts, tris = C.scatter(n_tris, seed)
    verts = verts.copy()
    verts[:, 0] = f32(0.25) + f32(0.75) * verts[:, 0]           # away from x = 0: a triangle that straddles it would become 2^e wide
    e = np.linspace(0.0, SKIN_E, n_tris)
    rng.shuffle(e)
    w1 = np.repeat(np.exp2(e - SKIN_S).astype(f32), 3)          # scatter: three vertices of their own per triangle
    weights = np.stack([f32(1) - w1, w1, 0 * w1, 0 * w1], 1).astype(f32)
    joints = np.tile(np.array([0, 1, 0, 0], np.uint16), (len(verts), 1))
    nrm = np.tile(np.array([0, 0, 1], f32), (len(verts), 1))
    b = G.GltfBuilder()
    acc = dict(POSITION=b.accessor(verts, G.F32, "VEC3", minmax=True), NORMAL=b.accessor(nrm, G.F32, "VEC3"),
               JOINTS_0=b.accessor(joints, G.U16, "VEC4"), WEIGHTS_0=b.accessor(weights, G.F32, "VEC4"))
    b.doc["meshes"] = [{"primitives": [{"attributes": acc, "indices": b.accessor(tris.reshape(-1), G.U32, "SCALAR")}]}]
    b.doc["nodes"] = [{"mesh": 0, "skin": 0}, {"children": [2]}, {"translation": [0, 0, 0]}]
    eye = np.stack([np.eye(4, dtype=f32), np.eye(4, dtype=f32)])
    b.doc["skins"] = [{"joints": [1, 2], "inverseBindMatrices": b.accessor(eye, G.F32, "MAT4")}]
    big = float(np.exp2(f32(SKIN_S)))
    t_in = b.accessor(np.array([0, 1, 2], f32), G.F32, "SCALAR", minmax=True)
    sc = b.accessor(np.array([[1, 1, 1], [big, 1, 1], [1, 1, 1]], f32), G.F32, "VEC3")
    b.doc["animations"] = [{"samplers": [{"input": t_in, "output": sc}], "channels": [{"sampler": 0, "target": {"node": 2, "path": "scale"}}]}]
    return b.glb()


def _geometry_tree(bridge, geometry, n_tris):
    """shape of the BLAS of one geometry in a host bridge's own arrays"""
    inst = np.asarray(bridge.instances, f32).reshape(-1, 36).view(np.uint32)
    off = int(inst[inst[:, 34] == geometry][0, 32])
    return C.tree_shape(np.asarray(bridge.blas, f32).reshape(-1, 8)[off:], n_tris)


@pytest.mark.gpu
def test_skinned_mesh_whose_tree_changes_shape_between_frames(W):
    """rt_world_update with level counts learnt from the previous frame's tree, on a mesh that is balanced at t = 0 and skewed at
    t = 1 (shape_changing_skinned_glb): going 0 -> 1 the tree gains more than 2 levels and more than 3 large-node levels
    (read from the HOST bridge's blas array), so the update builds again and large nodes pass through the generic level
    kernels; going 1 -> 0 both counts are far too large.  Device arrays equal host arrays at every time."""
    n_tris = 16384
    glb = shape_changing_skinned_glb(n_tris)
    r = W.WebGPURenderer(0)
    cpu_b, dev_b = W.WorldBridge(), W.WorldBridge()
    dev_b.setDeviceUpdater(r)
    cpu_b.loadScene("viewer", glbData=glb)
    dev_b.loadScene("viewer", glbData=glb)
    shapes = []
    for t in (0.0, 1.0, 0.0, 1.0, 0.5):
        cpu_b.update(t)
        dev_b.update(t)
        shapes.append(_geometry_tree(cpu_b, 2, n_tris))
        print("t=%g: host tree depth %d, large-node levels %d, largest leaf %d" % (t, shapes[-1].depth, shapes[-1].big_levels, shapes[-1].largest_leaf))
        assert dev_b.deviceResident, dev_b.deviceWarning
        _same(r, cpu_b, "shape-changing skin t=%g" % t)
    assert all(s.largest_leaf <= 7 for s in shapes)             # no overflowed leaf words: tree_shape means what it says
    for a, b in ((0, 1), (2, 3)):
        assert shapes[b].depth > shapes[a].depth + 2
        assert shapes[b].big_levels > shapes[a].big_levels + 3
    r.destroy()
