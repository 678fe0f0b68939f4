"""Drive the HIP renderer and the CPU oracle with the same call sequence and compare every
parity artefact of SURVEY.md §8(d): accumulation buffer, G-buffer planes, history, RGBA8 output,
uniform block and the deterministic ray counters."""
import numpy as np

DIAMOND_OBJ = ("v 0.0 1.0 0.0\nv 1.0 0.0 0.0\nv 0.0 0.0 1.0\nv -1.0 0.0 0.0\nv 0.0 0.0 -1.0\nv 0.0 -1.0 0.0\n"
               "f 1 3 2\nf 1 2 5\nf 1 5 4\nf 1 4 3\nf 6 2 3\nf 6 5 2\nf 6 4 5\nf 6 3 4\n")

# the ray counters every build maintains (nodes_visited, tris_tested and shaded_hits: the counting build only)
RAY_COUNTERS = ("primary_rays", "extension_rays", "shadow_rays")

LDS_PER_CU = 160 * 1024
WAVE_QUEUE = 64 * 32 + 64 * 7 * 4 + 64 * 8   # RT_WORK_BYTES_PER_WAVE
COL_PARK = 64 * 12                           # RT_PT_COL_BYTES_PER_WAVE

_bridges = {}


def dyn_lds(b):
    """Dynamic LDS of one workgroup of the persistent kernel's LDS form for the bridge `b` (rt_api.hip: four wave queues +
    launch_plan.h scene_lds_slots x 16 bytes)."""
    n_nodes = (len(b.tlas) + len(b.blas)) // 8
    n_tris, n_inst = len(b.mesh_topology) // 20, len(b.instances) // 36
    n_verts, n_lights = len(b.vertices) // 4, len(b.lights) // 2
    slots = (2 * n_nodes + 3 * n_tris + 4 * n_inst + (n_inst + 3) // 4 + 8 * n_tris + 5 * n_tris + n_verts +
             (n_verts + 1) // 2 + 9 * n_inst + (n_lights + 1) // 2 + 4 * n_lights)
    return 4 * WAVE_QUEUE + 16 * slots


def takes_wide_form(b):
    """the host runs a batched product dispatch of the one-leaf scene `b` in 512-thread workgroups: three of them, each with
    eight wave queues and eight waves' parked sample sums, fit the CU's LDS (tests/test_gpu_one_leaf_wide.py)"""
    return dyn_lds(b) + 4 * WAVE_QUEUE + 8 * COL_PARK <= LDS_PER_CU // 3


def diamond_obj_subdivided(n=11):
    """BASELINE.json words config 2 as a "~1k tris" diamond; public/diamond.obj is the 8-triangle octahedron.  Config 2b:
    the same octahedron with every face cut into n x n congruent triangles (n = 11: 968 triangles, 486 vertices on the
    flat faces — same shape, a deeper BLAS), as OBJ text for the `viewer` scene."""
    base_v = [(0, 1, 0), (1, 0, 0), (0, 0, 1), (-1, 0, 0), (0, 0, -1), (0, -1, 0)]
    base_f = [(1, 3, 2), (1, 2, 5), (1, 5, 4), (1, 4, 3), (6, 2, 3), (6, 5, 2), (6, 4, 5), (6, 3, 4)]
    verts, index, faces = [], {}, []

    def vid(p):
        key = tuple(round(c * n) for c in p)          # barycentric lattice points are exact multiples of 1/n
        if key not in index:
            index[key] = len(verts) + 1
            verts.append(tuple(k / n for k in key))
        return index[key]

    for fa, fb, fc in base_f:
        a, b, c = (np.array(base_v[i - 1], dtype=np.float64) for i in (fa, fb, fc))
        grid = {}
        for i in range(n + 1):
            for j in range(n + 1 - i):
                grid[i, j] = vid(a + (b - a) * (i / n) + (c - a) * (j / n))
        for i in range(n):
            for j in range(n - i):
                faces.append((grid[i, j], grid[i + 1, j], grid[i, j + 1]))
                if j < n - i - 1:
                    faces.append((grid[i + 1, j], grid[i + 1, j + 1], grid[i, j + 1]))
    return "".join("v %.9g %.9g %.9g\n" % v for v in verts) + "".join("f %d %d %d\n" % f for f in faces)


def bridge_for(pkg, scene):
    if scene not in _bridges:
        b = pkg.WorldBridge()
        if scene == "viewer_diamond":
            b.loadScene("viewer", DIAMOND_OBJ)
        elif scene == "viewer_diamond_1k":
            b.loadScene("viewer", diamond_obj_subdivided())
        else:
            b.loadScene(scene)
        _bridges[scene] = b
    return _bridges[scene]


def drive(renderer, pkg, bridge, w, h, depth, spp, frames, present=True, detailed=True):
    renderer.buildPipeline(depth, spp)
    pkg.upload_scene(renderer, bridge, w, h)
    if hasattr(renderer, "setCounting"):
        renderer.setCounting(detailed)
    renderer.resetCounters()
    for f in frames:
        renderer.compute(f)
        if present:
            renderer.present()
    renderer.sync()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 1: np.uint8, 8: np.uint64}[a.dtype.itemsize])


def describe_mismatch(name, a, b):
    ne = bits(a) != bits(b)
    idx = np.argwhere(ne)
    first = tuple(idx[0])
    return "%s differs at %d of %d elements; first at %s: gpu=%r oracle=%r" % (
        name, int(ne.sum()), ne.size, first, a[first], b[first])


def assert_accum_against_oracle(got, want, what, nan_as_class=False):
    """The accumulation-buffer twin of radiance_util.check_records_against_model.  got, want: (h, w, 4) f32, the renderer's
    and the oracle's.  Bit for bit, word by word.  nan_as_class: a word where the ORACLE has a NaN may hold a NaN of any
    payload and sign (they are not pinned across the two instruction sets); every other word stays bit-exact."""
    g, w = bits(got), bits(want)
    bad = g != w
    if nan_as_class:
        bad &= ~(np.isnan(np.asarray(got, np.float32)) & np.isnan(np.asarray(want, np.float32)))
    pixels = np.argwhere(bad.any(axis=-1))
    assert pixels.size == 0, ("accumulation buffer, " + what, "pixels that differ", len(pixels), pixels[:8].tolist(),
                              [np.asarray(got)[tuple(p)].tolist() for p in pixels[:4]],
                              [np.asarray(want)[tuple(p)].tolist() for p in pixels[:4]])


def assert_parity(gpu, cpu, check_output=True, check_counters=True):
    ga, ca = gpu.readAccum(), cpu.readAccum()
    assert np.array_equal(bits(ga), bits(ca)), describe_mismatch("accumulation buffer", ga, ca)
    if check_output:
        go, co = gpu.captureFrame()["data"], cpu.captureFrame()["data"]
        assert np.array_equal(go, co), describe_mismatch("RGBA8 output", go, co)
        gh, ch = gpu.readHistory(), cpu.readHistory()
        # +0 / -0 are the same value; compare with the sign of zero masked out
        gz, cz = gh.copy(), ch.copy()
        gz[gz == 0x8000] = 0
        cz[cz == 0x8000] = 0
        assert np.array_equal(gz, cz), describe_mismatch("history (rgba16f)", gh, ch)
    else:
        for name, g, c in zip(("albedo", "normal_id", "depth"), gpu.readGBuffer(), cpu.readGBuffer()):
            assert np.array_equal(bits(g), bits(c)), describe_mismatch("G-buffer " + name, g, c)
    assert np.array_equal(gpu.readUniforms(), cpu.readUniforms()), "uniform block differs"
    if check_counters:
        assert gpu.getCounters() == cpu.getCounters()


def check_traversal_nodes(r, b):
    """tnodes (csrc/k_treelet.hip.h) of the scene `b` uploaded to renderer `r`: a permutation of the bridge's nodes with
    both successors explicit.  Following them from the roots must walk every BLAS and the TLAS in the ORIGINAL pre-order,
    with the original boxes and leaf words.  Returns the array read back."""
    import ctypes
    tl, bl = np.asarray(b.tlas, np.float32).reshape(-1, 8), np.asarray(b.blas, np.float32).reshape(-1, 8)
    nodes = np.concatenate([tl, bl])
    n, n_tlas = len(nodes), len(tl)
    inst = np.asarray(b.instances, np.float32).reshape(-1, 36).view(np.uint32)
    tn = np.zeros((n, 8), np.float32)
    new = np.zeros(n, np.uint32)
    roots = np.zeros(len(inst), np.uint32)
    vp = ctypes.c_void_p
    got = r.L.rt_debug_read_traversal_nodes(r.ctx, tn.ctypes.data_as(vp), new.ctypes.data_as(vp), roots.ctypes.data_as(vp), n)
    assert got == n
    assert sorted(new.tolist()) == list(range(n)) and new[0] == 0           # a permutation; the TLAS root stays node 0
    u, tu = nodes.view(np.uint32), tn.view(np.uint32)
    END, INNER = 0xffffffff, 0x80000000
    # boxes travel with their node; leaves keep their word; inner nodes point at their first child, skips at the original target
    assert np.array_equal(tu[new][:, [0, 1, 2, 4, 5, 6]], u[:, [0, 1, 2, 4, 5, 6]])
    leaf = u[:, 7] != 0
    assert np.array_equal(tu[new[leaf], 7], u[leaf, 7])
    inner = np.flatnonzero(~leaf)
    reach = np.zeros(n, bool)           # nodes inside a TLAS / BLAS range that a walk can reach
    reach[:int(u[0, 3])] = True
    skip_target = np.full(n, -1, np.int64)
    skip_target[:n_tlas] = np.where(u[:n_tlas, 3] < u[0, 3], u[:n_tlas, 3].astype(np.int64), -1)
    for off in sorted(set(inst[:, 32].tolist())):
        root = n_tlas + off
        end = root + int(u[root, 3])
        reach[root:end] = True
        tgt = root + u[root:end, 3].astype(np.int64)
        skip_target[root:end] = np.where(tgt < end, tgt, -1)
    ri = inner[reach[inner]]
    assert np.array_equal(tu[new[ri], 7], INNER | new[ri + 1])
    rr = np.flatnonzero(reach)
    expect = np.where(skip_target[rr] >= 0, new[np.maximum(skip_target[rr], 0)], END).astype(np.uint32)
    assert np.array_equal(tu[new[rr], 3], expect)
    assert np.array_equal(roots, new[n_tlas + inst[:, 32]])
    return tn


def check_pair_records(r, b):
    """The child-pair records the trace kernels walk (csrc/k_pairs.hip.h, built on the GPU at upload) for the scene `b`
    uploaded to renderer `r`, against tests/pair_layout.py, byte for byte."""
    import ctypes
    import pair_layout
    pairs, troot, inst_root = pair_layout.build(b.tlas, b.blas, b.instances)
    got_pairs = np.zeros((len(pairs) + 1, 16), np.float32)
    got_roots = np.zeros((len(inst_root) + 1, 8), np.float32)
    vp = ctypes.c_void_p
    n = r.L.rt_debug_read_pairs(r.ctx, got_pairs.ctypes.data_as(vp), got_roots.ctypes.data_as(vp), len(got_pairs))
    assert n == len(pairs)
    assert np.array_equal(got_pairs[:n].view(np.uint32), pairs.view(np.uint32))
    assert np.array_equal(got_roots[:-1].view(np.uint32), inst_root.view(np.uint32))
    assert np.array_equal(got_roots[-1].view(np.uint32), troot.view(np.uint32))
