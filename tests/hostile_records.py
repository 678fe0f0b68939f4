"""Hostile topology records: copies of a random_scene bridge (with textures) in which chosen triangles carry ONE field that
no exporter writes - a non-finite or out-of-range material word, roughness, ior, metallic, albedo, emission, texture word,
vertex uv or vertex normal.  rt_upload accepts any float in these words (k_validate_scene checks indices only), so every
kernel form has to shade them exactly as the oracle does.  The fields are grouped into families; a family is one scene.

The hostile triangles are chosen among those a centroid ray reaches first (centroid_rays, query_set) and that are a depth-0
hit of every frame of the camera's picture at both sizes of the tests (picture_triangles), so that every one is shaded at
depth 0 by every frame form and by a ray of the query set; none is in the light list, so that a family's picture is not one
NaN.  To have ten such triangles in a picture that is mostly lit, the scenes are random_scene's with every triangle enlarged
(enlarged), vertex normals that follow the surfaces (with_surface_normals) and a fixed camera window (_windowed).  Where the field is only read by one material, the triangle is given
that material too (metallic, roughness: GGX; ior: dielectric), and a triangle with hostile uvs is given a base-colour
texture: the companion makes the hostile field live, it is not a second hostile field."""
import numpy as np

import random_scene

INF, NAN = np.float32(np.inf), np.float32(np.nan)
DENORMAL = np.float32(1e-40)
T_MIN = 0.001
# words of the 20-word triangle record (rt_topology)
ALBEDO, MAT, METALLIC, ROUGHNESS, IOR, TEX, EMISSION = 4, 7, 8, 9, 10, 12, 16
_BELOW, _AT, _ABOVE = (np.nextafter(np.float32(1e-4), np.float32(0)), np.float32(1e-4),
                       np.nextafter(np.float32(1e-4), np.float32(1)))


def clone(b, **kw):
    d = {k: v for k, v in b.__dict__.items() if k not in ("hasNewData", "hasNewGeometry")}
    d.update(kw)
    return random_scene.Bridge(**d)


def multi_instance(seed=31, tris=34):
    """six instances of three geometries, small enough for the forms that hold the whole scene in LDS"""
    b = random_scene.make(seed, tris_per_geom=tris, with_textures=True)
    return _windowed(with_surface_normals(enlarged(b, 2.5)), (0.21, 0.34), 0.2)


def one_leaf(seed=1, tris=30):
    """a single-instance scene of about 30 triangles whose TLAS is one leaf (tests/test_gpu_world_records.py _one_leaf)"""
    b = random_scene.make(seed, n_geoms=1, tris_per_geom=tris, n_instances=1, with_textures=True)
    assert len(b.tlas) // 8 == 1 and len(b.instances) // 36 == 1, "not a one-leaf TLAS"
    return _windowed(with_surface_normals(enlarged(b, 3.0)), (-0.29, -0.24), 0.3)


def topology(b):
    return np.array(b.mesh_topology, np.uint32).reshape(-1, 20).copy()


def instance_triangles(b):
    """[(instance, first triangle, count)] from the draw commands"""
    d = np.asarray(b.draw_commands, np.uint32).reshape(-1, 4)
    return [(int(si), int(start) // 3, int(cnt) // 3) for cnt, _, start, si in d]


def world_triangles(b):
    """-> (inst (m,), tri (m,), corners (m, 3, 3) f64 in world space) of every triangle of every instance"""
    pos = np.asarray(b.vertices, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    idx = topology(b)[:, 0:3].astype(np.int64)
    rows = np.asarray(b.instances, np.float32).reshape(-1, 36)
    inst, tri, corners = [], [], []
    for si, first, count in instance_triangles(b):
        m = rows[si, 0:16].reshape(4, 4).T.astype(np.float64)          # column-major
        t = np.arange(first, first + count)
        p = pos[idx[t]]                                                # (count, 3, 3)
        corners.append(p @ m[:3, :3].T + m[:3, 3])
        inst.append(np.full(count, si))
        tri.append(t)
    return np.concatenate(inst), np.concatenate(tri), np.concatenate(corners)


def _refit(nodes, base, end, leaf_box):
    """boxes of the stackless pre-order tree nodes[base:end] (skips relative to `base`) again from its leaves: a node's box is
    the union of the boxes of the leaves of its subtree, the nodes from itself up to its skip"""
    u = nodes.view(np.uint32)
    lo, hi = {}, {}
    for i in range(base, end):
        if u[i, 7]:
            lo[i], hi[i] = leaf_box(int(u[i, 7]))
    for i in range(base, end):
        leaves = [k for k in range(i, base + int(u[i, 3])) if k in lo]
        nodes[i, 0:3] = np.min([lo[k] for k in leaves], axis=0)
        nodes[i, 4:7] = np.max([hi[k] for k in leaves], axis=0)


def enlarged(b, factor):
    """`b` with every triangle scaled by `factor` about its centroid and the boxes of both BVH levels fitted again (same
    trees, same leaves, margins as random_scene leaves them).  The triangles of random_scene are small beside the space
    between them: a window that shows ten of them is mostly background."""
    idx = topology(b)[:, 0:3].astype(np.int64)
    v = np.array(b.vertices, np.float32).reshape(-1, 4).copy()
    p = v[idx][:, :, :3].astype(np.float64)
    c = p.mean(axis=1, keepdims=True)
    v[idx.reshape(-1), :3] = (c + factor * (p - c)).reshape(-1, 3).astype(np.float32)
    tri = v[idx][:, :, :3]
    blas = np.array(b.blas, np.float32).reshape(-1, 8).copy()

    def tri_box(word):
        t = tri[(word >> 3):(word >> 3) + (word & 7)].reshape(-1, 3)
        return t.min(axis=0) - np.float32(1e-4), t.max(axis=0) + np.float32(1e-4)

    root = 0
    while root < len(blas):
        end = root + int(blas.view(np.uint32)[root, 3])
        _refit(blas, root, end, tri_box)
        root = end
    tlas = np.array(b.tlas, np.float32).reshape(-1, 8).copy()
    rows = np.asarray(b.instances, np.float32).reshape(-1, 36)

    def inst_box(word):
        row = rows[word >> 3]
        m = row[0:16].reshape(4, 4).T.astype(np.float64)
        g = blas[int(row.view(np.uint32)[32])]
        corners = np.array([[x, y, z, 1.0] for x in (g[0], g[4]) for y in (g[1], g[5]) for z in (g[2], g[6])])
        wc = (corners @ m.T)[:, :3]
        return wc.min(axis=0) - 1e-3, wc.max(axis=0) + 1e-3

    _refit(tlas, 0, len(tlas), inst_box)
    return clone(b, vertices=v.reshape(-1), blas=blas.reshape(-1), tlas=tlas.reshape(-1))


def frame_triangles(b, width, height, depth=1, frames=(1, 2, 3)):
    """-> (oracle renderer after the frames, [{triangle: pixels it gets at depth 0} of every frame]) by the oracle's primary
    pass; every frame has its own sub-pixel jitter, so a small triangle can be in one and not in the next"""
    import oracle_lib
    import parity_util as pu
    import webgpu_raytracer_amd as W
    cpu = oracle_lib.OracleRenderer()
    pu.drive(cpu, W, b, width, height, depth, 1, (), present=False)
    out = []
    for f in frames:
        cpu.compute(f)
        _, normal_id, z = cpu.readGBuffer()
        hit = np.asarray(z).reshape(-1) < 1.0
        tris, count = np.unique(pu.bits(normal_id).reshape(-1, 4)[:, 2][hit], return_counts=True)
        out.append(dict(zip(tris.tolist(), count.tolist())))
    return cpu, out


def picture_triangles(b, sizes=((37, 29), (24, 16))):
    """{triangle: fewest pixels it gets at depth 0 in any frame at any of the `sizes`} of the triangles that are in every
    frame at every size (geometry alone decides it: the same in every family of a scene)"""
    least = None
    for w, h in sizes:
        for here in frame_triangles(b, w, h)[1]:
            least = here if least is None else {t: min(n, here[t]) for t, n in least.items() if t in here}
    return least


def _windowed(b, mid, half):
    """`b` with the camera's window centred on `mid` of the view plane (three units in front of the eye), `half` to either
    side, at 4 : 3.  The window of random_scene looks at open space around the objects, and the background is black; the
    windows of the two scenes here were picked by hand where the picture is dense, lit, and shows ten triangles and more
    outside the light list at both sizes of the tests (tests/test_hostile_records_model.py asserts all three)."""
    cam = np.array(b.cameraData, np.float32).copy()
    eye = cam[0:3].astype(np.float64)
    h = np.array([2 * half, 0, 0])
    v = np.array([0, 1.5 * half, 0])
    cam[4:7] = eye + np.array([mid[0], mid[1], 3.0]) - h / 2 - v / 2
    cam[8:11], cam[12:15] = h, v
    return clone(b, cameraData=cam)


def good_share(accum):
    """share of the pixels of an accumulation buffer that are finite and not black"""
    a = np.asarray(accum)[..., :3]
    return float((np.isfinite(a).all(axis=-1) & (a != 0).any(axis=-1)).mean())


def with_surface_normals(b, seed=5, tilt=0.3):
    """`b` with vertex normals that belong to its surfaces: the triangle's geometric normal, tilted by a random vector of
    length <= `tilt`.  random_scene draws vertex normals that know nothing of the geometry; half of all scattered rays then
    leave below the surface and end the path, and half of a picture stays black whatever the materials are."""
    rng = np.random.default_rng(seed)
    pos = np.asarray(b.vertices, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    idx = topology(b)[:, 0:3].astype(np.int64)
    n = np.cross(pos[idx[:, 1]] - pos[idx[:, 0]], pos[idx[:, 2]] - pos[idx[:, 0]])
    length = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(length > 0, n / np.maximum(length, 1e-300), [0.0, 0.0, 1.0])
    normals = np.array(b.normals, np.float32).reshape(-1, 4).copy()
    for k in range(3):
        v = n + rng.uniform(-1, 1, n.shape) * (tilt / np.sqrt(3.0))
        normals[idx[:, k], :3] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    return clone(b, normals=normals.reshape(-1))


def centroid_rays(b, distance=0.05):
    """Two rays per triangle of every instance, aimed at its world-space centroid along the geometric normal, one from either
    side, starting `distance` away.  -> (rays (m, 8) f32 in the rt_ray layout, pad = 7 i + 3; inst (m,); tri (m,))"""
    inst, tri, p = world_triangles(b)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    length = np.linalg.norm(n, axis=1)
    ok = length > 1e-9                                                 # a zero-area triangle has no side to look at
    inst, tri, p, n = inst[ok], tri[ok], p[ok], n[ok] / length[ok, None]
    c = p.mean(axis=1)
    rays = np.zeros((2 * len(c), 8), np.float32)
    for k, sign in enumerate((1.0, -1.0)):
        rays[k::2, 0:3] = c + sign * distance * n
        rays[k::2, 4:7] = -sign * n
    rays[:, 3] = 1e30
    rays.view(np.uint32)[:, 7] = (np.arange(len(rays), dtype=np.uint64) * 7 + 3).astype(np.uint32)
    return rays, np.repeat(inst, 2), np.repeat(tri, 2)


def first_hits(model, rays):
    """(tri (m,), inst (m,)) of the first hit of rays in the rt_ray layout, -1 for a miss, by the model's traversal"""
    o = np.empty_like(rays)
    o[:, 0:3], o[:, 3], o[:, 4:7], o[:, 7] = rays[:, 0:3], np.float32(T_MIN), rays[:, 4:7], rays[:, 3]
    out, _ = model.traceRays(o)
    return out[:, 1].astype(np.int64), out[:, 2].astype(np.int64)


def query_set(b, model):
    """The centroid rays of `b` that reach their own triangle first -> (rays, tri).  Geometry and BVH are the same in every
    family of a scene, so this is computed on the scene itself."""
    rays, inst, tri = centroid_rays(b)
    ht, hi = first_hits(model, rays)
    own = (ht == tri) & (hi == inst)
    return np.ascontiguousarray(rays[own]), tri[own]


# ---- the families: name -> list of edits, each edit(topo, geo, t) writes one hostile field into triangle t
def _set(word, value, also=()):
    def edit(topo, geo, t):
        f = topo.view(np.float32)
        f[t, word:word + np.size(value)] = value
        for w, v in also:
            f[t, w] = v
    edit.material = dict(also).get(MAT)      # the material that reads the field: a triangle that has it already comes first
    return edit


def _uv(vertex, comp, value):
    def edit(topo, geo, t):
        topo.view(np.float32)[t, TEX] = 0.0                 # a base-colour texture reads the uv
        geo["uvs"][topo[t, vertex], comp] = value
    return edit


def _normal(vertices, comps, value=None, scale=None):
    def edit(topo, geo, t):
        for v in vertices:
            for c in comps:
                if scale is None:
                    geo["normals"][topo[t, v], c] = value
                else:
                    geo["normals"][topo[t, v], c] *= np.float32(scale)
    return edit


def _tex_edits():
    values = (-0.5, -0.4999, 0.999, "layers", 1e9, INF, NAN)
    # the 28 (value, slot) pairs: the first 7 hold every value, any 4 in a row every slot; a scene takes as many as it has
    # triangles in its picture
    return [(v, k % 4) for k, v in enumerate(values * 4)]


FAMILIES = {
    "material_id": [_set(MAT, v) for v in (-1.0, 0.49, 0.5, 2.5, 3.4, 4.0, 1e9, INF, -INF, NAN)],
    "metallic": [_set(METALLIC, v, also=((MAT, 1.0),)) for v in (-1.0, 2.0, NAN)],
    "roughness": [_set(ROUGHNESS, v, also=((MAT, 1.0),)) for v in (0.0, -1.0, 1e-30, INF, NAN)],
    "ior": [_set(IOR, v, also=((MAT, 2.0),)) for v in (0.0, 1.0, -1.5, 1e-30, INF, NAN)],
    "albedo": [_set(ALBEDO, v) for v in ((0.0, 0.0, 0.0), (-0.5, 0.3, 0.2), (DENORMAL,) * 3, (INF, 0.5, 0.5), (0.5, NAN, 0.5))],
    "emission": [_set(EMISSION, v) for v in ((-1.0, 0.5, 0.5), (0.5, INF, 0.5), (0.5, 0.5, NAN))],
    "emission_length": [_set(EMISSION, v) for v in ((_BELOW, 0, 0), (0, _AT, 0), (0, 0, _ABOVE))],
    "texture_words": None,          # made per scene: one value is the scene's layer count
    "vertex_uvs": [_uv(k % 3, k % 2, v) for k, v in enumerate(
        (NAN, INF, -INF, 1e30, -1e30, 2.0 ** 31, -2.0 ** 31, -0.0, DENORMAL))],
    "normals": [_normal((0, 1, 2), (0, 1, 2), 0.0), _normal((1,), (0,), NAN), _normal((2,), (1,), INF),
                _normal((0, 1, 2), (0, 1, 2), DENORMAL), _normal((0, 1, 2), (0, 1, 2), scale=37.5),
                _normal((0,), (0, 1, 2), scale=1e20), _normal((1,), (0, 1, 2), scale=1e-3)],
    # only what scene_facts.h triangle_is_plain still accepts, on a scene made plain first
    "plain_preserving": [_set(MAT, v) for v in (-1.0, 0.49, 3.4, NAN)] +
                        [_set(ALBEDO, v) for v in ((0.0, 0.0, 0.0), (-0.5, 0.3, 0.2), (DENORMAL,) * 3, (INF, 0.5, 0.5),
                                                   (0.5, NAN, 0.5))] +
                        [_set(EMISSION, (0.5, NAN, 0.5))],
}
NAMES = tuple(FAMILIES)


def decode_material(word):
    """u32(word + 0.5) as the kernel converts: truncation, saturation, NaN -> 0"""
    w = np.asarray(word, np.float32) + np.float32(0.5)
    with np.errstate(invalid="ignore"):
        return np.where(w > 0, np.minimum(np.floor(np.where(w > 0, w, 0)), 4294967295.0), 0.0).astype(np.uint64)


def is_plain(topo):
    """scene_facts.h triangle_is_plain, per record"""
    f = topo.view(np.float32)
    mat = decode_material(f[:, MAT])
    with np.errstate(invalid="ignore", over="ignore"):
        textured = (f[:, TEX:TEX + 4] > -0.5).any(axis=1)
        e = f[:, EMISSION:EMISSION + 3]
        emits = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]) > np.float32(1e-4)
    return ((mat == 0) | (mat == 3)) & ~textured & ~((mat != 3) & emits)


def made_plain(b):
    """`b` with every triangle that is not a light an untextured Lambertian without emission, and the lights untextured"""
    topo = topology(b)
    f = topo.view(np.float32)
    f[f[:, MAT] != 3.0, MAT] = 0.0
    f[:, TEX:TEX + 4] = -1.0
    f[f[:, MAT] != 3.0, EMISSION:EMISSION + 3] = 0.0
    assert is_plain(topo).all()
    return clone(b, mesh_topology=topo.reshape(-1))


def family(b, name, candidates):
    """The scene `b` with the hostile fields of family `name` -> (bridge, hostile triangles (k,)).  `candidates`: the
    triangles that may carry one (Prepared.order), in the order in which they are taken.  Every edit of the family gets a
    triangle of its own; of the texture words, the first seven (every value) must, the rest go as far as the triangles do."""
    if name == "plain_preserving":
        b = made_plain(b)
    topo = topology(b)
    geo = {"uvs": np.array(b.uvs, np.float32).reshape(-1, 2).copy(), "normals": np.array(b.normals, np.float32).reshape(-1, 4).copy()}
    edits = FAMILIES[name]
    if name == "texture_words":
        layers = float(b.textureCount)
        edits = [_set(TEX + slot, layers if v == "layers" else v) for v, slot in _tex_edits()]
    free = [int(t) for t in candidates]
    need = len(edits) if name != "texture_words" else 7
    assert len(free) >= need, (name, "triangles that may carry a hostile field", len(free), "edits", need)
    edits = edits[:len(free)]
    material = topo.view(np.float32)[:, MAT].copy()
    chosen = []
    for edit in edits:
        wanted = getattr(edit, "material", None)
        left = [t for t in free if t not in chosen]
        t = next((t for t in left if material[t] == wanted), left[0])
        chosen.append(t)
        edit(topo, geo, t)
    if name == "plain_preserving":
        assert is_plain(topo).all()
    out = clone(b, mesh_topology=topo.reshape(-1), uvs=geo["uvs"].reshape(-1), normals=geo["normals"].reshape(-1))
    return out, np.array(chosen, np.int64)


# ---- the two scenes of the tests, with their query sets, made once
_prepared = {}


class Prepared:
    """A scene of the tests: the bridge, its model (gather_util.GatherModel: the oracle, radiance queries and gathers), the
    centroid rays that reach their own triangle, the gather points just in front of their hits, and the triangles that may
    carry a hostile field: outside the light list, reached by a centroid ray, and a depth-0 hit of the camera's picture at
    both sizes of the tests - so every hostile record is shaded at depth 0 by every frame form and by a query ray.  `pixels`:
    the fewest pixels each of them gets; they are taken in the order of the triangle numbers."""

    def __init__(self, bridge):
        import gather_util as gu
        import webgpu_raytracer_amd as W
        self.bridge = bridge
        self.model = gu.model_for(W, bridge)
        self.rays, self.ray_tri = query_set(bridge, self.model)
        self.points = gu.points_from_rays(self.model, self.rays)
        reached = set(self.ray_tri.tolist())
        listed = set(np.asarray(bridge.lights, np.uint32).reshape(-1, 2)[:, 1].tolist())
        self.pixels = {int(t): n for t, n in picture_triangles(bridge).items() if t in reached and t not in listed}
        self.order = sorted(self.pixels)
        self._families = {}

    def family(self, name):
        """(bridge, hostile triangles) of a family, made once"""
        if name not in self._families:
            self._families[name] = family(self.bridge, name, self.order)
        return self._families[name]


SCENES = {"multi_instance": multi_instance, "one_leaf": one_leaf}


def prepared(scene):
    if scene not in _prepared:
        _prepared[scene] = Prepared(SCENES[scene]())
    return _prepared[scene]
