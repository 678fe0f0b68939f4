"""Shared pieces of the frame-motion tests (RT_FRAME_TEMPORAL_MOTION): the reference model of the rule
(tests/model/frame_motion_model.cpp), built with the flags of oracle/Makefile as the other models are, as a library and as a
stand-alone program; the scene arrays the stage follows indices into, as a small class; what a context keeps between frames -
frame_temporal_util.History plus the snapshot; a whole call as prepare -> carry -> stage -> passes -> finish; and a small
ray caster that makes the inputs of the stage for hand-built scenes of a few triangles."""
import ctypes
import functools
import os

import numpy as np

import frame_denoise_util as fu
import frame_temporal_util as tu
import model_build
import radiance_util as ru

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "model", "frame_motion_model.cpp")
LIB = os.path.join(HERE, "model", "_build", "libframe_motion_model.so")
PROGRAM = os.path.join(HERE, "model", "_build", "frame_motion_model_san")
SAME_INSTANCE, MOTION = 1, 2
BACKGROUND, UNTRACKED, UNMOVED, MOVED = 0, 1, 2, 3
NO_ID = 0xffffffff
F = np.float32
U = fu.U


@functools.lru_cache(maxsize=None)
def model_lib():
    L = ctypes.CDLL(model_build.build(SRC, LIB, ru.FLAGS + ["-I", os.path.join(REPO, "include"), "-shared"]))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.fm_model_carry.argtypes = [vp, vp, vp, u32, vp, u32, vp, u32, vp, vp, vp, u32, u32, vp, vp]
    L.fm_model_carry.restype = None
    L.fm_model_scatter.argtypes = [vp, u32, vp, vp]
    L.fm_model_scatter.restype = None
    L.fm_model_stage.argtypes = [vp] * 9 + [u32, u32] + [vp] * 4
    L.fm_model_stage.restype = ctypes.c_int
    return L


def sanitized_program():
    """the model as a stand-alone program (its own main: every UNTRACKED cause on arrays of their exact sizes) under
    AddressSanitizer and UBSan -> path"""
    flags = [f for f in ru.FLAGS if f not in ("-fPIC", "-O2")] + ["-O1", "-g", "-fsanitize=address,undefined",
                                                                   "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "include")]
    return model_build.build(SRC, PROGRAM, flags, program=True)


class Scene:
    """the arrays the stage follows G-buffer indices into: topo (n_tris, 20) u32 rows, pos (n_verts, 4) f32, inst (n_inst, 36)
    f32 in TLAS order, ids (n_inst,) u32 or None (the identity)"""

    def __init__(self, topo, pos, inst, ids=None):
        self.topo = np.ascontiguousarray(topo, np.uint32).reshape(-1, 20)
        self.pos = np.ascontiguousarray(pos, F).reshape(-1, 4)
        self.inst = np.ascontiguousarray(inst, F).reshape(-1, 36)
        self.ids = None if ids is None else np.ascontiguousarray(ids, np.uint32).reshape(-1)

    def sid(self, p):
        return int(p if self.ids is None else self.ids[p])


class History(tu.History):
    """frame_temporal_util.History and the snapshot: positions, transforms by stable id, the id plane"""

    def __init__(self):
        super().__init__()
        self.snap_pos = self.snap_xf = self.pix_id = None


def _p(a):
    return None if a is None else a.ctypes.data


def carry(normal_id, guide, scene, state):
    """the motion stage by the model -> carry (H, W, 8) f32, pix_id (H, W) u32; state: a History (its snapshot, or none)"""
    nid, guide = np.ascontiguousarray(normal_id, F), np.ascontiguousarray(guide, F)
    H, W = guide.shape[:2]
    out, pid = np.empty((H, W, 8), F), np.empty((H, W), np.uint32)
    have = state.hist is not None and state.snap_pos is not None
    model_lib().fm_model_carry(_p(nid), _p(guide), _p(scene.topo), len(scene.topo), _p(scene.pos), len(scene.pos), _p(scene.inst),
                               len(scene.inst), _p(scene.ids), _p(state.snap_pos) if have else None,
                               _p(state.snap_xf) if have else None, W, H, _p(out), _p(pid))
    return out, pid


def stage(col, guide, normal_id, uniforms, d, scene, state):
    """One run of motion + temporal stage by the model; state advanced IN PLACE, the snapshot taken after the stage, the
    history dropped first when the snapshot's counts differ.  -> integ (H, W, 4), accepted (H, W) u32, carry (H, W, 8)"""
    d = tu.desc(**d) if isinstance(d, dict) else np.ascontiguousarray(d, tu.DESC_DTYPE)
    assert int(d["flags"][0]) & MOTION
    col, guide = np.ascontiguousarray(col, F), np.ascontiguousarray(guide, F)
    H, W = col.shape[:2]
    if state.hist is not None and (len(state.snap_pos) != len(scene.pos) or len(state.snap_xf) != len(scene.inst)):
        state.__init__()
    c, pid = carry(normal_id, guide, scene, state)
    integ, hist, mom = np.empty((H, W, 4), F), np.empty((H, W, 4), F), np.empty((H, W, 2), F)
    acc = np.zeros((H, W), np.uint32)
    have = state.hist is not None
    if have:
        ph, pm, pg = (np.ascontiguousarray(a, F) for a in (state.hist, state.mom, state.guide))
        pu = np.ascontiguousarray(state.uniforms, np.uint8)
        pi = np.ascontiguousarray(state.pix_id, np.uint32)
    r = model_lib().fm_model_stage(_p(col), _p(guide), _p(c), _p(ph) if have else None, _p(pm) if have else None,
                                   _p(pg) if have else None, _p(pi) if have else None, _p(pu) if have else None, _p(d), W, H,
                                   _p(integ), _p(hist), _p(mom), _p(acc))
    assert r == 0, "the model refuses this descriptor"
    state.hist, state.mom, state.guide, state.pix_id = hist, mom, guide.copy(), pid
    state.uniforms = np.array(uniforms, np.uint8)
    state.frames += 1
    state.snap_pos = scene.pos.copy()
    state.snap_xf = np.zeros((len(scene.inst), 16), F)
    model_lib().fm_model_scatter(_p(scene.inst), len(scene.inst), _p(scene.ids), _p(state.snap_xf))
    return integ, acc, c


def call(fr, scene, d, t, state):
    """A whole call with both stages on: prepare -> carry -> stage -> passes -> finish (frame_temporal_util.call with the flag).
    -> out (H, W, 4), integ, accepted, carry"""
    dd = fu.desc(**d) if isinstance(d, dict) else np.ascontiguousarray(d, fu.DESC_DTYPE)
    demod = int(dd["flags"][0]) & fu.DEMODULATE
    if state.hist is not None and getattr(state, "demod", demod) != demod:
        state.__init__()
    state.demod = demod
    col, guide, mod = fu.prepare(fr, int(dd["flags"][0]))
    integ, acc, c = stage(col, guide, fr.normal_id, fr.uniforms, t, scene, state)
    return tu.filter_from(integ, guide, mod, dd), integ, acc, c


def status(c):
    return fu.words(c[..., 3])


# ---- hand-built scenes
def transform(translate=(0.0, 0.0, 0.0), rot_z=0.0):
    """an rt_instance (36 words): rotation about z by rot_z radians, then the translation; the inverse beside it"""
    c, s = np.cos(rot_z), np.sin(rot_z)
    m = np.eye(4)
    m[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    m[:3, 3] = translate
    r = np.zeros(36, F)
    r[0:16] = m.T.reshape(-1)                     # column-major
    r[16:32] = np.linalg.inv(m).T.reshape(-1)
    return r


def card_scene(transforms, ids=None, half=0.5, verts=None):
    """instances of ONE two-triangle card, the square [-half, half]^2 of the object's plane z = 0 (or `verts`, (4, 3)), one per
    transform: triangles (0, 1, 2) and (0, 2, 3)"""
    v = np.array([[-half, -half, 0], [half, -half, 0], [half, half, 0], [-half, half, 0]], np.float64) if verts is None else verts
    pos = np.ones((4, 4), F)
    pos[:, :3] = v
    topo = np.zeros((2, 20), np.uint32)
    topo[0, :3], topo[1, :3] = (0, 1, 2), (0, 2, 3)
    return Scene(topo, pos, np.stack(transforms), ids)


def cast(scene, uniforms, pattern, background=None):
    """The inputs of the stage for `scene` seen through the pinhole of `uniforms`, by a float64 ray caster: the nearest triangle
    per pixel.  pattern(sid, tri, b1, b2) -> rgb of a point, b1 and b2 its barycentrics along the edges v0v1 and v0v2.  ->
    col (H, W, 4) {rgb, 0.125}, guide (H, W, 8), normal_id (H, W, 4): P is the f32 rounding of the exact hit point, so no depth
    quantisation enters."""
    u32 = np.asarray(uniforms, np.uint8).view(np.uint32)
    u = np.asarray(uniforms, np.uint8).view(F).astype(np.float64)
    W, H = int(u32[53]), int(u32[54])
    eye, ll, hor, ver = u[0:3], u[4:7], u[8:11], u[12:15]
    col = np.zeros((H, W, 4), F)
    guide = np.zeros((H, W, 8), F)
    nid = np.zeros((H, W, 4), F)
    for y in range(H):
        for x in range(W):
            uu = (x + 0.5 + u[56] * W) / W
            vv = 1.0 - (y + 0.5 + u[57] * H) / H
            dr = ll + uu * hor + vv * ver - eye
            best = None
            for p in range(len(scene.inst)):
                m = scene.inst[p, :16].astype(np.float64).reshape(4, 4).T
                for t in range(len(scene.topo)):
                    a, b, c = (m[:3, :3] @ scene.pos[i, :3].astype(np.float64) + m[:3, 3] for i in scene.topo[t, :3])
                    e1, e2 = b - a, c - a
                    n = np.cross(e1, e2)
                    den = np.dot(n, dr)
                    if abs(den) < 1e-12:
                        continue
                    tt = np.dot(n, a - eye) / den
                    if tt <= 0 or (best is not None and tt >= best[0]):
                        continue
                    hp = eye + tt * dr - a
                    g = np.array([[e1 @ e1, e1 @ e2], [e1 @ e2, e2 @ e2]])
                    b1, b2 = np.linalg.solve(g, [hp @ e1, hp @ e2])
                    if b1 < 0 or b2 < 0 or b1 + b2 > 1:
                        continue
                    nn = n / np.linalg.norm(n)
                    best = (tt, p, t, b1, b2, eye + tt * dr, nn if nn @ dr < 0 else -nn)
            if best is None:
                col[y, x, :3] = 0.0 if background is None else background
                continue
            _, p, t, b1, b2, P, N = best
            col[y, x] = (*pattern(scene.sid(p), t, b1, b2), 0.125)
            guide[y, x, 0:3], guide[y, x, 4:7] = P, N
            guide[y, x, 3:4].view(np.uint32)[:] = p
            guide[y, x, 7:8].view(np.uint32)[:] = 1
            nid[y, x, 2:4].view(np.uint32)[:] = (t, p)
    return col, guide, nid


# ---- sequence (a) of the GPU tests: a hand-built scene on the upload path.  An emissive back wall and two instances of one
# two-triangle card; card A translates and rotates, card B stays; the order of the instance array - the TLAS order - changes
# every frame and the stable ids are declared beside it.
SEQ_A_ORDERS = ((0, 1, 2), (0, 2, 1), (2, 0, 1))        # declaration index at each TLAS position, per frame
# at 260 x 2 the camera stands to the left, so that the moving card lies across columns 255 | 256, the seam of the blocks
SEQ_A_EYE_X = {(260, 2): -2.55}


def _rt_instance(m, blas_offset, geom):
    row = np.zeros(36, F)
    m32 = m.astype(F)
    row[0:16] = m32.T.reshape(-1)
    row[16:32] = np.linalg.inv(m32.astype(np.float64)).astype(F).T.reshape(-1)
    row.view(np.uint32)[32:36] = [blas_offset, 0, geom, 0]
    return row


def _matrix(translate, rot_z=0.0):
    c, s = np.cos(rot_z), np.sin(rot_z)
    m = np.eye(4)
    m[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    m[:3, 3] = translate
    return m


def sequence_a(k, width, height):
    """frame k = 0, 1, 2 -> (bridge, ids): a random_scene.Bridge with every array of the upload path, and the stable id of the
    instance at each position of its instance array"""
    import random_scene as rs
    quad = lambda hx, hy: np.array([[-hx, -hy, 0], [hx, -hy, 0], [hx, hy, 0], [-hx, hy, 0]], F)
    V = np.concatenate([quad(8.0, 8.0), quad(0.5, 1.5)])
    vertices = np.concatenate([V, np.ones((8, 1), F)], axis=1).reshape(-1)
    normals = np.tile(np.array([0, 0, 1, 0], F), 8)
    uvs = np.zeros(16, F)
    topo = np.zeros((4, 20), np.uint32)
    tf = topo.view(F)
    for t, (v, g) in enumerate((((0, 1, 2), 0), ((0, 2, 3), 0), ((4, 5, 6), 1), ((4, 6, 7), 1))):
        topo[t, 0:3], topo[t, 3] = v, g
        tf[t, 4:7] = (2.0, 2.0, 2.0) if g == 0 else (0.7, 0.5, 0.3)
        tf[t, 7] = 3.0 if g == 0 else 0.0
        tf[t, 9], tf[t, 10] = 1.0, 1.5
        tf[t, 12:16] = -1.0
        tf[t, 16:19] = (2.0, 2.0, 2.0) if g == 0 else 0.0
        tf[t, 19] = -1.0
    blas_nodes = []
    for g, first in ((0, 0), (1, 2)):
        v = V[4 * g:4 * g + 4]
        blas_nodes.append([v.min(axis=0) - 1e-3, v.max(axis=0) + 1e-3, 1, (first << 3) | 2])
    mats = [_matrix((0.0, 0.0, -4.0)), _matrix((-0.7 + 0.15 * k, 0.02 * k, -2.0 + 0.03 * k), 0.04 * k), _matrix((0.7, 0.0, -2.2))]
    geoms = (0, 1, 1)
    order = SEQ_A_ORDERS[k]
    rows, lo, hi = [], [], []
    for d in order:
        rows.append(_rt_instance(mats[d], geoms[d], geoms[d]))
        v = V[4 * geoms[d]:4 * geoms[d] + 4].astype(np.float64)
        w = (mats[d][:3, :3] @ v.T).T + mats[d][:3, 3]
        lo.append(w.min(axis=0) - 1e-3)
        hi.append(w.max(axis=0) + 1e-3)
    lo, hi = np.array(lo), np.array(hi)
    tlas = [[lo.min(axis=0), hi.max(axis=0), 5, 0], [lo[0], hi[0], 2, (0 << 3) | 1],
            [lo[1:].min(axis=0), hi[1:].max(axis=0), 5, 0], [lo[1], hi[1], 4, (1 << 3) | 1], [lo[2], hi[2], 5, (2 << 3) | 1]]
    wall_at = order.index(0)
    lights = np.array([wall_at, 0, wall_at, 1], np.uint32)
    draw = np.array([c for p, d in enumerate(order) for c in (6, 1, 0 if geoms[d] == 0 else 6, p)], np.uint32)
    cam = np.zeros(24, F)
    eye = np.array([SEQ_A_EYE_X.get((width, height), 0.0), 0.0, 0.0], F)
    cam[0:3] = eye
    cam[4:7] = eye + np.array([-1, -1, -1], F)
    cam[8:11], cam[12:15] = (2, 0, 0), (0, 2, 0)
    cam[16:19], cam[20:23] = (1, 0, 0), (0, 1, 0)
    b = rs.Bridge(vertices=vertices, normals=normals, uvs=uvs, mesh_topology=topo.reshape(-1), tlas=rs._pack(tlas),
                  blas=rs._pack(blas_nodes), instances=np.concatenate(rows), lights=lights, draw_commands=draw, cameraData=cam,
                  textures=None)
    return b, np.array(order, np.uint32)


def scene_of(b, ids):
    return Scene(b.mesh_topology, b.vertices, b.instances, ids)


def upload_frame(pkg, r, b, ids, width, height, first):
    """frame of a sequence on any renderer: the whole scene at first (upload_scene sizes the screen, which drops every
    history), then only what changes - BVH, instances, lights, draw commands - and the ids where the renderer has them"""
    if first:
        pkg.upload_scene(r, b, width, height)
    else:
        r.updateCombinedBVH(b.tlas, b.blas)
        r.updateBuffer("instance", b.instances)
        r.updateBuffer("lights", b.lights)
        r.updateBuffer("draw_commands", b.draw_commands)
        r.updateSceneUniforms(b.cameraData, 0, b.lightCount)
    if hasattr(r, "setFrameMotionIds"):
        r.setFrameMotionIds(ids)
    r.resetAccumulation()


def sequence_conditions(carry, n, guide, width, height):
    """what the middle frame of a sequence must exercise at the shapes above 40 pixels: MOVED pixels with history, UNMOVED
    pixels, pixels without history; at 260 x 2, MOVED pixels on both sides of the seam of the 256-thread blocks"""
    if width * height <= 40:
        return
    s = status(carry)
    surf = fu.words(guide[..., 7]) != 0
    assert ((s == MOVED) & (n >= 2)).any() and (s == UNMOVED).any() and (surf & (n == 1)).any(), (width, height)
    if width > 256:
        cols = np.nonzero(s == MOVED)[1]
        assert (cols <= 255).any() and (cols >= 256).any(), "the moving card lies across the seam of the 256-thread blocks"


# ---- the quality gate: tests/random_scene.py's scene with one instance translated, its TLAS rebuilt around it
def moved_random_scene(b0, which, shift):
    """random_scene's bridge `b0` with the instance of declaration index `which` (its position in b0's instance array)
    translated by `shift` world units: the instance array re-sorted by a TLAS rebuilt over the new boxes, lights and draw
    commands with it.  -> (bridge, ids): ids[p] = the position in b0 of the instance now at p"""
    import random_scene as rs
    topo = np.asarray(b0.mesh_topology, np.uint32).reshape(-1, 20)
    pos = np.asarray(b0.vertices, F).reshape(-1, 4)[:, :3].astype(np.float64)
    rows = np.array(b0.instances, F).reshape(-1, 36).copy()
    m = rows[which, 0:16].reshape(4, 4).T.astype(np.float64)
    m[:3, 3] += shift
    rows[which, 0:16] = m.astype(F).T.reshape(-1)
    rows[which, 16:32] = np.linalg.inv(m.astype(F).astype(np.float64)).astype(F).T.reshape(-1)
    n = len(rows)
    lo, hi, ranges = np.zeros((n, 3)), np.zeros((n, 3)), []
    for i in range(n):
        g = int(rows[i].view(np.uint32)[34])
        tri = np.nonzero(topo[:, 3] == g)[0]
        ranges.append((int(tri[0]), len(tri)))
        v = pos[np.unique(topo[tri, 0:3])]
        mi = rows[i, 0:16].reshape(4, 4).T.astype(np.float64)
        w = v @ mi[:3, :3].T + mi[:3, 3]
        lo[i], hi[i] = w.min(axis=0) - 1e-3, w.max(axis=0) + 1e-3
    order = np.arange(n)
    tl = rs._build_bvh(lo, hi, order, np.random.default_rng(7), 1, lambda first, count: (first << 3) | 1)
    lights, draw = [], []
    for si, i in enumerate(order):
        start, cnt = ranges[i]
        draw += [cnt * 3, 1, start * 3, si]
        for k in range(cnt):
            if topo[start + k, 7:8].view(F)[0] == 3.0:
                lights += [si, start + k]
    b = rs.Bridge(vertices=b0.vertices, normals=b0.normals, uvs=b0.uvs, mesh_topology=b0.mesh_topology, tlas=rs._pack(tl),
                  blas=b0.blas, instances=np.concatenate([rows[i] for i in order]), lights=np.array(lights, np.uint32),
                  draw_commands=np.array(draw, np.uint32), cameraData=b0.cameraData, textures=b0.textures)
    return b, order.astype(np.uint32)
