"""The frame motion rule (RT_FRAME_TEMPORAL_MOTION, include/mi355rt.h "THE FRAME MOTION RULE") held to its properties on the
reference model (tests/model/frame_motion_model.cpp), which the GPU tests then compare the kernels with word for word.  No GPU.

The scenes are hand-built cards of one or two triangles in front of the pinhole of frame_denoise_util.uniforms (eye at the
origin, image plane z = -1 spanning [-1, 1]^2), cast by frame_motion_util.cast: the guide's P is the f32 rounding of the exact
hit point, so what the tests bound is the rule's own arithmetic, not the depth plane's quantisation."""
import subprocess

import numpy as np
import pytest

import frame_denoise_util as fu
import frame_motion_util as mu
import frame_temporal_util as tu

F = np.float32
W_, H_ = 24, 16
T = dict(flags=mu.MOTION, max_history=32, var_history=4, normal_cos=0.9, plane_eps=0.01)
# "A few ulps" for a pattern of values in [0, 1.2] on these images: the footprint coordinate fx is about eight roundings at
# magnitudes up to W_ = 24 < 32, an absolute error of 8 * 32 * U pixels, and the pattern changes by at most 0.2 per pixel: 51 U;
# the barycentrics and P' are about twelve more roundings at magnitudes up to 4 with the same slope per world unit (a pixel is
# 1 / 6 world units at z = -2): 12 * 4 * U * 6 * 0.2 = 58 U; the four products and sums of the bilinear mean and the blend are
# eight roundings at magnitude 1.2: 10 U.  In all under 128 U.
EXACT = 128 * mu.U


def uniforms(jitter=(0.0, 0.0)):
    return fu.uniforms(W_, H_, jitter)


def obj_xy(tri, b1, b2, half):
    """object coordinates of a point of mu.card_scene's card"""
    return (-half + 2 * half * (b1 + b2), -half + 2 * half * b2) if tri == 0 else (-half + 2 * half * b1, -half + 2 * half * (b1 + b2))


def linear_in_object(half):
    return lambda sid, tri, b1, b2: (0.6 + 0.5 * obj_xy(tri, b1, b2, half)[0] / half, 0.6 + 0.5 * obj_xy(tri, b1, b2, half)[1] / half,
                                     0.25 + 0.125 * sid)


def run(frames, t, static=False):
    """frames: [(scene, uniforms, pattern)] -> per frame (col, integ, accepted, carry or None, state's n)"""
    st = tu.History() if static else mu.History()
    out = []
    for scene, u, pattern in frames:
        col, guide, nid = mu.cast(scene, u, pattern)
        if static:
            integ, acc = tu.stage(col, guide, u, dict(t, flags=t["flags"] & ~mu.MOTION), st)
            c = None
        else:
            integ, acc, c = mu.stage(col, guide, nid, u, t, scene, st)
        out.append(dict(col=col, guide=guide, integ=integ, acc=acc, carry=c, n=st.n().copy(), hist=st.hist.copy(), mom=st.mom.copy()))
    return out, st


def clean_masks(out, frames):
    """per frame, the pixels whose whole history is exact by construction: all four taps accepted, and each of them such a pixel
    of the frame before (a pixel at the card's edge takes fewer taps, renormalises their weights and is no longer the bilinear
    value of its point: correct, but not what an exactness test may look at - nor at whoever blends it in later)"""
    masks = [fu.words(out[0]["guide"][..., 7]) != 0]
    for k in range(1, len(out)):
        fx, fy, _ = tu.footprint(out[k]["carry"], frames[k - 1][1])
        full = out[k]["acc"] == 4
        x0, y0 = np.floor(np.where(full, fx, 0)).astype(int), np.floor(np.where(full, fy, 0)).astype(int)
        m = full.copy()
        H, W = full.shape
        for dy in (0, 1):
            for dx in (0, 1):
                qx, qy = np.clip(x0 + dx, 0, W - 1), np.clip(y0 + dy, 0, H - 1)
                m &= masks[-1][qy, qx]
        masks.append(m)
    return masks


# the descriptors of tests/test_gpu_frame_temporal.py
GPU_DESCRIPTORS = (tu.CORNELL, dict(tu.CORNELL, flags=tu.SAME_INSTANCE, max_history=2, var_history=1), dict(tu.CORNELL, max_history=1),
                   dict(tu.CORNELL, normal_cos=float("nan")))


@pytest.mark.parametrize("t", GPU_DESCRIPTORS)
def test_where_nothing_moved_the_words_are_the_static_rules(t):
    wall = mu.transform((0.0, 0.0, -3.0))
    card = mu.transform((0.3, 0.1, -2.0), 0.3)
    scene = mu.card_scene([wall, card], half=0.9)
    scene.inst[0, 0] = scene.inst[0, 5] = 4.0                       # the wall is the card scaled by 4
    frames = [(scene, fu.uniforms(W_, H_, j, eye=e), linear_in_object(0.9))
              for j, e in (((0.0, 0.0), (0, 0, 0)), ((0.004, -0.003), (0.03, 0.01, 0)), ((-0.002, 0.001), (0.13, 0.06, 0.02)))]
    moving, _ = run(frames, dict(t, flags=t["flags"] | mu.MOTION))
    static, _ = run(frames, t, static=True)
    for k, (a, b) in enumerate(zip(moving, static)):
        for key in ("integ", "hist", "mom", "acc"):
            assert np.array_equal(fu.words(a[key]) if key != "acc" else a[key], fu.words(b[key]) if key != "acc" else b[key]), (k, key)
        s = mu.status(a["carry"])
        surf = fu.words(a["guide"][..., 7]) != 0
        assert (s[surf] == (mu.UNTRACKED if k == 0 else mu.UNMOVED)).all() and (s[~surf] == mu.BACKGROUND).all(), k
    assert (static[2]["n"] >= 2).any() or t["max_history"] == 1 or t["normal_cos"] != t["normal_cos"]


def _sliding(k):
    return mu.card_scene([mu.transform((-0.3 + 0.11 * k, -0.1 + 0.05 * k, -2.0), 0.07 * k)], half=1.4)


def test_a_card_sliding_in_its_own_plane_keeps_its_own_points():
    frames = [(_sliding(k), uniforms(), linear_in_object(1.4)) for k in range(4)]
    moving, _ = run(frames, T)
    static, _ = run(frames, T, static=True)
    err_m = err_s = 0.0
    clean = clean_masks(moving, frames)
    for k in range(1, 4):
        full = clean[k]
        assert full.sum() >= 12, k
        assert (mu.status(moving[k]["carry"])[full] == mu.MOVED).all()
        assert (moving[k]["n"][full] >= 2).all() and moving[k]["n"].max() == k + 1
        err_m = max(err_m, float(np.abs(moving[k]["integ"][full, :3] - moving[k]["col"][full, :3]).max()))
        # the static rule accepts - the card stays in its plane - and blends another point's colour
        both = full & (static[k]["n"] >= 2)
        assert both.sum() * 5 >= full.sum() * 4, k
        err_s = max(err_s, float(np.abs(static[k]["integ"][both, :3] - static[k]["col"][both, :3]).max()))
    print("sliding card: motion error %.3g (%.1f U), static error %.3g" % (err_m, err_m / mu.U, err_s))
    assert err_m <= EXACT
    assert err_s > 100 * EXACT and err_s > err_m


def test_a_card_moving_along_its_normal_keeps_its_history():
    frames = [(mu.card_scene([mu.transform((0.0, 0.0, -2.0 - 0.05 * k))], half=1.4), uniforms(), linear_in_object(1.4)) for k in range(4)]
    moving, _ = run(frames, T)
    static, _ = run(frames, T, static=True)
    clean = clean_masks(moving, frames)
    for k in range(1, 4):
        surf = fu.words(moving[k]["guide"][..., 7]) != 0
        assert (static[k]["n"][surf] == 1).all(), "0.05 per frame is five times plane_eps: the static rule restarts"
        centre = clean[k]
        assert centre.sum() >= 12 and (moving[k]["n"][centre] >= 2).all()
        assert moving[k]["n"].max() == k + 1
        assert float(np.abs(moving[k]["integ"][centre, :3] - moving[k]["col"][centre, :3]).max()) <= EXACT


def test_per_vertex_deformation_is_exact_for_a_pattern_linear_in_barycentrics():
    base = np.array([[-1.7, -1.3, -2.0], [1.7, -1.2, -2.0], [-0.1, 1.5, -2.0]])
    step = np.array([[0.06, 0.02, 0.0], [-0.03, 0.05, 0.0], [0.02, -0.07, 0.0]])   # each corner on its own way, in the plane
    frames = []
    for k in range(4):
        pos = np.ones((3, 4), F)
        pos[:, :3] = base + k * step
        topo = np.zeros((1, 20), np.uint32)
        topo[0, :3] = (0, 1, 2)
        frames.append((mu.Scene(topo, pos, [mu.transform()]), uniforms(), lambda sid, tri, b1, b2: (0.1 + b1, 0.1 + b2, 0.5)))
    moving, _ = run(frames, T)
    clean = clean_masks(moving, frames)
    for k in range(1, 4):
        full = clean[k]
        assert full.sum() >= 8 and (mu.status(moving[k]["carry"])[full] == mu.MOVED).all()
        assert float(np.abs(moving[k]["integ"][full, :3] - moving[k]["col"][full, :3]).max()) <= EXACT
        assert moving[k]["n"].max() == k + 1


def test_same_instance_follows_the_ids_across_a_tlas_reorder():
    a, b = mu.transform((-0.8, 0.0, -2.0)), mu.transform((0.8, 0.0, -2.0))   # coplanar neighbours: only the instance test tells
    t = dict(T, flags=mu.MOTION | mu.SAME_INSTANCE)
    frames = [(mu.card_scene([a, b], ids=[0, 1], half=0.8), uniforms(), linear_in_object(0.8)),
              (mu.card_scene([b, a], ids=[1, 0], half=0.8), uniforms(), linear_in_object(0.8))]
    moving, _ = run(frames, t)
    static, _ = run(frames, t, static=True)
    surf = fu.words(moving[1]["guide"][..., 7]) != 0
    assert surf.sum() >= 40 and (moving[1]["n"][surf] == 2).all()   # nothing moved: every pixel finds itself
    assert (mu.status(moving[1]["carry"])[surf] == mu.UNMOVED).all(), "the instances did not move: only their positions in the TLAS"
    assert (static[1]["n"][surf] == 1).all(), "the static comparison sees another TLAS position under every pixel"
    # and it does separate the two: with a jittered second frame the footprints at the seam straddle both cards, which are
    # coplanar, and only the id test refuses the other card's taps
    jittered = [frames[0], (frames[1][0], uniforms((0.01, 0.0)), frames[1][2])]
    same, _ = run(jittered, t)
    plain, _ = run(jittered, T)
    assert (same[1]["acc"] <= plain[1]["acc"]).all() and (same[1]["acc"] < plain[1]["acc"]).sum() >= 4
    assert (same[1]["n"][fu.words(same[1]["guide"][..., 7]) != 0] == 2).sum() >= 40


def test_disocclusion_behind_a_moving_card_restarts_the_wall():
    def scene(k):
        s = mu.card_scene([mu.transform((0.0, 0.0, -3.0)), mu.transform((-0.6 + 0.5 * k, 0.0, -2.0))], half=0.6)
        s.inst[0, 0] = s.inst[0, 5] = 6.0
        return s
    frames = [(scene(k), uniforms(), lambda sid, tri, b1, b2: (0.2 + 0.6 * sid, 0.3, 0.4)) for k in range(2)]
    moving, _ = run(frames, T)
    inst0, inst1 = (fu.words(m["guide"][..., 3]) for m in moving)
    revealed = (inst1 == 0) & (inst0 == 1)
    kept = (inst1 == 0) & (inst0 == 0)
    assert revealed.sum() >= 8 and kept.sum() >= 50
    assert (moving[1]["n"][revealed] == 1).all()
    assert (moving[1]["n"][kept] == 2).sum() >= 50
    card = inst1 == 1
    assert (moving[1]["n"][card & (moving[1]["acc"] == 4)] == 2).all() and (mu.status(moving[1]["carry"])[card] == mu.MOVED).all()


def _one_pixel(scene, state, tri=0, inst=0):
    nid = np.zeros((1, 1, 4), F)
    nid[0, 0, 2:4].view(np.uint32)[:] = (tri, inst)
    guide = np.zeros((1, 1, 8), F)
    guide[0, 0, :3] = (0.1, 0.1, -2.0)
    guide[0, 0, 6] = 1.0
    guide[0, 0, 7:8].view(np.uint32)[:] = 1
    c, pid = mu.carry(nid, guide, scene, state)
    return int(mu.status(c)[0, 0]), c[0, 0], guide[0, 0], int(pid[0, 0])


def test_every_untracked_cause_gives_no_history_and_reads_nothing():
    prev = mu.card_scene([mu.transform((0.0, 0.0, -2.0)), mu.transform((5.0, 0.0, -2.0))], half=0.8)
    st = mu.History()
    col, guide, nid = mu.cast(prev, uniforms(), linear_in_object(0.8))
    mu.stage(col, guide, nid, uniforms(), T, prev, st)
    now = mu.card_scene([mu.transform((0.05, 0.0, -2.0)), mu.transform((5.0, 0.0, -2.0))], half=0.8)
    assert _one_pixel(now, st)[0] == mu.MOVED and _one_pixel(now, st, inst=1)[0] == mu.UNMOVED
    n_tris, n_verts, n_inst = len(now.topo), len(now.pos), len(now.inst)
    cases = {}
    cases["tri == n_tris"] = _one_pixel(now, st, tri=n_tris)
    cases["tri = 2^32 - 1"] = _one_pixel(now, st, tri=0xffffffff)
    cases["inst == n_inst"] = _one_pixel(now, st, inst=n_inst)
    cases["inst = 2^31"] = _one_pixel(now, st, inst=1 << 31)
    for name, v in (("vertex == n_verts", n_verts), ("vertex = 2^32 - 1", 0xffffffff)):
        for k in range(3):
            bad = mu.Scene(now.topo.copy(), now.pos, now.inst)
            bad.topo[0, k] = v
            cases["%s, corner %d" % (name, k)] = _one_pixel(bad, st)
    cases["sid == n_inst"] = _one_pixel(mu.Scene(now.topo, now.pos, now.inst, ids=[n_inst, 1]), st)
    cases["sid = 2^32 - 1"] = _one_pixel(mu.Scene(now.topo, now.pos, now.inst, ids=[0xffffffff, 1]), st)
    cases["no snapshot"] = _one_pixel(now, mu.History())
    flat = mu.Scene(now.topo.copy(), now.pos, now.inst)
    flat.topo[0, 2] = flat.topo[0, 1]
    cases["a triangle of no area"] = _one_pixel(flat, st)
    nan = mu.History()
    nan.__dict__.update(st.__dict__)
    nan.snap_pos = st.snap_pos.copy()
    nan.snap_pos[0, 0] = np.nan
    cases["a NaN vertex in the snapshot"] = _one_pixel(now, nan)
    inf = mu.Scene(now.topo, now.pos.copy(), now.inst)
    inf.pos[1, 0] = np.inf
    cases["an infinite vertex now"] = _one_pixel(inf, st)
    for name, (s, c, g, pid) in cases.items():
        assert s == mu.UNTRACKED, name
        assert np.array_equal(fu.words(c[:3]), fu.words(g[:3])) and np.array_equal(fu.words(c[4:7]), fu.words(g[4:7])), name
        want = mu.NO_ID if ("inst" in name or "sid" in name) else 0
        assert pid == want == int(fu.words(c[7:8])[0]), name
    # ... and through the temporal stage each is the no-history path: n == 1, the colour passed through bit for bit
    bad = mu.Scene(now.topo.copy(), now.pos, now.inst)
    bad.topo[:, 0] = n_verts
    col, guide, nid = mu.cast(now, uniforms(), linear_in_object(0.8))
    integ, acc, c = mu.stage(col, guide, nid, uniforms(), T, bad, st)
    surf = fu.words(guide[..., 7]) != 0
    assert (mu.status(c)[surf] == mu.UNTRACKED).all() and (st.n()[surf] == 1).all() and (acc == 0).all()
    assert np.array_equal(fu.words(integ), fu.words(col))


def test_the_model_as_a_program_is_clean_under_the_sanitizers():
    """its main runs every out-of-range case on arrays of their exact sizes: a load through a bad index would be reported"""
    r = subprocess.run([mu.sanitized_program()], capture_output=True, text=True)
    assert r.returncode == 0 and "0 bad cases" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_a_change_of_the_counts_drops_the_history():
    two = mu.card_scene([mu.transform((0.0, 0.0, -2.0)), mu.transform((5.0, 0.0, -2.0))], half=0.8)
    three = mu.card_scene([mu.transform((0.0, 0.0, -2.0)), mu.transform((5.0, 0.0, -2.0)), mu.transform((9.0, 0.0, -2.0))], half=0.8)
    more = mu.Scene(two.topo, np.concatenate([two.pos, two.pos[:1]]), two.inst)
    for other in (three, more):
        out, st = run([(two, uniforms(), linear_in_object(0.8))] * 2 + [(other, uniforms(), linear_in_object(0.8))] * 2, T)
        assert [int(o["n"].max()) for o in out] == [1, 2, 1, 2]
        assert st.frames == 2
