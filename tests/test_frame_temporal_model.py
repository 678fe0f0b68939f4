"""The frame temporal rule (include/mi355rt.h, "THE FRAME TEMPORAL RULE") on its CPU restatement,
tests/model/frame_temporal_model.cpp: the properties the rule promises on synthetic G-buffers (frame_denoise_util.Frame scenes
seen through frame_temporal_util.camera), with bounds derived from operation counts, and the quality gate on the oracle's
cornell.  No GPU needed; the GPU kernel is compared with this model word for word in tests/test_gpu_frame_temporal.py.

THE BOUND OF A FRAME on a constant image.  hq = fl(acc / wsum): a term w * h is rounded once and passes through at most three
additions, wsum through at most three, the division adds one: 8 roundings.  The blend hq + a * (c - hq) adds four (the
difference, a, the product, the sum).  A constant therefore stays within (1 + u)^12 per frame of history, u = 2^-24."""
import os
import subprocess

import numpy as np
import pytest

import frame_denoise_util as fu
import frame_temporal_util as tu
import model_build
import radiance_util as ru

F = np.float32
U = tu.U
T = dict(flags=0, max_history=32, var_history=4, normal_cos=0.9, plane_eps=0.01)
ROUNDINGS_PER_FRAME = 12


def _surface(guide):
    return fu.words(guide[..., 7]) != 0


def _same(a, b):
    return not fu.differing(a, b).any()


def _program(tmp_path, name, extra):
    exe = str(tmp_path / name)
    flags = [f for f in ru.FLAGS if f != "-fPIC"] + extra + ["-I", os.path.join(tu.REPO, "include")]
    model_build.build(tu.SRC, exe, flags, program=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_model_self_check_builds_and_runs_stand_alone(tmp_path):
    """the model has a main of its own: the same file as a program"""
    r = _program(tmp_path, "frame_temporal_model", [])
    assert r.returncode == 0, r.stdout + r.stderr


def test_model_self_check_is_clean_under_the_sanitizers(tmp_path):
    """... and as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer: nothing is loaded into Python"""
    r = _program(tmp_path, "frame_temporal_model_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def _random_frame(W, H, seed, **kw):
    rng = np.random.default_rng(seed)
    fr = tu.wall(W, H, **kw)
    fr.accum[..., 0:3] = rng.uniform(0.1, 3.0, (H, W, 3))
    fr.background(rng.random((H, W)) < 0.15)
    return fr


@pytest.mark.parametrize("shape", [(1, 1), (40, 1), (1, 40), (33, 9)])
def test_first_frame_reset_and_max_history_1_give_prepares_texels(shape):
    W, H = shape
    fr = _random_frame(W, H, 3)
    col, guide, _ = fu.prepare(fr, 0)
    surf = _surface(guide)

    def first(integ, st):
        assert fu.words(integ).tolist() == fu.words(col).tolist()
        assert (st.n()[surf] == 1).all() and (st.n()[~surf] == 0).all()
        assert fu.words(st.hist[..., :3]).tolist() == fu.words(col[..., :3]).tolist()
        l = fu.words(st.mom[..., 0])
        lum = ((F(0.2126) * col[..., 0] + F(0.7152) * col[..., 1]) + F(0.0722) * col[..., 2]).astype(F)
        assert (l[surf] == fu.words(lum)[surf]).all() and (fu.words(st.mom[..., 1])[surf] == fu.words(lum * lum)[surf]).all()
        assert (st.mom[~surf] == 0).all()

    st = tu.History()
    first(tu.stage(col, guide, fr.uniforms, T, st)[0], st)              # the first frame
    tu.stage(col, guide, fr.uniforms, T, st)
    assert H * W == 1 and not surf.any() or (st.n()[surf] == 2).all()
    st = tu.History()                                                    # a frame after a reset
    first(tu.stage(col, guide, fr.uniforms, T, st)[0], st)
    for _ in range(3):                                                   # max_history = 1 keeps none, frame after frame
        integ, acc = tu.stage(col, guide, fr.uniforms, dict(T, max_history=1), st)
        first(integ, st)
        assert (acc == 0).all()


def test_static_camera_history_grows_to_max_history_and_a_constant_stays_constant():
    W, H, K, M = 37, 21, 7, 4
    fr = tu.wall(W, H, rgb=(0.3, 1.7, 2.9), jitter=(0.004, -0.003))
    fr.background(np.arange(H)[:, None] + np.arange(W)[None, :] > 45)
    col, guide, _ = fu.prepare(fr, 0)
    surf = _surface(guide)
    st = tu.History()
    for k in range(1, K + 1):
        integ, _ = tu.stage(col, guide, fr.uniforms, dict(T, max_history=M), st)
        assert (st.n()[surf] == min(k, M)).all() and (st.n()[~surf] == 0).all() and st.n().max() <= M
        rel = np.abs(integ[..., :3][surf].astype(np.float64) / col[..., :3][surf].astype(np.float64) - 1.0).max()
        bound = (1.0 + U) ** (ROUNDINGS_PER_FRAME * (k - 1)) - 1.0
        print("frame", k, "max relative deviation", rel, "bound", bound)
        assert rel <= bound
        assert fu.words(integ[~surf]).tolist() == fu.words(col[~surf]).tolist()
    assert st.frames == K


def test_reprojection_is_exact_on_a_pattern_linear_in_world_x_and_y():
    """Colour = a + b X + c Y on the plane z = -2; the plane is parallel to the image plane, so pixel -> world is affine and the
    bilinear footprint of the previous colours IS the current colour, up to rounding.  The cameras differ by a translation of
    non-integer pixel fractions, a roll, and both jitters are non-zero: a wrong jitter sign, v flip or axis would move the
    footprint by tenths of a pixel, 1e-2 in colour.
    THE BOUND.  Fewer than 64 roundings on magnitudes of at most 8 (|e| < 4, |nrm| = 4) precede the division by |hor|^2 = 4:
    the plane coordinate is off by at most 128 u of the image, which is 4 world units wide there: 512 u world units.  The two
    stored positions carry three roundings each on magnitudes below 4: 24 u more.  With G the sum of the colour's gradient
    magnitudes per world unit that is 536 u G; the interpolation and the blend add 12 roundings on colours of at most cmax."""
    W, H = 48, 40
    coef = np.array([[1.5, 0.31, -0.22], [2.0, -0.17, 0.4], [0.9, 0.25, 0.12]])
    G, cmax = np.abs(coef[:, 1:]).sum(axis=1).max(), 4.0
    bound = 536 * U * G + 12 * U * cmax

    def frame(**kw):
        fr = tu.wall(W, H, **kw)
        _, guide, _ = fu.prepare(fr, 0)
        P = guide[..., 0:3].astype(np.float64)
        fr.accum[..., 0:3] = (coef[:, 0] + P[..., 0:1] * coef[:, 1] + P[..., 1:2] * coef[:, 2]).astype(F)
        assert 0 < fr.accum[..., 0:3].min() and fr.accum[..., 0:3].max() < cmax
        return fr

    pixel = 4.0 / W
    prev = frame(eye=(0.05, -0.02, 0.0), roll=0.05, jitter=(0.006, -0.004))
    cur = frame(eye=(0.05 + 1.37 * pixel, -0.02 - 0.61 * pixel, 0.0), roll=0.02, jitter=(-0.003, 0.007))
    st = tu.History()
    for fr in (prev, cur):
        col, guide, _ = fu.prepare(fr, 0)
        integ, acc = tu.stage(col, guide, fr.uniforms, T, st)
    full = acc == 4
    assert full.sum() > W * H // 2 and (st.n()[full] == 2).all()
    err = np.abs(integ[..., :3].astype(np.float64) - col[..., :3].astype(np.float64))[full].max()
    print("max colour error", err, "bound", bound, "pixels", int(full.sum()))
    assert err <= bound


def test_disocclusion_restarts_the_history_and_nothing_leaks():
    W, H = 44, 30
    prev = tu.wall(W, H, rgb=1.0, jitter=(0.002, 0.001))
    prev.depth[8:20, 10:30] = fu.depth_of(1.0)          # an occluder at view depth 1
    prev.accum[8:20, 10:30, 0:3] = 1e6
    rng = np.random.default_rng(9)
    cur = tu.wall(W, H, jitter=(-0.004, 0.003))
    cur.accum[..., 0:3] = rng.uniform(0.5, 2.0, (H, W, 3))
    st = tu.History()
    col, guide, _ = fu.prepare(prev, 0)
    tu.stage(col, guide, prev.uniforms, T, st)
    col, guide, _ = fu.prepare(cur, 0)
    fx, fy, _ = tu.footprint(guide, prev.uniforms)
    x0, y0 = np.floor(fx), np.floor(fy)
    onto = (x0 >= 10) & (x0 + 1 < 30) & (y0 >= 8) & (y0 + 1 < 20)      # all four taps are the occluder's
    integ, acc = tu.stage(col, guide, cur.uniforms, T, st)
    assert onto.sum() > 100
    assert (st.n()[onto] == 1).all() and (acc[onto] == 0).all()
    assert fu.words(integ[onto]).tolist() == fu.words(col[onto]).tolist()
    assert integ[..., :3].max() <= col[..., :3].max() and st.hist[..., :3].max() <= col[..., :3].max()
    assert (st.n()[~onto] == 2).sum() > W * H // 2


def test_the_instance_test_applies_only_with_the_flag():
    W, H = 20, 12
    a, b = tu.wall(W, H, inst=3), tu.wall(W, H, inst=4)
    for flags, want in ((tu.SAME_INSTANCE, 1), (0, 2)):
        st = tu.History()
        for fr in (a, b):
            col, guide, _ = fu.prepare(fr, 0)
            tu.stage(col, guide, fr.uniforms, dict(T, flags=flags), st)
        assert (st.n() == want).all(), flags
    st = tu.History()
    for fr in (a, a):
        col, guide, _ = fu.prepare(fr, 0)
        tu.stage(col, guide, fr.uniforms, dict(T, flags=tu.SAME_INSTANCE), st)
    assert (st.n() == 2).all()


def test_the_normal_test_and_a_nan_parameter_reject_every_tap():
    W, H = 20, 12
    fr = tu.wall(W, H)
    col, guide, _ = fu.prepare(fr, 0)
    st = tu.History()
    tu.stage(col, guide, fr.uniforms, T, st)
    st.guide[..., 4:7] = (0.6, 0.0, 0.8)                 # the previous normals: 0.8 against the current ones
    keep = (st.hist.copy(), st.mom.copy(), st.guide.copy(), st.uniforms.copy())
    for t, want in ((dict(T, normal_cos=0.9), 1), (dict(T, normal_cos=0.7), 2), (dict(T, normal_cos=np.nan), 1),
                    (dict(T, normal_cos=0.7, plane_eps=np.nan), 1)):
        st.hist, st.mom, st.guide, st.uniforms = (k.copy() for k in keep)
        tu.stage(col, guide, fr.uniforms, t, st)
        assert (st.n() == want).all(), t


def test_a_point_behind_the_previous_camera_gets_no_history():
    W, H = 20, 12
    fr = tu.wall(W, H)
    col, guide, _ = fu.prepare(fr, 0)
    st = tu.History()
    tu.stage(col, guide, fr.uniforms, T, st)
    st.uniforms = tu.camera(W, H, eye=(0.0, 0.0, -4.0))  # the wall z = -2 is behind this pinhole, mirrored into its image
    fx, fy, s = tu.footprint(guide, st.uniforms)
    assert (s < 0).all() and ((fx > 0) & (fx < W - 1) & (fy > 0) & (fy < H - 1)).all()
    integ, acc = tu.stage(col, guide, fr.uniforms, T, st)
    assert (acc == 0).all() and (st.n() == 1).all() and fu.words(integ).tolist() == fu.words(col).tolist()


def test_a_nan_history_texel_reaches_only_the_footprints_that_hold_it():
    W, H, ny, nx = 30, 22, 9, 13
    pixel = 4.0 / W
    prev = tu.wall(W, H)
    prev.accum[..., 0:3] = np.random.default_rng(4).uniform(0.1, 3.0, (H, W, 3))
    cur =tu.wall(W, H, eye=(0.37 * pixel, 0.41 * pixel * W / H, 0.0))
    cur.accum[..., 0:3] = 1.0
    st = tu.History()
    col, guide, _ = fu.prepare(prev, 0)
    tu.stage(col, guide, prev.uniforms, T, st)
    st.hist[ny, nx, 1] = np.nan
    st.mom[ny, nx, 0] = np.nan
    col, guide, _ = fu.prepare(cur, 0)
    fx, fy, _ = tu.footprint(guide, prev.uniforms)
    x0, y0 = np.floor(fx), np.floor(fy)
    frac = np.minimum(np.minimum(fx - x0, x0 + 1 - fx), np.minimum(fy - y0, y0 + 1 - fy))
    assert frac.min() > 0.05, "every weight is well above 0: the footprints are unambiguous"
    holds = ((x0 == nx) | (x0 + 1 == nx)) & ((y0 == ny) | (y0 + 1 == ny)) & _surface(guide)
    assert holds.sum() == 4
    integ, acc = tu.stage(col, guide, cur.uniforms, dict(T, var_history=2), st)
    assert (np.isnan(integ[..., 1]) == holds).all() and not np.isnan(integ[..., 0]).any() and not np.isnan(integ[..., 2]).any()
    assert (np.isnan(st.hist[..., 1]) == holds).all() and (np.isnan(st.mom[..., 0]) == holds).all()
    assert not np.isnan(st.mom[..., 1]).any() and not np.isnan(st.n()).any()


def test_variance_switches_from_spatial_to_temporal_exactly_at_var_history():
    W, H, V = 26, 14, 3
    st = tu.History()
    for k in range(1, 6):
        fr = tu.wall(W, H)
        fr.accum[..., 0:3] = np.random.default_rng(20 + k).uniform(0.1, 3.0, (H, W, 3))
        col, guide, _ = fu.prepare(fr, 0)
        integ, _ = tu.stage(col, guide, fr.uniforms, dict(T, var_history=V), st)
        assert (st.n() == k).all()
        m1, m2 = st.mom[..., 0], st.mom[..., 1]
        temporal = np.maximum((m2 - (m1 * m1).astype(F)).astype(F), F(0))
        want = temporal if k >= V else col[..., 3]
        assert fu.words(integ[..., 3]).tolist() == fu.words(want).tolist(), k
        assert k < V or (fu.words(integ[..., 3]) != fu.words(col[..., 3])).any()


def _structured(k, eye):
    """three surfaces, two instances, a background band, random colours: frame k of a sequence seen from `eye`"""
    rng = np.random.default_rng(30 + k)
    W, H = 50, 30
    fr = tu.wall(W, H, eye=eye, jitter=(0.003 - 0.001 * k, -0.002 + 0.0015 * k))
    fr.accum[..., 0:3] = rng.uniform(0.0, 3.0, (H, W, 3))
    fr.accum[..., 3] = 2.0
    fr.normal_id[:, 40:, 0:2] = (0.6, 0.2)
    fr.normal_id[15:, :, 3] = np.full((15, W), 1, np.uint32).view(F)
    fr.albedo = (np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint32) << np.array([0, 8, 16], np.uint32)).sum(
        axis=2).astype(np.uint32) | 0xff000000
    fr.background(np.arange(H)[:, None] + np.arange(W)[None, :] > 70)
    return fr


def test_a_call_is_the_composition_of_its_stages():
    d = dict(fu.CORNELL, passes=3)
    st, manual = tu.History(), tu.History()
    for k in range(3):
        fr = _structured(k, (0.011 * k, -0.007 * k, 0.0))
        out, integ, _ = tu.call(fr, d, T, st)
        col, guide, mod = fu.prepare(fr, d["flags"])
        want, _ = tu.stage(col, guide, fr.uniforms, T, manual)
        assert _same(integ, want)
        for p in range(d["passes"]):
            want = fu.one_pass(want, guide, d["step"] << p, flags=d["flags"], normal_cos=d["normal_cos"], plane_eps=d["plane_eps"],
                               sigma_lum=d["sigma_lum"])
        assert _same(out, fu.finish(want, mod))
        # with no history to blend the call is the plain call of the frame-denoise model, word for word
        assert _same(tu.call(fr, d, dict(T, max_history=1), tu.History())[0], fu.call(fr, d))
        if k == 0:
            assert _same(out, fu.call(fr, d))
    assert (st.n() >= 2).any() and st.frames == 3
    # a change of the DEMODULATE bit drops the history
    out, _, acc = tu.call(_structured(3, (0.03, -0.02, 0.0)), dict(d, flags=0), T, st)
    assert (acc == 0).all() and st.n().max() == 1


# measured on this test's own inputs with the model (the oracle's cornell, 64 x 64, depth 4, eight frames of 1 spp with the
# accumulation reset every frame and the camera moved by frame_temporal_util.GATE_STEP = (0.01, 0.005, 0) per frame, against 512
# spp at the last camera; frame_denoise_util.CORNELL behind frame_temporal_util.CORNELL): rgb RMSE of the last frame, spatial
# filter alone r_s = 0.07061, with the temporal stage ahead of it r_t = 0.06959, ratio 0.9856
MEASURED_R_T = 0.06959


def test_quality_on_the_oracles_cornell(W, oracle_lib):
    seq = tu.cornell_sequence(W, oracle_lib)
    clean = seq["clean"]
    r_s = fu.rmse(fu.call(seq["frames"][-1], fu.CORNELL)[..., :3], clean)
    st = tu.History()
    for fr in seq["frames"]:
        out, integ, _ = tu.call(fr, fu.CORNELL, tu.CORNELL, st)
    r_t = fu.rmse(out[..., :3], clean)
    print("rgb RMSE against 512 spp: spatial alone %.5f, temporal ahead of it %.5f, ratio %.4f" % (r_s, r_t, r_t / r_s))
    assert r_t < r_s
    assert r_t < (r_s + MEASURED_R_T) / 2.0
    assert (out[..., 3] == 1.0).all()
