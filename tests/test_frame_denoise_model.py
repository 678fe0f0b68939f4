"""The frame denoise rule (include/mi355rt.h, "THE FRAME DENOISE RULE") on its CPU restatement, tests/model/frame_denoise_model.cpp:
the properties the rule promises on synthetic G-buffers, with bounds derived from the tap count, and the quality gate on the
oracle's cornell.  No GPU needed; the GPU kernels are compared with this model word for word in tests/test_gpu_frame_denoise.py.

THE BOUND OF A PASS (sigma_lum <= 0).  A surface pixel's colour is fl(acc / wsum).  The 25 weights h are 9, 3 or 1 times a
power of two and multiples of 2^-8 that sum to at most 1, so wsum is exact.  acc is a chain of at most 25 products h * c, each
rounded once, and 24 additions that are rounded (the first lands on +0): a term passes through at most 25 roundings, the
division adds one.  With every accepted colour in [lo, hi] of one sign the result lies in [lo (1 + u)^-26, hi (1 + u)^26], u =
2^-24; p passes compose to the exponent 26 p."""
import numpy as np
import pytest

import frame_denoise_util as fu

F = np.float32
U = fu.U


def pass_bound(passes, extra=0):
    """relative: (1 + u)^(26 passes + extra) - 1"""
    return (1.0 + U) ** (26 * passes + extra) - 1.0


def test_model_self_check_builds_and_runs_stand_alone(tmp_path):
    """the model has a main of its own: the same file as a program"""
    import os
    import subprocess
    import model_build
    import radiance_util as ru
    exe = str(tmp_path / "frame_denoise_model")
    model_build.build(fu.SRC, exe, [f for f in ru.FLAGS if f != "-fPIC"] + ["-I", os.path.join(fu.REPO, "include")], program=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("step,passes", [(1, 1), (1, 5), (16, 1), (3, 2)])
@pytest.mark.parametrize("shape", [(1, 1), (40, 1), (1, 40), (33, 9), (70, 37)])
def test_constant_image_on_one_surface_stays_constant(shape, step, passes):
    W, H = shape
    fr = fu.Frame(W, H, rgb=(0.3, 1.7, 2.9), weight=3.0)
    rad = fr.radiance()
    out = fu.call(fr, dict(passes=passes, step=step, flags=0, normal_cos=0.9, plane_eps=0.02, sigma_lum=0.0))
    rel = np.abs(out[..., :3].astype(np.float64) / rad.astype(np.float64) - 1.0).max()
    print("max relative deviation", rel, "bound", pass_bound(passes))
    assert rel <= pass_bound(passes)
    assert (out[..., 3] == 1.0).all()
    # with the luminance stop, in the first pass: lum_q - lum_p is exactly 0, rt_exp(-0 / den) is 1, the weights are h again
    # (later passes see the first one's last-place differences and weigh them)
    if passes == 1:
        out_s = fu.call(fr, dict(passes=1, step=step, flags=0, normal_cos=0.9, plane_eps=0.02, sigma_lum=4.0))
        assert not fu.differing(out_s, out).any()


def test_outputs_lie_inside_the_extremes_of_the_accepted_taps():
    rng = np.random.default_rng(5)
    fr = fu.Frame(37, 21, z=2.0)
    fr.accum[..., 0:3] = rng.uniform(0.1, 4.0, (21, 37, 3))
    fr.normal_id[:, 20:, 0:2] = (1.0, 0.0)      # a wall: normal +x
    fr.background(rng.random((21, 37)) < 0.1)
    col, guide, _ = fu.prepare(fr, 0)
    for step in (1, 4, 16):
        for sigma in (0.0, 2.0):
            out, lo, hi, n = fu.one_pass(col, guide, step, sigma_lum=sigma, extremes=True)
            surf = n > 0
            assert surf.any() and (n[surf] >= 1).all() and (n <= 25).all()
            # sigma > 0: the weights are no longer exact, wsum carries its own 25 roundings and each weight two more
            b = pass_bound(1) if sigma == 0.0 else (1.0 + U) ** (2 * 26 + 4) - 1.0
            o = out[..., :3].astype(np.float64)
            assert (o[surf] >= lo[surf] * (1.0 - b)).all() and (o[surf] <= hi[surf] * (1.0 + b)).all(), (step, sigma)
            assert (out[..., 3][surf] >= 0).all()


def test_background_passes_through_bit_for_bit_and_never_leaks():
    rng = np.random.default_rng(6)
    fr = fu.Frame(40, 24, rgb=1.0, weight=2.0)
    bg = rng.random((24, 40)) < 0.3
    fr.background(bg)
    fr.accum[bg, 0:3] = rng.uniform(1e5, 1e6, (int(bg.sum()), 3))
    w = fr.accum.view(np.uint32)
    ys, xs = np.nonzero(bg)
    w[ys[0], xs[0], 0] = 0x7fc00123          # a NaN with a payload in a background pixel
    rad = fr.radiance()
    for flags in (0, fu.DEMODULATE):
        out = fu.call(fr, dict(passes=5, step=1, flags=flags, normal_cos=0.9, plane_eps=0.02, sigma_lum=0.0))
        keep = fu.words(out[..., :3])[bg] == fu.words(rad)[bg]
        keep[0, 0] = bool(np.isnan(out[..., 0][bg][0]))   # the NaN stays a NaN (rad * 1 may quieten it, never lose it)
        assert keep.all()
        # the surface is the constant 0.5: radiance / albedo and back adds three roundings
        assert np.abs(out[..., :3][~bg].astype(np.float64) / 0.5 - 1.0).max() <= pass_bound(5, 3)


def test_coplanar_normals_apart_by_more_than_plane_eps_do_not_mix():
    fr = fu.Frame(40, 12, z=2.0)
    fr.depth[:, 20:] = fu.depth_of(2.5)
    fr.accum[:, :20, 0:3], fr.accum[:, 20:, 0:3] = 1.0, 3.0
    kw = dict(passes=5, step=1, flags=0, normal_cos=0.9, sigma_lum=0.0)
    out = fu.call(fr, dict(kw, plane_eps=0.1))
    assert np.abs(out[:, :20, :3] / 1.0 - 1.0).max() <= pass_bound(5) and np.abs(out[:, 20:, :3] / 3.0 - 1.0).max() <= pass_bound(5)
    mixed = fu.call(fr, dict(kw, plane_eps=1.0))   # ... and with a plane stop wider than the gap they do
    assert mixed[:, 19, 0] .min() > 1.1 and mixed[:, 20, 0].max() < 2.9


def test_instances_of_one_plane_mix_only_without_same_instance():
    fr = fu.Frame(40, 12, inst=3)
    fr.normal_id[:, 20:, 3] = np.full((12, 20), 4, np.uint32).view(F)
    fr.accum[:, :20, 0:3], fr.accum[:, 20:, 0:3] = 1.0, 3.0
    kw = dict(passes=3, step=1, normal_cos=0.9, plane_eps=0.02, sigma_lum=0.0)
    same = fu.call(fr, dict(kw, flags=fu.SAME_INSTANCE))
    assert np.abs(same[:, :20, :3] / 1.0 - 1.0).max() <= pass_bound(3) and np.abs(same[:, 20:, :3] / 3.0 - 1.0).max() <= pass_bound(3)
    free = fu.call(fr, dict(kw, flags=0))
    assert free[:, 19, 0].min() > 1.1 and free[:, 20, 0].max() < 2.9


@pytest.mark.parametrize("step", [1, 2, 4, 8, 16])
def test_sigma_lum_not_above_zero_is_the_h_only_filter(step):
    rng = np.random.default_rng(7)
    fr = fu.Frame(45, 38)
    fr.accum[..., 0:3] = rng.uniform(0.0, 4.0, (38, 45, 3))
    col, guide, _ = fu.prepare(fr, 0)
    want = fu.numpy_pass(col, lambda dx, dy, inside: inside, step)      # one plane: every tap inside the image is accepted
    for sigma in (0.0, -0.0, -1.0, float("nan"), float("-inf")):
        assert not fu.differing(fu.one_pass(col, guide, step, sigma_lum=sigma), want).any(), sigma
    assert fu.differing(fu.one_pass(col, guide, step, sigma_lum=1.0), want).any()


def test_a_nan_guide_or_colour_fails_its_comparison_and_stays_confined():
    fr = fu.Frame(15, 11)
    fr.accum[..., 0:3] = np.arange(15 * 11, dtype=F).reshape(11, 15, 1) + 1.0
    col, guide, _ = fu.prepare(fr, 0)
    g = guide.copy()
    g[5, 7, 4] = np.nan                      # a NaN normal: the pixel accepts only its centre, and no neighbour accepts it
    out, _, _, n = fu.one_pass(col, g, 1, extremes=True)
    assert n[5, 7] == 1 and fu.words(out[5, 7, :3]).tolist() == fu.words(col[5, 7, :3]).tolist()
    clean_n = fu.one_pass(col, guide, 1, extremes=True)[3]
    near = np.zeros((11, 15), bool)
    near[3:8, 5:10] = True
    near[5, 7] = False
    assert (n[near] == clean_n[near] - 1).all() and (n[~near & ~np.isnan(g[..., 4])] == clean_n[~near & ~np.isnan(g[..., 4])]).all()
    assert not np.isnan(out).any()
    g = guide.copy()
    g[5, 7, 0] = np.nan                      # a NaN position fails the plane comparison in the same way
    assert (fu.one_pass(col, g, 1, extremes=True)[3] == n).all()
    c = col.copy()
    c[5, 7, 1] = np.nan                      # a NaN colour reaches exactly the pixels that accept it, in that channel
    out = fu.one_pass(c, guide, 1)
    got = np.isnan(out)
    want = np.zeros_like(got)
    want[3:8, 5:10, 1] = True
    assert (got == want).all()
    out = fu.one_pass(c, guide, 1, sigma_lum=4.0)   # with the luminance stop the weight is a NaN: every channel of those pixels
    want[3:8, 5:10, :] = True
    assert (np.isnan(out) == want).all()


def test_a_call_is_the_composition_of_its_passes():
    c = _cornell_frame()
    for d in (dict(fu.CORNELL, passes=3), dict(fu.CORNELL, passes=2, step=4, flags=fu.SAME_INSTANCE, sigma_lum=0.0)):
        col, guide, mod = fu.prepare(c, d["flags"])
        for p in range(d["passes"]):
            col = fu.one_pass(col, guide, d["step"] << p, flags=d["flags"], normal_cos=d["normal_cos"], plane_eps=d["plane_eps"],
                              sigma_lum=d["sigma_lum"])
        assert not fu.differing(fu.call(c, d), fu.finish(col, mod)).any()
    # {1, 3} is {1, 1}, {2, 1} and {4, 1} on each other's colour images
    a = fu.call(c, dict(fu.CORNELL, passes=3, flags=0))
    col, guide, mod = fu.prepare(c, 0)
    kw = {k: fu.CORNELL[k] for k in ("normal_cos", "plane_eps", "sigma_lum")}
    for s in (1, 2, 4):
        col = fu.one_pass(col, guide, s, **kw)
    assert not fu.differing(a, fu.finish(col, mod)).any()


_frames = {}


def _cornell_frame():
    """a small frame with real structure and no renderer: three surfaces, two instances, a background band, random colours"""
    if "f" not in _frames:
        rng = np.random.default_rng(11)
        fr = fu.Frame(50, 30, jitter=(0.003, -0.002))
        fr.accum[..., 0:3] = rng.uniform(0.0, 3.0, (30, 50, 3))
        fr.accum[..., 3] = 2.0
        fr.normal_id[:, 30:, 0:2] = (0.6, 0.2)
        fr.depth[:, 30:] = fu.depth_of(np.linspace(2.0, 3.0, 20, dtype=F))[None, :]
        fr.normal_id[15:, :, 3] = np.full((15, 50), 1, np.uint32).view(F)
        fr.albedo = (rng.integers(0, 256, (30, 50, 3), dtype=np.uint32) << np.array([0, 8, 16], np.uint32)).sum(axis=2).astype(np.uint32) | 0xff000000
        fr.background(np.arange(30)[:, None] + np.arange(50)[None, :] > 70)
        _frames["f"] = fr
    return _frames["f"]


def test_demodulate_then_remodulate_returns_a_flat_irradiance_image():
    """radiance = E * albedo with E flat: q = fl(fl(E m) / m) is E to two roundings, the passes keep a value within their inputs'
    extremes to 26 roundings each, the remodulation adds one, and the radiance the result is compared with carries one itself:
    (1 + u)^(26 p + 4) - 1."""
    rng = np.random.default_rng(8)
    W, H, E = 41, 27, F(1.75)
    fr = fu.Frame(W, H)
    bytes_ = rng.integers(1, 256, (H, W, 3), dtype=np.uint32)       # an albedo byte of 0 is floored at 1 / 255: no way back
    fr.albedo = (bytes_[..., 0] | (bytes_[..., 1] << 8) | (bytes_[..., 2] << 16) | 0xff000000).astype(np.uint32)
    m = (bytes_.astype(np.float64) / 255.0).astype(F)
    fr.accum[..., 0:3] = E * m
    for passes in (1, 4):
        out = fu.call(fr, dict(passes=passes, step=1, flags=fu.DEMODULATE, normal_cos=0.9, plane_eps=0.02, sigma_lum=0.0))
        rel = np.abs(out[..., :3].astype(np.float64) / fr.accum[..., 0:3].astype(np.float64) - 1.0).max()
        print("passes", passes, "max relative deviation", rel, "bound", pass_bound(passes, 4))
        assert rel <= pass_bound(passes, 4)
    # without the flag the texture is blurred away: the same image moves by far more than the bound
    out = fu.call(fr, dict(passes=4, step=1, flags=0, normal_cos=0.9, plane_eps=0.02, sigma_lum=0.0))
    assert np.abs(out[..., :3] / fr.accum[..., 0:3] - 1.0).max() > 0.1


# measured on this test's own inputs (the oracle's cornell, 64 x 64, depth 4, 4 spp against 512 spp, CORNELL = {step 1, passes
# 4, DEMODULATE, normal_cos 0.9, plane_eps 0.02, sigma_lum 4}): unfiltered rgb RMSE 0.1168, filtered 0.0784, ratio 0.671
MEASURED_RATIO = 0.671


def test_quality_on_the_oracles_cornell(W, oracle_lib):
    c = fu.cornell_oracle(W, oracle_lib)
    fr = fu.frame_of(c["noisy"], c["gbuffer"], c["uniforms"])
    clean = c["clean"][..., :3] / c["clean"][..., 3:4]
    before = fu.rmse(fr.radiance(), clean)
    out = fu.call(fr, fu.CORNELL)
    after = fu.rmse(out[..., :3], clean)
    print("rgb RMSE against 512 spp: unfiltered %.5f filtered %.5f ratio %.4f" % (before, after, after / before))
    assert after < before
    assert after / before < (1.0 + MEASURED_RATIO) / 2.0
    assert (out[..., 3] == 1.0).all()
