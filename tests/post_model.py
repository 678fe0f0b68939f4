"""An independent statement of the post pass and the images it is tested on.

`model()` is PostProcess.wgsl:36-176 written down from the shader in vectorised float64 numpy (numpy exp, **, sqrt,
minimum / maximum).  It shares no code with oracle/rt_oracle.cpp, include/mi355rt_math.h or the HIP kernel, so a
misreading of the shader that kernel and oracle have in common does not pass it.  `check()` holds the conditions under
which an f32 implementation must agree with it (derivation in its docstring); tests/test_post_model.py applies them to
the CPU oracle, tests/test_gpu_post.py to k_postprocess.
"""
import numpy as np

IMAGES = ("lognormal", "fireflies_holes", "steps", "noisy_steps", "checker", "ramp", "seams")
# exactly flat regions: beyond 16 frames the history window there is 60 standard deviations of f32 rounding noise
FLAT_IMAGES = ("steps", "seams")
SHAPES = [(23, 17), (16, 16), (33, 2), (3, 40), (47, 31), (1, 1)]       # (w, h)
FRAME_COUNTS = [1, 2, 5, 16, 17, 64]


# ------------------------------------------------------------------------------------------------------------ the model
def average_jitter(uniforms):
    """scene.average_jitter of the renderer's 256-byte uniform block (bytes 232..239, two f32)."""
    return np.frombuffer(np.ascontiguousarray(uniforms, dtype=np.uint8).tobytes(), dtype=np.float32, count=2, offset=232)


def widen_history(hist_u16):
    """rgba16f bits (h, w, 4) uint16 -> float64"""
    return np.ascontiguousarray(hist_u16, dtype=np.uint16).view(np.float16).astype(np.float64)


def _aces(c):   # :36-39
    return np.minimum(np.maximum((c * (2.51 * c + 0.03)) / (c * (2.43 * c + 0.59) + 0.14), 0.0), 1.0)


def model(accum, history, frame_count, avg_jitter):
    """accum (h, w, 4) f32; history (h, w, 3 or 4) float (the texture the pass reads); frame_count >= 1;
    avg_jitter 2 floats.  Returns a dict of float64 arrays (h, w, 3): `out255` (the 0..255 value before rounding), `hdr`
    (what is written to the history), `mean`, `stddev`, `lo`, `hi` (the clamp window) and bool `active` (history outside
    the window, per channel)."""
    if frame_count < 1:
        raise ValueError("the model is for finite jitter and alpha: frame_count >= 1")
    acc = np.asarray(accum, dtype=np.float32).astype(np.float64)
    h, w = acc.shape[:2]
    with np.errstate(divide="ignore", invalid="ignore"):
        rad = np.where(acc[..., 3:4] <= 0.0, 0.0, acc[..., :3] / acc[..., 3:4])     # get_radiance, :41-47

    def get_radiance(X, Y):          # integer coordinate arrays of any shape, clamped one by one
        return rad[np.clip(Y, 0, h - 1), np.clip(X, 0, w - 1)]

    offsets = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]

    def clean(X, Y):                 # :49-68
        center = get_radiance(X, Y)
        max_nb = np.full(center.shape, -1e6)
        for dx, dy in offsets:
            if dx == 0 and dy == 0:
                continue
            max_nb = np.maximum(max_nb, get_radiance(X + dx, Y + dy))
        return np.minimum(np.maximum(center, 0.0), max_nb * 3.0 + 0.1)

    def nearest(X, Y):               # :71-97
        if frame_count > 16:
            return clean(X, Y)
        u = (X + 0.5) / float(w) - float(avg_jitter[0])
        v = (Y + 0.5) / float(h) - float(avg_jitter[1])
        fx, fy = u * w - 0.5, v * h - 0.5
        ix, iy = np.floor(fx), np.floor(fy)
        tx, ty = (fx - ix)[..., None], (fy - iy)[..., None]
        ix, iy = ix.astype(np.int64), iy.astype(np.int64)
        c00, c10 = clean(ix, iy), clean(ix + 1, iy)
        c01, c11 = clean(ix, iy + 1), clean(ix + 1, iy + 1)
        top = c00 * (1.0 - tx) + c10 * tx
        bot = c01 * (1.0 - tx) + c11 * tx
        return top * (1.0 - ty) + bot * ty

    # main() asks for get_radiance_nearest at id + (-1..1): coordinates -1 .. w and -1 .. h, NOT clamped at this level
    Yg, Xg = np.meshgrid(np.arange(-1, h + 1), np.arange(-1, w + 1), indexing="ij")
    near = nearest(Xg, Yg)           # (h + 2, w + 2, 3)

    def at(dx, dy):
        return near[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    center = at(0, 0)
    filtered = np.zeros_like(center)
    total = np.zeros(center.shape[:2] + (1,))
    m1 = np.zeros_like(center)
    m2 = np.zeros_like(center)
    for dx, dy in offsets:           # :113-148
        nc = at(dx, dy)
        w_s = np.exp(-float(dx * dx + dy * dy) / (2.0 * 0.5 * 0.5))
        cd = nc - center
        w_r = np.exp(-np.sum(cd * cd, axis=-1, keepdims=True) / (2.0 * 0.1 * 1.0 * 1.0))
        wgt = w_s * w_r
        filtered += nc * wgt
        total += wgt
        m1 += nc
        m2 += nc * nc
    denoised = filtered / np.maximum(total, 1e-4)
    mean = m1 / 9.0
    stddev = np.sqrt(np.maximum(m2 / 9.0 - mean * mean, 0.0))
    k = 60.0 if frame_count > 16 else 1.0
    lo, hi = mean - stddev * k, mean + stddev * k
    hist = np.asarray(history, dtype=np.float64)[..., :3]
    clamped = np.minimum(np.maximum(hist, lo), hi)
    alpha = 1.0 / float(frame_count)
    if frame_count == 1:
        alpha = 0.1
    alpha = max(alpha, 0.0001)
    hdr = clamped * (1.0 - alpha) + denoised * alpha
    sharpened = _aces(hdr) + _aces(center - denoised) * 0.3
    ldr = np.minimum(np.maximum(sharpened, 0.0), 1.0) ** (1.0 / 2.2)
    return {"out255": ldr * 255.0, "hdr": hdr, "mean": mean, "stddev": stddev, "lo": lo, "hi": hi,
            "active": (hist < lo) | (hist > hi)}


# ------------------------------------------------------------------------------------------------------- the conditions
FLAGGED_CAP = 0.02      # share of a case's pixels that may be left out beyond 16 frames


def f16_ulp(v):
    """Spacing of binary16 at |v| (2^-24 in the subnormal range)."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (np.maximum(e, -14.0) - 10.0)


def flagged(m):
    """Pixels where, in some channel, the history clamp is active AND the neighbourhood variance is below 1e-4 x mean^2.
    The f32 `m2 / 9 - mean^2` there is a difference of two numbers that agree to four digits or more: what is left of it is
    rounding noise of the order of 1e-7 x mean^2, its root a few 1e-4 x mean, and the clamped history sits on that window
    edge.  Everywhere else the result is a well-conditioned function of the inputs."""
    low_var = m["stddev"] ** 2 < 1e-4 * m["mean"] ** 2
    return (m["active"] & low_var).any(axis=-1)


def compared_pixels(m, frame_count):
    """(mask of the pixels compared with the strict bounds, mask of those compared with the flagged bounds).  Asserts the
    cap on what is left out from the model alone, so a case that needs the exclusion to pass fails here."""
    fl = flagged(m)
    if frame_count <= 16:
        return ~fl, fl
    share = fl.mean()
    assert share <= FLAGGED_CAP, "%.1f %% of the pixels are ill conditioned beyond 16 frames (cap %.0f %%): not a case " \
                                 "for the model" % (100 * share, 100 * FLAGGED_CAP)
    return ~fl, np.zeros_like(fl)


def check(m, rgba8, hist_u16, frame_count, what, stats=None):
    """An f32 implementation's RGBA8 output and rgba16f history against the model `m`.

    Well-conditioned pixels: every byte within 1 code value of floor(model + 0.5), at most max(1, 1 %) of the case's
    components different at all; history within 1 f16 ulp of the model value (half an ulp of rounding plus one boundary
    flip).  Flagged pixels up to 16 frames (window = 1 stddev): 1 code value, 2 f16 ulp.  Flagged pixels beyond 16 frames
    (window = 60 stddev of noise) are left out, capped by compared_pixels().  Alpha byte 255 and history w == 1.0
    everywhere.  `stats` (a dict) collects the worst figures seen."""
    rgba8 = np.asarray(rgba8)
    got = rgba8[..., :3].astype(np.float64)
    hist = widen_history(hist_u16)
    good, fl = compared_pixels(m, frame_count)
    want = np.floor(m["out255"] + 0.5)
    code = np.abs(got - want)
    ulps = np.abs(hist[..., :3] - m["hdr"]) / f16_ulp(m["hdr"])
    n_good = int(good.sum()) * 3
    differing = int((code[good] != 0).sum())
    if stats is not None:
        def worst(key, v):
            stats[key] = max(stats.get(key, 0.0), float(v))
        if n_good:
            worst("good_codes", code[good].max())
            worst("good_differing_share", differing / n_good)
            worst("good_distance", np.abs(got - m["out255"])[good].max())
            worst("good_ulp", ulps[good].max())
        if fl.any():
            worst("flagged_codes", code[fl].max())
            worst("flagged_ulp", ulps[fl].max())
        worst("flagged_share_%s" % ("le16" if frame_count <= 16 else "gt16"), flagged(m).mean())
    assert (rgba8[..., 3] == 255).all(), what + ": alpha byte"
    assert (np.asarray(hist_u16)[..., 3] == 0x3c00).all(), what + ": history w"
    if n_good:
        assert code[good].max() <= 1.0, "%s: RGBA8 %g code values from the model at %s" % (
            what, code[good].max(), np.argwhere((code > 1.0) & good[..., None])[0])
        assert differing <= max(1, 0.01 * n_good), "%s: %d of %d components differ from the model" % (what, differing, n_good)
        assert ulps[good].max() <= 1.0, "%s: history %.3f f16 ulp from the model at %s" % (
            what, ulps[good].max(), np.argwhere((ulps > 1.0) & good[..., None])[0])
    if fl.any():
        assert code[fl].max() <= 1.0, "%s: flagged pixel %g code values from the model" % (what, code[fl].max())
        assert ulps[fl].max() <= 2.0, "%s: flagged pixel %.3f f16 ulp from the model" % (what, ulps[fl].max())


def runs_against_model(image, w, h, frame_count):
    """Exactly flat images and the one-pixel shape are all flagged beyond 16 frames: not compared with the model there."""
    return frame_count <= 16 or not (image in FLAT_IMAGES or w * h == 1)


# ------------------------------------------------------------------------------------------------------------ the images
SEAM_COORDS = (15, 16, 17, 31, 32)
_TINT = np.array([1.0, 0.8, 0.6])


def _rng(name, w, h):
    return np.random.default_rng([IMAGES.index(name) if name in IMAGES else 99, w, h])


def radiance(name, w, h):
    """(rgb (h, w, 3) float64 radiance, weight factor (h, w): 1, 0 or -1 times the frame count)"""
    rng = _rng(name, w, h)
    wf = np.ones((h, w))
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if name in ("lognormal", "fireflies_holes"):
        rgb = np.exp(rng.normal(-1.0, 1.0, (h, w, 3)))
        if name == "fireflies_holes":
            for i in range(12):
                x, y = int(rng.integers(w)), int(rng.integers(h))
                rgb[y, x] = rng.uniform(20.0, 400.0, 3)
                wf[y, x] = (1.0, 1.0, 0.0, -1.0)[i % 4]
    elif name in ("steps", "noisy_steps"):
        level = np.where(yy < h // 2, np.where(xx < w // 2, 0.05, 2.0), np.where(xx < w // 2, 0.6, 9.0))
        rgb = level[..., None] * _TINT
        if name == "noisy_steps":
            rgb = rgb * (1.0 + 0.05 * rng.standard_normal((h, w, 3)))
    elif name == "checker":
        rgb = np.where(((xx + yy) & 1)[..., None] == 0, 0.08, 1.5) * _TINT
    elif name == "ramp":
        # geometric (a ramp in stops), 12 % / 12 % / 10 % per pixel along x / y / the diagonal, starting over every 45 / 40 /
        # 48 pixels.  A ramp that is linear in radiance, or geometric over the whole of a wide image, has a relative
        # gradient of 1-2 % per pixel, a neighbourhood variance of 1e-4 .. 1e-3 x mean^2: above the flagging threshold,
        # and yet beyond 16 frames the window edge mean - 60 stddev carries 30 x (rounding error of the f32 variance,
        # ~3e-7 mean^2) / (stddev x mean), more than one f16 ulp (2^-11 .. 2^-10 relative) once stddev / mean is below
        # ~0.02.  Measured on such ramps against the CPU oracle: 2.13 f16 ulp (linear, 33 x 2, 17 frames, last column)
        # and 9.87 f16 ulp (2 % per pixel, 257 x 3, 64 frames).  Here stddev / mean is 0.04 or more everywhere.
        rgb = np.stack([0.02 * 1.12 ** (xx % 45), 0.02 * 1.12 ** (yy % 40), 0.05 * 1.10 ** ((xx + yy) % 48)], axis=-1)
    elif name == "seams":
        # a step edge on every tile seam of the LDS-tiled kernel and single bright pixels on and around the seams
        cells = np.searchsorted(np.array([16, 32]), xx, side="right") + np.searchsorted(np.array([16, 32]), yy, side="right")
        rgb = np.array([0.1, 1.2, 0.4, 3.0, 0.25])[cells][..., None] * _TINT
        for x in SEAM_COORDS + (w - 1,):
            for y in SEAM_COORDS + (h - 1,):
                if x < w and y < h and (x + y) % 2 == 0:
                    rgb[y, x] = (6.0, 5.0, 7.0)
        for x in SEAM_COORDS:
            if x < w:
                rgb[h - 1, x] = (4.0, 0.0, 2.0)
        for y in SEAM_COORDS:
            if y < h:
                rgb[y, w - 1] = (0.0, 4.0, 2.0)
    else:
        raise KeyError(name)
    return rgb, wf


def accum(name, w, h, frame_count):
    """The accumulation buffer after `frame_count` frames of image `name`: radiance x n with weight n (0 frames: as 1)."""
    rgb, wf = radiance(name, w, h)
    n = float(max(frame_count, 1))
    acc = np.empty((h, w, 4), dtype=np.float32)
    acc[..., :3] = (rgb * n).astype(np.float32)
    acc[..., 3] = (wf * n).astype(np.float32)
    return acc


def specials(w, h, frame_count):
    """A lognormal base with one pixel each of the values a path tracer never produces but the C ABI accepts, placed at
    image corners, tile corners (15/16, 31/32), on the last row / column and in a tile interior.  Values are the stored
    accumulator values (not scaled by the frame count), so the f16 boundaries are hit as written for weight 1."""
    acc = accum("lognormal", w, h, frame_count)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    fmax = np.finfo(np.float32).max
    px = [(nan, nan, nan, 1.0), (inf, inf, inf, 1.0), (-inf, -inf, -inf, 1.0), (nan, 0.5, inf, 1.0),
          (0.5, 0.5, 0.5, nan), (0.5, 0.5, 0.5, -0.0), (0.5, 0.5, 0.5, -1.0), (0.5, 0.5, 0.5, inf),
          (1e-40, 1e-40, 1e-40, 1.0), (0.5, 0.25, 1.0, 1e-40), (1e-40, 1e-40, 1e-40, 1e-40),
          (fmax, fmax, fmax, 1.0), (fmax, 1.0, 0.0, fmax), (-fmax, -1.0, -0.0, 1.0)]
    for v in (65503.0, 65504.0, 65519.0, 65520.0, 65536.0, 7e4, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25):
        px.append((v, v, v, 1.0))          # rgb at the boundary
        px.append((1.0, 0.5, 2.0, v))      # weight at the boundary
    sites = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
    sites += [(x, y) for x in (15, 16, 31, 32) for y in (15, 16, 31, 32)]
    sites += [(x, h - 1) for x in (3, 8, 15, 16, 24)] + [(w - 1, y) for y in (3, 8, 15, 16, 24)]
    sites += [(x, y) for y in (5, 8, 11, 21, 25) for x in (4, 7, 10, 20, 24, 27)]
    sites = list(dict.fromkeys((x, y) for x, y in sites if 0 <= x < w and 0 <= y < h))
    acc = acc.copy()
    with np.errstate(over="ignore"):
        for i, (x, y) in enumerate(sites):        # small images: as many of the values as there are sites
            acc[y, x] = np.array(px[i % len(px)], dtype=np.float32)
        for i in range(len(sites), len(px)):      # large images: the rest in tile interiors, spread by a fixed stride
            j = (i * 7919) % (w * h)
            acc[j // w, j % w] = np.array(px[i], dtype=np.float32)
    return acc
