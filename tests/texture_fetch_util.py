"""Shared pieces of the known-answer tests of the texture fetch (sample_tex: csrc/k_common.hip.h, restated in
oracle/rt_oracle.cpp): structured textures made by formula, the sample points at which a fetch goes wrong, one-instance scenes
of one tiny triangle per sample point whose radiance query at max_depth = 1 returns the fetched texel, and a float64 numpy
statement of WebGPU's textureSampleLevel written from the specification (level 0, 2d-array, repeat addressing, linear filter,
rgba8unorm, no sRGB), with the deliberate convention errors the tests must be able to tell from it.

The observable.  A ray that hits a light triangle (material 3) with data0 = (1, 1, 1) at max_depth = 1, spp = 1 returns
1 * sample_tex(uv, base-colour word) in float32: throughput is 1, the product with 1 and the sum with the 0 the radiance
starts from are exact, and so is the division by spp = 1.  A black Lambertian triangle (data0 = 0) with data3 = (1, 1, 1)
returns sample_tex(uv, emissive word) the same way: its next-event term is a product with albedo / pi = 0 and adds +0.

The tolerance (tolerance() below), per sample and channel, derived and not tuned.  u = 2^-24 is the unit roundoff of float32.
  1. The uv that reaches the sampler.  All three vertices of a triangle carry the same uv U, and the kernel forms
     U * w + U * a + U * b with w = 1 - a - b.  w carries two roundings of values <= 1 (<= 2^-25 each): w + a + b = 1 + e,
     |e| <= u.  The three products and the two sums each carry a relative error <= u on terms whose weights add up to 1 + e.
     In all |uv - U| <= (u + u + 2 u) |U| to first order; 5 u |U| covers the second-order terms.
  2. The texel coordinate.  U * 1024 is exact (a power of two), x = U * 1024 - 0.5 rounds once: <= u (|x| + 0.5); floor is
     exact and x - floor(x) is exact except just below an integer, where it rounds to 1 with an error <= 2^-25.  So the
     coordinate is off by at most d = 1024 * 5 u |U| + u (|x| + 1.5) texels, per axis.
  3. Bilinear interpolation is continuous across texel borders and its slope along an axis is a convex combination of
     differences of neighbouring texels, so the result moves by at most (d_x + d_y) * D, with D the largest difference
     (max - min, of the channel) among the texels the footprint can touch: the 4 x 4 block around the exact footprint,
     since d < 1 can move the footprint by one texel at most.
  4. Rounding of the fetch itself: q / 255 is correctly rounded (<= 2^-25), each mix a (1 - t) + b t of values <= 1 carries
     four roundings (<= 2^-23 together), and the three mixes nest two deep: <= 2 * 2^-23 + 2^-25 < 3 * 2^-23.
  tolerance = (d_x + d_y) * D + 3 * 2^-23.  With |U| <= 2.5 that is at most 2e-4 on these textures, and typically 4e-5;
  the smallest convention error moves a channel by half a level, 2e-3."""
import numpy as np

import random_scene

N = 1024                      # RT_TEX_SIZE
LAYERS = 3
U32 = 2.0 ** -24
# layer words: as the kernel decodes them (> -0.5: a texture; truncation toward zero; clamped to [0, layers - 1]) ...
WORDS = (0.0, 1.0, 2.0, 3.0, 0.7, 1.999, -0.4)
NO_TEXTURE_WORDS = (-0.5, -1.0)     # ... and two that are no texture: the fetch is skipped, the colour is data0 / data3
CHUNK = 96                    # triangles of one scene: what the LDS forms hold beside their wave queues, with room to spare
ERRORS = ("half_texel_shift", "xy_swap", "clamp_to_edge", "rb_swap", "layer_off_by_one", "weights_swapped")


def _closed_walk(start, mul_up, mul_down, phase):
    """1024 levels along an axis: periods of 64 texels, 32 steps up then 32 steps down, every step 1..8 levels, each size
    four times on the way up and four times on the way down (so every period closes, and the walk closes across the wrap
    edge), the order of the sizes another in every period."""
    k = np.arange(N)
    period, pos = k >> 6, k & 63
    up = pos < 32
    size = 1 + np.where(up, (pos * mul_up + period) % 8, ((pos - 32) * mul_down + 2 * period + phase) % 8)
    step = np.where(up, size, -size)            # step[k] = level[k + 1] - level[k]
    assert int(step.sum()) == 0
    level = start + np.concatenate([[0], np.cumsum(step)[:-1]])
    d = np.abs(np.roll(level, -1) - level)
    assert d.min() >= 1 and d.max() <= 8 and level.min() >= 0 and level.max() <= 255
    return level.astype(np.int64)


def make_textures():
    """(LAYERS, 1024, 1024, 4) u8, indexed [layer, y, x, channel].  R depends on x alone and G on y alone, neighbours 1..8
    levels apart (also across the wrap edge), by different walks and with another phase in every layer; B = 40 * layer +
    5 * (x >> 8) + 3 * (y >> 7): the layer number and a coarse pattern that x <-> y does not keep; A is noise nothing reads."""
    fx = _closed_walk(20, 3, 5, 0)
    gy = _closed_walk(60, 5, 3, 3)
    assert not np.array_equal(fx, gy)
    x, y = np.meshgrid(np.arange(N), np.arange(N))
    tex = np.empty((LAYERS, N, N, 4), np.uint8)
    for l in range(LAYERS):
        tex[l, :, :, 0] = np.roll(fx, -37 * l)[x]
        tex[l, :, :, 1] = np.roll(gy, -53 * l)[y]
        tex[l, :, :, 2] = 40 * l + 5 * (x >> 8) + 3 * (y >> 7)
        tex[l, :, :, 3] = (x * 7 + y * 13) & 255
    return tex


def sample_points():
    """-> (uv (n, 2) f32, word (n,) f32, slot (n,) int: 0 base colour on a light, 3 emissive on a black Lambertian).
    Coordinates in texels (s = u * 1024, all exact in float32): texel centres (s = i + 0.5: fx = 0) and texel borders (s = i:
    fx = 0.5), two general positions, both sides of uv = 0 and of uv = 1 within half a texel (x0 = 1023, x1 = 0), and
    uv = -1.25 and 2.5 with a neighbour each; u != v in every pair; every layer word on every pair in turn."""
    s = np.array([5.5, 701.0, 333.75, 90.3125,
                  -0.25, 0.25, 0.0, 0.5, -0.5,
                  1023.75, 1024.25, 1024.0, 1023.5, 1024.5,
                  -1280.0, 2560.0, -1279.5, 2560.25], np.float64)
    coord = (s / N).astype(np.float32)
    assert np.array_equal(coord.astype(np.float64) * N, s)
    pairs = [(i, (i + k) % len(s)) for k in (1, 5, 7, 11) for i in range(len(s))]
    uv, word, slot = [], [], []
    for p, (i, j) in enumerate(pairs):
        for q in range(4):                                   # base colour: four of the seven words on every pair
            uv.append((coord[i], coord[j])); word.append(WORDS[(p + 2 * q) % len(WORDS)]); slot.append(0)
        uv.append((coord[i], coord[j])); word.append(WORDS[(p + 3) % len(WORDS)]); slot.append(3)   # emissive: one
        if p % 3 == 0:                                       # no texture at all, in either slot
            uv.append((coord[i], coord[j])); word.append(NO_TEXTURE_WORDS[(p // 3) % 2]); slot.append(3 * ((p // 6) % 2))
    uv, word, slot = np.array(uv, np.float32), np.array(word, np.float32), np.array(slot)
    assert (uv[:, 0] != uv[:, 1]).all() and len(uv) == 4 * CHUNK
    # interleave, so that every scene of CHUNK consecutive points holds every kind
    order = np.arange(len(uv)).reshape(-1, 4).T.reshape(-1)
    return uv[order], word[order], slot[order]


def scene(uv, word, slot, textures):
    """A one-instance bridge (identity transform, one-leaf TLAS) of one tiny triangle per sample point in the plane z = 0,
    all three vertex uvs equal to the point's, and the rays (n, 8) f32 in the rt_ray layout, one per triangle, aimed at its
    centroid.  The first two light triangles are the scene's light list."""
    n = len(uv)
    rng = np.random.default_rng(4)
    cx, cy = (np.arange(n) % 12) * 0.05 - 0.3, (np.arange(n) // 12) * 0.05 - 0.2
    corner = np.array([[-0.011, -0.007, 0.0], [0.012, -0.008, 0.0], [0.001, 0.013, 0.0]])
    tri = (np.stack([cx, cy, np.zeros(n)], axis=1)[:, None, :] + corner[None]).astype(np.float32)
    bmin, bmax = tri.min(axis=1) - 1e-4, tri.max(axis=1) + 1e-4
    order = np.arange(n)
    nodes = random_scene._build_bvh(bmin, bmax, order, rng, 4, lambda first, count: (first << 3) | count)
    topo = np.zeros((n, 20), np.uint32)
    f = topo.view(np.float32)
    for pos, t in enumerate(order):
        topo[pos, 0:3] = 3 * t + np.arange(3)
        f[pos, 12:16] = -1.0
        f[pos, 19] = -1.0
        f[pos, 9], f[pos, 10] = 0.5, 1.5
        if slot[t] == 0:
            f[pos, 4:8] = (1.0, 1.0, 1.0, 3.0)
            f[pos, 12] = word[t]
        else:
            f[pos, 4:8] = (0.0, 0.0, 0.0, 0.0)
            f[pos, 15] = word[t]
            f[pos, 16:19] = 1.0
    lights = [v for pos in np.flatnonzero(f[:, 7] == 3.0)[:2] for v in (0, int(pos))]
    vertices = np.concatenate([tri.reshape(-1, 3), np.ones((3 * n, 1), np.float32)], axis=1).reshape(-1)
    normals = np.tile(np.array([0, 0, -1, 0], np.float32), 3 * n)
    inst = np.zeros(36, np.float32)
    inst[0:16] = inst[16:32] = np.eye(4, dtype=np.float32).reshape(-1)
    tlas = random_scene._pack([[bmin.min(axis=0) - 1e-3, bmax.max(axis=0) + 1e-3, 1, (0 << 3) | 1]])
    cam = np.zeros(24, np.float32)               # a query reads no camera; upload_scene wants one
    cam[0:3], cam[4:7], cam[8:11], cam[12:15] = (0, 0, -4), (-1, -1, -1), (2, 0, 0), (0, 2, 0)
    cam[16:19], cam[20:23] = (1, 0, 0), (0, 1, 0)
    b = random_scene.Bridge(vertices=vertices, normals=normals, uvs=np.repeat(uv, 3, axis=0).reshape(-1).astype(np.float32),
                            mesh_topology=topo.reshape(-1), tlas=tlas, blas=random_scene._pack(nodes), instances=inst,
                            lights=np.array(lights, np.uint32), draw_commands=np.array([3 * n, 1, 0, 0], np.uint32),
                            cameraData=cam, textures=list(textures))
    rays = np.zeros((n, 8), np.float32)
    centroid = tri.astype(np.float64).mean(axis=1)
    rays[:, 0:3] = centroid - np.array([0.3, 0.2, 1.0])      # no axis-parallel ray: every slab test is an ordinary one
    rays[:, 3] = 1e30
    rays[:, 4:7] = (0.3, 0.2, 1.0)
    return b, rays


def scenes(textures):
    """the sample points in scenes of CHUNK triangles: [(bridge, rays with pads, slice of the sample arrays)]"""
    import radiance_util as ru
    uv, word, slot = sample_points()
    out = []
    for lo in range(0, len(uv), CHUNK):
        sl = slice(lo, lo + CHUNK)
        b, rays = scene(uv[sl], word[sl], slot[sl], textures)
        out.append((b, ru.with_pads(rays), sl))
    return out


def decode_layer(word, layers=LAYERS):
    """the layer a record's texture word names, as the kernel decodes it, or -1 for no texture: `word > -0.5` (false for a
    NaN), conversion to i32 by truncation toward zero, clamped to [0, layers - 1]"""
    w = np.asarray(word, np.float64)
    with np.errstate(invalid="ignore"):
        has = w > -0.5
    layer = np.clip(np.trunc(np.where(has, w, 0.0)), 0, layers - 1).astype(np.int64)
    return np.where(has, layer, -1)


def reference(tex, uv, word, error=None):
    """textureSampleLevel(t, s, uv, layer, 0) of the WebGPU specification in float64, for a 2d-array texture of rgba8unorm
    texels with a repeat / linear sampler: the texel i covers [i, i + 1) / 1024 with its centre at (i + 0.5) / 1024; the
    sample is the bilinear blend of the four texels whose centres surround uv * 1024, addresses wrapped modulo 1024; a
    unorm texel is q / 255.  -> (rgb (n, 3) f64, footprint corner (n, 2) i64, layer (n,) i64; -1: no texture, rgb = 1).
    `error`: one of ERRORS, the convention error to commit on purpose."""
    assert error is None or error in ERRORS
    uv = np.asarray(uv, np.float64)
    layer = decode_layer(word, tex.shape[0])
    has = layer >= 0
    lay = np.where(has, layer, 0)
    if error == "layer_off_by_one":
        lay = np.minimum(lay + 1, tex.shape[0] - 1)
    p = uv * N - (0.0 if error == "half_texel_shift" else 0.5)
    i0 = np.floor(p)
    frac = p - i0
    i0 = i0.astype(np.int64)
    if error == "weights_swapped":
        frac = 1.0 - frac

    def addr(i):
        return np.clip(i, 0, N - 1) if error == "clamp_to_edge" else i % N

    def texel(ix, iy):
        xx, yy = addr(ix), addr(iy)
        if error == "xy_swap":
            xx, yy = yy, xx
        return tex[lay, yy, xx, :3].astype(np.float64) / 255.0

    fx, fy = frac[:, 0:1], frac[:, 1:2]
    x0, y0 = i0[:, 0], i0[:, 1]
    top = texel(x0, y0) * (1.0 - fx) + texel(x0 + 1, y0) * fx
    bot = texel(x0, y0 + 1) * (1.0 - fx) + texel(x0 + 1, y0 + 1) * fx
    rgb = top * (1.0 - fy) + bot * fy
    if error == "rb_swap":
        rgb = rgb[:, ::-1]
    return np.where(has[:, None], rgb, 1.0), i0, layer


def tolerance(tex, uv, word):
    """(n, 3) f64: the bound of the module docstring, per sample and channel (no texture: the value is exact)"""
    uv64 = np.asarray(uv, np.float64)
    _, i0, layer = reference(tex, uv, word)
    p = np.abs(uv64 * N - 0.5)
    d = N * 5 * U32 * np.abs(uv64) + U32 * (p + 1.5)              # texels, per axis
    assert d.max() < 1.0
    lay = np.maximum(layer, 0)
    k = np.arange(-1, 3)
    xx = (i0[:, 0, None] + k[None]) % N
    yy = (i0[:, 1, None] + k[None]) % N
    block = tex[lay[:, None, None], yy[:, :, None], xx[:, None, :], :3].astype(np.float64) / 255.0     # (n, 4, 4, 3)
    D = block.max(axis=(1, 2)) - block.min(axis=(1, 2))
    tol = d.sum(axis=1)[:, None] * D + 3 * 2.0 ** -23
    return np.where((layer >= 0)[:, None], tol, 0.0)
