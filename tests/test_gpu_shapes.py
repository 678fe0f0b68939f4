"""Every kernel form at degenerate image shapes, stripe partitions and resizes, against the CPU oracle bit for bit.

The rest of the suite renders comfortable sizes.  The index arithmetic that depends on the shape is exercised here:
the 8x8 tile tickets and the x | y << 16 pixel packing of the persistent kernel (up to 65535 per side), the
queue-id -> (frame, pixel) split of the wavefront shade kernel, the tile grid of primary visibility (four tiles per
workgroup), the 16x16 post-pass blocks with their clamped halo, the batch accumulation grid, the compact tile-row list of
tile-aligned stripes (ranks that own no row included) and the buffers a live context keeps across rt_resize.  The last
test checks primary visibility against an independent float64 ray cast, which bit parity with the oracle cannot replace
(an error both sides share, such as swapped x / y, would pass it).
"""
import numpy as np
import pytest

import parity_util as pu
import random_scene
import test_gpu_product_build as pb

pytestmark = pytest.mark.gpu

FRAMES = (1, 2, 3)
DEPTH = 4

SHAPES = [
    (1, 1), (1, 2), (2, 1), (7, 3),             # tiny
    (8, 8), (9, 9),                             # around the 8x8 tile
    (63, 1), (1, 63), (65, 1), (1, 65),         # one row / column around a wave
    (15, 33), (17, 17),                         # around the 16x16 post block
    (257, 3), (3, 257), (4096, 1), (1, 4096),   # long and thin
    (65535, 1), (1, 65535),                     # the x | y << 16 packing limit of the persistent kernel
]
SMALL_SHAPES = [(1, 1), (7, 3), (1, 65), (65, 1), (17, 17)]
THIN_SHAPES = [(1, 1), (3, 257), (257, 3)]
FORMS = [(1, None), (2, 0), (2, 1)]   # persistent; wavefront with the node walk and with the pair walk

_scenes = {}


def _textured_scene():
    if "textured" not in _scenes:
        _scenes["textured"] = random_scene.make(24, with_textures=True)
    return _scenes["textured"]


def _renderer(W, variant, walk=None):
    r = W.WebGPURenderer(0)
    r.setKernelVariant(variant)
    if walk is not None:
        r.setWalk(walk)
    return r


def _check_gbuffer(gpu, cpu, what=""):
    for name, g, c in zip(("albedo", "normal_id", "depth"), gpu.readGBuffer(), cpu.readGBuffer()):
        assert np.array_equal(pu.bits(g), pu.bits(c)), pu.describe_mismatch(what + "G-buffer " + name, g, c)


def _live_loop(W, oracle_lib, b, w, h, variant, walk, spp=1, frames=FRAMES):
    """compute(f); present() per frame on a fresh renderer and a fresh oracle: every parity artefact must agree."""
    cpu = oracle_lib.OracleRenderer()
    gpu = _renderer(W, variant, walk)
    try:
        pu.drive(gpu, W, b, w, h, DEPTH, spp, frames, present=True)
        pu.drive(cpu, W, b, w, h, DEPTH, spp, frames, present=True)
        pu.assert_parity(gpu, cpu, check_output=True)
        _check_gbuffer(gpu, cpu)
        assert gpu.getCounters()["primary_rays"] == w * h * len(frames)
    finally:
        gpu.destroy()


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("variant,walk", FORMS)
def test_cornell_shape_matrix(W, oracle_lib, w, h, variant, walk):
    _live_loop(W, oracle_lib, pu.bridge_for(W, "cornell"), w, h, variant, walk)


@pytest.mark.parametrize("w,h", SMALL_SHAPES)
@pytest.mark.parametrize("variant,spp", [(0, 1), (3, 1), (1, 4)])
def test_cornell_other_forms_small_shapes(W, oracle_lib, w, h, variant, spp):
    """the one-pixel-per-lane megakernel, the auto choice and SPP > 1 inside one persistent dispatch"""
    _live_loop(W, oracle_lib, pu.bridge_for(W, "cornell"), w, h, variant, None, spp=spp)


@pytest.mark.parametrize("w,h", THIN_SHAPES)
@pytest.mark.parametrize("variant,walk", FORMS)
def test_global_memory_paths_thin_shapes(W, oracle_lib, w, h, variant, walk):
    """instanced1000 does not fit LDS: nodes, triangles and instance rows are read through the L1"""
    _live_loop(W, oracle_lib, pu.bridge_for(W, "instanced1000"), w, h, variant, walk)


@pytest.mark.parametrize("w,h", THIN_SHAPES)
@pytest.mark.parametrize("variant,walk", FORMS)
def test_textured_random_scene_thin_shapes(W, oracle_lib, w, h, variant, walk):
    _live_loop(W, oracle_lib, _textured_scene(), w, h, variant, walk)


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("variant", [1, 2])
def test_cornell_batch_of_three(W, oracle_lib, w, h, variant):
    """computeBatch of 3 frames: the first two frames' G-buffers go to the gbuf_batch planes, the colours to frame_col,
    and k_accumulate_frames adds them in order"""
    b = pu.bridge_for(W, "cornell")
    cpu = oracle_lib.OracleRenderer()
    pu.drive(cpu, W, b, w, h, DEPTH, 1, FRAMES, present=False)
    gpu = _renderer(W, variant)
    try:
        gpu.buildPipeline(DEPTH, 1)
        W.upload_scene(gpu, b, w, h)
        gpu.setCounting(True)
        gpu.resetCounters()
        gpu.computeBatch(list(FRAMES))
        gpu.sync()
        pu.assert_parity(gpu, cpu, check_output=False)
        gpu.present()
        cpu.present()
        pu.assert_parity(gpu, cpu, check_output=True, check_counters=False)
    finally:
        gpu.destroy()


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (1, 65), (65, 1), (17, 17), (3, 257), (4096, 1), (1, 65535)])
@pytest.mark.parametrize("variant,walk", FORMS)
@pytest.mark.parametrize("batch", [1, 3])
def test_product_build_shapes(W, oracle_lib, w, h, variant, walk, batch):
    """the kernels bench.py times (detailed counters off)"""
    b = pu.bridge_for(W, "cornell")
    cpu = oracle_lib.OracleRenderer()
    pu.drive(cpu, W, b, w, h, DEPTH, 1, FRAMES, present=False)
    gpu = W.WebGPURenderer(0)
    try:
        pb._run(W, gpu, b, w, h, DEPTH, 1, FRAMES, batch, variant, walk)
        pb._check(gpu, cpu)
    finally:
        gpu.destroy()


# ---------------------------------------------------------------- stripes

STRIPE_W = 21
STRIPE_HEIGHTS = (1, 5, 8, 17, 67)


@pytest.mark.parametrize("rows", [1, 3, 8, 16])
@pytest.mark.parametrize("count", [2, 3, 8])
@pytest.mark.parametrize("variant", [1, 2])
def test_stripes_at_odd_shapes(W, oracle_lib, rows, count, variant):
    """setStripes(rows, rank, count) for every rank, heights 1 .. 67: a rank writes nothing outside its rows, its rows equal
    a striped oracle run, the ranks' images sum to the full render bit for bit and their counters to its counters.  Many of
    these ranks own no row at all (rows = 8 or 16: the compact tile-row list is empty, own_tile_rows = 0)."""
    b = pu.bridge_for(W, "cornell")
    w, frames = STRIPE_W, (1, 2)
    for h in STRIPE_HEIGHTS:
        full_r = _renderer(W, variant)
        try:
            pu.drive(full_r, W, b, w, h, DEPTH, 1, frames, present=False)
            full, full_counts = full_r.readAccum(), full_r.getCounters()
        finally:
            full_r.destroy()
        cpu = oracle_lib.OracleRenderer()
        pu.drive(cpu, W, b, w, h, DEPTH, 1, frames, present=False)
        assert np.array_equal(pu.bits(full), pu.bits(cpu.readAccum())), \
            pu.describe_mismatch("full render (h=%d)" % h, full, cpu.readAccum())
        total = np.zeros_like(full)
        counts = {}
        for rank in range(count):
            what = "h=%d rank %d: " % (h, rank)
            r = _renderer(W, variant)
            try:
                r.setStripes(rows, rank, count)
                pu.drive(r, W, b, w, h, DEPTH, 1, frames, present=False)
                part = r.readAccum()
                rank_counts = r.getCounters()
            finally:
                r.destroy()
            owned = (np.arange(h) // rows) % count == rank
            assert not part[~owned].any(), what + "wrote outside its rows"
            ref = oracle_lib.OracleRenderer()
            ref.setStripes(rows, rank, count)
            pu.drive(ref, W, b, w, h, DEPTH, 1, frames, present=False)
            want = ref.readAccum()
            assert np.array_equal(pu.bits(part[owned]), pu.bits(want[owned])), \
                pu.describe_mismatch(what + "owned rows", part[owned], want[owned])
            assert rank_counts == ref.getCounters(), what + "counters"
            total += part
            for k, v in rank_counts.items():
                counts[k] = counts.get(k, 0) + v
        assert np.array_equal(pu.bits(total), pu.bits(full)), pu.describe_mismatch("h=%d stripe sum" % h, total, full)
        assert counts == full_counts, "h=%d: stripe counters do not add up" % h


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_more_ranks_than_tile_rows_batched(W, oracle_lib, variant):
    """distributed.py's default stripes (one 8-row tile row) at 64x36 over 8 ranks: ranks 5-7 own no tile row.  Before the
    fix the primary-visibility launch of such a rank got a grid of x-size 0 and compute() failed with "invalid
    configuration argument".  Batched dispatches: the primary grid has one y-slice per frame."""
    from webgpu_raytracer_amd.distributed import STRIPE_ROWS
    b = pu.bridge_for(W, "cornell")
    w, h, frames, count = 64, 36, [1, 2, 3, 4], 8
    cpu = oracle_lib.OracleRenderer()
    pu.drive(cpu, W, b, w, h, DEPTH, 1, frames, present=False)
    want = cpu.readAccum()
    total = np.zeros_like(want)
    for rank in range(count):
        r = _renderer(W, variant)
        try:
            r.setStripes(STRIPE_ROWS, rank, count)
            r.buildPipeline(DEPTH, 1)
            W.upload_scene(r, b, w, h)
            r.computeBatch(frames)
            r.sync()
            part = r.readAccum()
        finally:
            r.destroy()
        owned = (np.arange(h) // STRIPE_ROWS) % count == rank
        assert not part[~owned].any()
        total += part
    assert np.array_equal(pu.bits(total), pu.bits(want)), pu.describe_mismatch("stripe sum", total, want)


# ---------------------------------------------------------------- resize on a live context

RESIZES = [(96, 64), (1, 1), (65, 1), (96, 64), (7, 3), (33, 21)]
BATCHES = (4, 1, 3)


@pytest.mark.parametrize("scene,variant,walk,lookahead", [
    ("cornell", 1, None, 0),
    ("cornell", 1, None, 4),          # compute() traces ahead; rt_resize must drop what was traced for the old screen
    ("cornell", 2, 0, 0),
    ("cornell", 2, 1, 0),
    ("instanced1000", 3, None, 0),    # auto: wavefront form for the 4-frame batches, persistent kernel otherwise
])
def test_resize_sequence_on_live_context(W, oracle_lib, scene, variant, walk, lookahead):
    """One renderer through 96x64 -> 1x1 -> 65x1 -> 96x64 -> 7x3 -> 33x21 with the batch size changing between steps
    (4, 1, 3): every step must equal one oracle renderer driven through the same sequence (totalFrames carries across).
    Buffers that survive the resize (frame_col, gbuf_batch, wavefront path state and queues, the occupancy cache, the
    slot ring) were sized or shaped for another screen."""
    b = pu.bridge_for(W, scene)
    cpu = oracle_lib.OracleRenderer()
    gpu = _renderer(W, variant, walk)
    try:
        detailed = lookahead == 0     # lookahead is off while the detailed counters are on
        if lookahead:
            gpu.setLookahead(lookahead)
        for r in (gpu, cpu):
            r.buildPipeline(DEPTH, 1)
            W.upload_scene(r, b, *RESIZES[0])
        gpu.setCounting(detailed)
        frames = (1, 2, 3, 4)
        for step, (w, h) in enumerate(RESIZES):
            what = "step %d (%dx%d): " % (step, w, h)
            if step:
                b.updateCamera(w, h)
                for r in (gpu, cpu):
                    r.updateScreenSize(w, h)
                    r.updateSceneUniforms(b.cameraData, 0, b.lightCount)
                    r.resetAccumulation()
            for r in (gpu, cpu):
                r.resetCounters()
            batch = BATCHES[step % len(BATCHES)]
            for i in range(0, len(frames), batch):
                chunk = frames[i:i + batch]
                if lookahead or len(chunk) == 1:
                    for f in chunk:
                        gpu.compute(f)
                else:
                    gpu.computeBatch(list(chunk))
            for f in frames:
                cpu.compute(f)
            gpu.sync()
            ga, ca = gpu.readAccum(), cpu.readAccum()
            assert np.array_equal(pu.bits(ga), pu.bits(ca)), pu.describe_mismatch(what + "accumulation", ga, ca)
            _check_gbuffer(gpu, cpu, what)
            assert np.array_equal(gpu.readUniforms(), cpu.readUniforms()), what + "uniform block"
            if detailed:   # with lookahead the counters include the frames traced ahead
                assert gpu.getCounters() == cpu.getCounters(), what + "counters"
            gpu.present()
            cpu.present()
            go, co = gpu.captureFrame()["data"], cpu.captureFrame()["data"]
            assert np.array_equal(go, co), pu.describe_mismatch(what + "RGBA8 output", go, co)
    finally:
        gpu.destroy()


# ---------------------------------------------------------------- primary visibility against a float64 ray cast

# Two triangles in view-plane coordinates (u, v) in [0, 1]^2 (u to the right, v up): A covers u + v < 0.8 at the
# view-plane distance, B covers u + v > 1.2 half as far again; between them is background.  A row or column of the view
# crosses at least two of the three regions wherever the jitter puts it.
TRI_UV = {0: ((-0.5, -0.5), (1.3, -0.5), (-0.5, 1.3)), 1: ((1.5, 1.5), (-0.3, 1.5), (1.5, -0.3))}
TRI_T = {0: 1.0, 1: 1.5}


def _diagonal_scene():
    cam = np.zeros(24, dtype=np.float32)
    eye = np.array([0.0, 0.2, -4.2], np.float32)
    hor, ver = np.array([3.6, 0, 0], np.float32), np.array([0, 2.7, 0], np.float32)
    cam[0:3] = eye
    cam[4:7] = eye + np.array([0, 0, 3.0], np.float32) - hor / 2 - ver / 2
    cam[8:11], cam[12:15] = hor, ver
    cam[16:19], cam[20:23] = [1, 0, 0], [0, 1, 0]
    e, ll = eye.astype(np.float64), cam[4:7].astype(np.float64)
    verts, topo, blas, inst, draw, boxes = [], [], [], [], [], []
    for g in (0, 1):
        tri = np.array([e + TRI_T[g] * (ll + u * hor + v * ver - e) for u, v in TRI_UV[g]], np.float32)
        verts.append(tri)
        row = np.zeros(20, np.uint32)
        f = row.view(np.float32)
        row[0:3] = 3 * g + np.arange(3)
        row[3] = g
        f[4:7] = (0.8, 0.5, 0.2) if g == 0 else (0.2, 0.5, 0.8)
        f[7] = 0.0                                   # lambertian
        f[12:16] = -1.0                              # no textures
        f[19] = -1.0
        topo.append(row)
        lo, hi = tri.min(axis=0) - 1e-4, tri.max(axis=0) + 1e-4
        boxes.append((lo, hi))
        blas.append([lo, hi, 1, (g << 3) | 1])        # a BLAS of one leaf holding triangle g
        m = np.eye(4, dtype=np.float32)
        row_i = np.zeros(36, np.float32)
        row_i[0:16] = m.reshape(-1)
        row_i[16:32] = m.reshape(-1)
        row_i.view(np.uint32)[32:36] = [g, 0, g, 0]
        inst.append(row_i)
        draw += [3, 1, 3 * g, g]
    lo = np.minimum(boxes[0][0], boxes[1][0])
    hi = np.maximum(boxes[0][1], boxes[1][1])
    tlas = [[lo, hi, 3, 0], [boxes[0][0], boxes[0][1], 2, (0 << 3) | 1], [boxes[1][0], boxes[1][1], 3, (1 << 3) | 1]]
    V = np.concatenate(verts)
    n = np.tile(np.array([0, 0, -1, 0], np.float32), (len(V), 1))
    return random_scene.Bridge(
        vertices=np.concatenate([V, np.ones((len(V), 1), np.float32)], axis=1).reshape(-1),
        normals=n.reshape(-1), uvs=np.zeros(2 * len(V), np.float32), mesh_topology=np.concatenate(topo),
        tlas=random_scene._pack(tlas), blas=random_scene._pack(blas), instances=np.concatenate(inst),
        lights=np.zeros(0, np.uint32), draw_commands=np.array(draw, np.uint32), cameraData=cam, textures=None), V


def _classify(uniforms, V, w, h):
    """float64 pinhole ray of every pixel (start_sample: u = (x + 0.5 + jitter.x * W) / W, v = 1 - (y + 0.5 + jitter.y *
    H) / H), cast against both triangles.  Returns (class per pixel: -1 background, else the triangle; mask of pixels whose
    ray passes within 1e-5 (barycentric) of a triangle edge)."""
    f = uniforms.view(np.float32)
    o, ll, hor, ver = (f[4 * i:4 * i + 3].astype(np.float64) for i in range(4))
    jx, jy = float(f[56]), float(f[57])                    # jitter at byte 224
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    u = (xs + 0.5 + jx * w) / w
    v = 1.0 - (ys + 0.5 + jy * h) / h
    d = ll[None, None] + u[..., None] * hor + v[..., None] * ver - o
    cls = np.full((h, w), -1, np.int64)
    best = np.full((h, w), np.inf)
    near = np.zeros((h, w), bool)
    for g in (0, 1):
        a, b, c = (V[3 * g + k].astype(np.float64) for k in range(3))
        e1, e2 = b - a, c - a
        p = np.cross(d, e2)
        det = p @ e1
        s = o - a
        bu = (p @ s) / det
        q = np.cross(s, e1)
        bv = (d @ q) / det
        t = (q @ e2) / det
        bw = 1.0 - bu - bv
        inside = (bu >= 0) & (bv >= 0) & (bw >= 0) & (t > 0)
        near |= (t > 0) & (np.minimum(np.minimum(np.abs(bu), np.abs(bv)), np.abs(bw)) < 1e-5)
        take = inside & (t < best)
        cls[take] = g
        best[take] = t[take]
    return cls, near


@pytest.mark.parametrize("w,h", [(1, 65), (65, 1), (1, 4096), (4096, 1), (7, 3), (257, 3)])
def test_primary_visibility_against_float64_cast(W, oracle_lib, w, h):
    b, V = _diagonal_scene()
    gpu = W.WebGPURenderer(0)
    cpu = oracle_lib.OracleRenderer()
    try:
        for r in (gpu, cpu):
            pu.drive(r, W, b, w, h, 1, 1, (1, 2), present=False)
        _check_gbuffer(gpu, cpu)
        u = gpu.readUniforms()
        _, nid, dep = gpu.readGBuffer()
        cls, near = _classify(u, V, w, h)
        ok = ~near
        assert ok.mean() > 0.95, "only %d of %d pixels are away from an edge" % (int(ok.sum()), ok.size)
        assert len(set(cls[ok].tolist())) >= 2, "the image never crosses an edge"
        bg = dep >= 1.0
        assert np.array_equal(bg[ok], cls[ok] < 0), "background mask: %d pixels differ" % int((bg[ok] != (cls[ok] < 0)).sum())
        ids = nid[..., 2:4].view(np.uint32)
        hit = ok & (cls >= 0)
        assert np.array_equal(ids[hit][:, 0], cls[hit].astype(np.uint32)), "triangle ids"
        assert np.array_equal(ids[hit][:, 1], cls[hit].astype(np.uint32)), "instance ids"
        assert not nid[ok & (cls < 0)].any()
    finally:
        gpu.destroy()
