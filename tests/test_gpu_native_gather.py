"""The sharded image as a capability of the library itself (rt_dist_*, include/mi355rt.h): HIP pack / unpack kernels, the
host-moved exchange (rt_dist_read_block / rt_dist_write_block) and the RCCL gather (rt_gather_stripes).

Every comparison is bit for bit, and the reference is always ONE plain WebGPURenderer context rendering the same frames.
The shares of the cases are worked out by hand from the ownership rule (row y belongs to rank (y / stripe_rows) % world):
  160 x 96, world 2, stripe 8   rows 0-7 -> 0, 8-15 -> 1, ...: 6 stripes each                  48 / 48
  100 x 52, world 3, stripe 8   stripes 0..6 -> ranks 0 1 2 0 1 2 0, the last one cut to 4 rows   20 / 16 / 16
  64 x 16,  world 3, stripe 8   two stripes, rank 2 owns nothing                               8 / 8 / 0
  96 x 40,  world 2, stripe 5   8 stripes of 5 rows (not tile-aligned)                          20 / 20
  96 x 64,  world 1             everything                                                     64
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import parity_util as pu

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(REPO, "tests", "native_gather_child.py")
DEPTH, FRAMES_A, FRAMES_B, BATCH = 6, tuple(range(1, 9)), tuple(range(9, 13)), 4

CASES = [
    ("cornell", 160, 96, 2, 8, (48, 48)),
    ("cornell", 100, 52, 3, 8, (20, 16, 16)),
    ("cornell", 64, 16, 3, 8, (8, 8, 0)),
    ("cornell", 96, 40, 2, 5, (20, 20)),
    ("cornell", 96, 64, 1, 8, (64,)),
    ("mixed", 100, 52, 3, 8, (20, 16, 16)),
    ("viewer_diamond", 96, 40, 2, 5, (20, 20)),
]


def spec_rows(rank, world, stripe, height):
    """The unchanged Python restatement of the layout (distributed.ShardedImage.rows_of) as the independent spec."""
    from webgpu_raytracer_amd.distributed import ShardedImage
    return ShardedImage.rows_of(types.SimpleNamespace(stripe_rows=stripe, world=world), rank, height)


def new_context(W, scene, w, h, depth=DEPTH):
    b = pu.bridge_for(W, scene)
    r = W.WebGPURenderer(0)
    r.buildPipeline(depth, 1)
    W.upload_scene(r, b, w, h)
    return r


def render(r, frames):
    for i in range(0, len(frames), BATCH):
        r.computeBatch(frames[i:i + BATCH])


def single_context_moments(W, scene, w, h, moments=(FRAMES_A, FRAMES_B)):
    r = new_context(W, scene, w, h)
    out = []
    for frames in moments:
        render(r, frames)
        r.present()
        r.sync()
        out.append((r.readAccum().copy(), r.captureFrame()["data"].copy()))
    r.destroy()
    return out


def host_gather(ranks):
    """pack on every rank, carry every block to rank 0 through the host, unpack + present there; returns the blocks"""
    blocks = []
    for r in ranks:
        r.packStripes()
        blocks.append(r.readBlock().copy())
    for k, blk in enumerate(blocks):
        ranks[0].writeBlock(k, blk)
    ranks[0].unpackStripes()
    ranks[0].present()
    ranks[0].sync()
    return blocks


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("scene,w,h,world,stripe,shares", CASES,
                         ids=["%s-%dx%d-w%d-s%d" % c[:5] for c in CASES])
def test_contexts_as_ranks_with_host_exchange_equal_one_context(W, scene, w, h, world, stripe, shares):
    """`world` contexts on device 0 without a communicator: each renders its stripes and packs, the test carries the blocks
    to rank 0, rank 0 unpacks and presents.  Display buffer and RGBA8 output equal the single context's at two moments of a
    progressive render; every block is the documented layout; nobody wrote outside its rows."""
    W._build.build_rt()
    assert [len(spec_rows(k, world, stripe, h)) for k in range(world)] == list(shares)
    ref = single_context_moments(W, scene, w, h)
    ranks = [new_context(W, scene, w, h) for _ in range(world)]
    try:
        for k, r in enumerate(ranks):
            r.distInit(k, world, stripe)
            assert r.distBlockBytes() == max(shares) * w * 16
        assert not ranks[0].readDisplay().any(), "the display buffer does not start zeroed"
        for m, frames in enumerate((FRAMES_A, FRAMES_B)):
            for r in ranks:
                render(r, frames)
            blocks = host_gather(ranks)
            for k, blk in enumerate(blocks):
                rows = spec_rows(k, world, stripe, h)
                assert blk.shape == (max(shares), w, 4)
                assert same_bits(blk[:len(rows)], ref[m][0][rows]), "block of rank %d is not single_accum[rows_of(rank)]" % k
                assert not blk[len(rows):].view(np.uint32).any(), "padding rows of rank %d's block are not zero" % k
            disp = ranks[0].readDisplay()
            assert same_bits(disp, ref[m][0]), pu.describe_mismatch("assembled image %d" % m, disp, ref[m][0])
            got = ranks[0].captureFrame()["data"]
            assert np.array_equal(got, ref[m][1]), pu.describe_mismatch("RGBA8 output %d" % m, got, ref[m][1])
        for k, r in enumerate(ranks):
            own = np.zeros(h, bool)
            own[spec_rows(k, world, stripe, h)] = True
            acc = r.readAccum()
            assert not acc[~own].view(np.uint32).any(), "rank %d wrote outside its rows (or a gather touched its accumulator)" % k
            assert same_bits(acc[own], ref[1][0][own])
    finally:
        for r in ranks:
            r.destroy()


def test_native_sharded_image_with_an_exchange_function(W):
    """distributed.NativeShardedImage without a unique id: the caller's exchange function moves the blocks."""
    from webgpu_raytracer_amd.distributed import NativeShardedImage
    W._build.build_rt()
    w, h, world = 100, 52, 3
    ref = single_context_moments(W, "cornell", w, h)
    mailbox = {}

    def exchange(rank, block):
        mailbox[rank] = block.copy()
        return mailbox

    ranks = [new_context(W, "cornell", w, h) for _ in range(world)]
    try:
        shards = [NativeShardedImage(r, k, world, 8, exchange=exchange) for k, r in enumerate(ranks)]
        assert shards[1].wire_bytes_per_rank() == 20 * w * 16
        for m, frames in enumerate((FRAMES_A, FRAMES_B)):
            for s in shards:
                s.render(frames, batch=BATCH)
            for s in reversed(shards):   # rank 0 last: by then every block is in the mailbox
                s.gather(present=True)
            shards[0].synchronize()
            assert same_bits(shards[0].read_image(), ref[m][0])
            assert np.array_equal(ranks[0].captureFrame()["data"], ref[m][1])
        with pytest.raises(ValueError):
            NativeShardedImage(ranks[0], 0, 2)
    finally:
        for r in ranks:
            r.destroy()


def test_a_rank_follows_a_resize_without_rebinding(W):
    """After updateScreenSize the blocks and the display buffer are the context's own business: the next gather equals the
    single context at the new size, rt_dist_block_bytes follows, the display buffer starts zeroed again."""
    W._build.build_rt()
    world, stripe = 2, 8
    (w0, h0), (w1, h1) = (96, 40), (120, 70)   # 70 rows: stripes 0..8, the last cut to 6 rows: 38 / 32
    b = pu.bridge_for(W, "cornell")

    def resize(r):
        r.updateScreenSize(w1, h1)
        b.updateCamera(w1, h1)
        r.updateSceneUniforms(b.cameraData, 0, b.lightCount)

    single = new_context(W, "cornell", w0, h0)
    render(single, FRAMES_A)
    single.present()
    resize(single)
    render(single, FRAMES_B)
    single.present()
    single.sync()
    ref_acc, ref_rgba = single.readAccum().copy(), single.captureFrame()["data"].copy()
    single.destroy()

    ranks = [new_context(W, "cornell", w0, h0) for _ in range(world)]
    try:
        for k, r in enumerate(ranks):
            r.distInit(k, world, stripe)
            assert r.distBlockBytes() == 24 * w0 * 16       # 40 rows: stripes 0 1 0 1 0 -> 24 / 16
            render(r, FRAMES_A)
        host_gather(ranks)
        for r in ranks:
            resize(r)
            assert r.distBlockBytes() == 38 * w1 * 16
        assert not ranks[0].readDisplay().any()
        for r in ranks:
            render(r, FRAMES_B)
        host_gather(ranks)
        assert same_bits(ranks[0].readDisplay(), ref_acc)
        assert np.array_equal(ranks[0].captureFrame()["data"], ref_rgba)
    finally:
        for r in ranks:
            r.destroy()


def test_misuse_is_refused_and_leaves_the_context_renderable(W):
    W._build.build_rt()
    w, h = 64, 48
    ref = single_context_moments(W, "cornell", w, h, moments=(FRAMES_B,))[0]
    r0, r1 = new_context(W, "cornell", w, h), new_context(W, "cornell", w, h)
    try:
        # a plain context has no blocks
        for call in (r0.packStripes, r0.unpackStripes, r0.gatherStripes, r0.readDisplay, r0.readBlock):
            with pytest.raises(W.RendererError, match="no rank"):
                call()
        assert r0.distBlockBytes() == 0
        # arguments of rt_dist_init
        with pytest.raises(W.RendererError, match="rank >= world"):
            r0.distInit(2, 2, 8)
        with pytest.raises(W.RendererError, match="world must be"):
            r0.distInit(0, 0, 8)
        with pytest.raises(W.RendererError, match="stripe_rows"):
            r0.distInit(0, 2, 0)
        assert r0.distBlockBytes() == 0
        r0.distInit(0, 2, 8)
        r1.distInit(1, 2, 8)
        block = r0.distBlockBytes()
        assert block == 24 * w * 16
        with pytest.raises(W.RendererError, match="a rank already"):
            r0.distInit(0, 2, 8)
        # rank-0-only entry points on rank 1
        for call in (r1.unpackStripes, r1.readDisplay, lambda: r1.writeBlock(0, np.zeros(block, np.uint8))):
            with pytest.raises(W.RendererError, match="only rank 0"):
                call()
        with pytest.raises(W.RendererError, match="from_rank >= world"):
            r0.writeBlock(2, np.zeros(block, np.uint8))
        for n in (block - 16, block + 16):
            with pytest.raises(W.RendererError, match="rt_dist_block_bytes"):
                r0.writeBlock(1, np.zeros(n, np.uint8))
        # external bindings and a contradicting stripe spec
        with pytest.raises(W.RendererError, match="rank of a sharded image"):
            r0.bindAccum(r1.accumDevicePtr())
        with pytest.raises(W.RendererError, match="rank of a sharded image"):
            r0.bindPresentSource(r1.accumDevicePtr())
        for spec in ((8, 1, 2), (16, 0, 2), (8, 0, 3), (8, 0, 1)):
            with pytest.raises(W.RendererError, match="contradicts the rank"):
                r0.setStripes(*spec)
        r0.setStripes(8, 0, 2)   # saying the same again is fine
        # no communicator: the collective is refused and names the way that works
        with pytest.raises(W.RendererError, match="rt_dist_write_block"):
            r0.gatherStripes()
        # nothing above was enqueued or changed anything: the two ranks still assemble the single context's image
        for r in (r0, r1):
            render(r, FRAMES_B)
        host_gather([r0, r1])
        assert same_bits(r0.readDisplay(), ref[0])
        assert np.array_equal(r0.captureFrame()["data"], ref[1])
        # ... and after rt_dist_shutdown the context is a plain one again: all rows, presents its own accumulator
        r1.distShutdown()
        r1.distShutdown()
        assert r1.distBlockBytes() == 0
        r1.resetAccumulation()
        r1.computeBatch([21, 22])
        r1.sync()
        assert r1.readAccum()[..., 3].min() == 2.0, "after rt_dist_shutdown the context does not render every row"
    finally:
        r0.destroy()
        r1.destroy()


def test_bind_before_init_is_refused(W):
    """rt_dist_init on a context with an external accumulator: refused, the binding stays."""
    W._build.build_rt()
    a, b = new_context(W, "cornell", 64, 48), new_context(W, "cornell", 64, 48)
    try:
        a.bindAccum(b.accumDevicePtr())
        with pytest.raises(W.RendererError, match="unbind"):
            a.distInit(0, 1, 8)
        a.bindAccum(0)
        a.distInit(0, 1, 8)
    finally:
        a.destroy()
        b.destroy()


def _run_children(tmp_path, mode, world):
    """One fresh process per rank (rank k on device k), each with a time limit of its own; a process that is still running
    when one has failed or timed out is killed."""
    id_file, out = str(tmp_path / "unique_id"), str(tmp_path / "img.npz")
    env = dict(os.environ)
    procs = [subprocess.Popen([sys.executable, CHILD, mode, str(k), str(world), str(k), id_file, out], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for k in range(world)]
    outs, codes = [], []
    try:
        for p in procs:
            try:
                text, _ = p.communicate(timeout=300)
            except subprocess.TimeoutExpired:
                p.kill()
                text, _ = p.communicate()
                text += "\n[killed after 300 s]"
            outs.append(text)
            codes.append(p.returncode)
            if p.returncode != 0:
                break
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    log = "\n".join("--- rank %d (exit %s)\n%s" % (k, codes[k], outs[k][-3000:]) for k in range(len(outs)))
    print(log)
    if 3 in codes:
        reason = [l for t in outs for l in t.splitlines() if l.startswith("RCCL_UNAVAILABLE:")]
        pytest.skip("RCCL could not be initialised here: %s" % (reason[0] if reason else log[-500:]))
    assert codes == [0] * world, log
    z = np.load(out)
    return [(z["acc%d" % k], z["rgba%d" % k]) for k in range(2)], outs


def _child_reference(W):
    import native_gather_child as c
    assert (c.DEPTH, c.FRAMES_A, c.FRAMES_B, c.BATCH) == (DEPTH, FRAMES_A, FRAMES_B, BATCH)
    return single_context_moments(W, "cornell", c.W_, c.H_)


@pytest.mark.parametrize("mode", ["notorch", "torch"])
def test_rccl_gather_with_one_rank_equals_the_plain_render(W, tmp_path, mode):
    """rt_dist_unique_id -> rt_dist_init(0, 1, id) -> render -> rt_gather_stripes -> present, twice, in a fresh process: one
    that never imports torch (the system's librccl is loaded) and one that has (PyTorch's mapped copy is taken)."""
    W._build.build_rt()
    got, outs = _run_children(tmp_path, mode, 1)
    assert ("torch_loaded=%d" % (mode == "torch")) in outs[0]
    ref = _child_reference(W)
    for k in range(2):
        assert same_bits(got[k][0], ref[k][0]), "assembled image %d differs" % k
        assert np.array_equal(got[k][1], ref[k][1]), "RGBA8 output %d differs" % k


def test_rccl_gather_of_two_ranks_on_two_gpus_equals_the_single_gpu_image(W, tmp_path):
    """One process per GPU, the unique id passed through a file, the blocks over RCCL."""
    W._build.build_rt()
    from webgpu_raytracer_amd import renderer
    if renderer.load_library().rt_device_count() < 2:
        pytest.skip("needs two GPUs (RCCL refuses two ranks on one device)")
    got, _ = _run_children(tmp_path, "notorch", 2)
    ref = _child_reference(W)
    for k in range(2):
        assert same_bits(got[k][0], ref[k][0]), "assembled image %d differs" % k
        assert np.array_equal(got[k][1], ref[k][1]), "RGBA8 output %d differs" % k
