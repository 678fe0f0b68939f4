"""One rank of a sharded image in a fresh process, gathered by rt_gather_stripes (RCCL) — started by
tests/test_gpu_native_gather.py, never collected by pytest.

usage: native_gather_child.py <torch|notorch> <rank> <world> <device> <id_file> <out.npz>

Rank 0 makes the unique id and writes it to <id_file> (written under another name and renamed, so a reader never sees half
of it); the other ranks wait for the file.  Exit codes: 0 = done (rank 0 wrote <out.npz>), 3 = RCCL could not be
initialised (the reason is printed after "RCCL_UNAVAILABLE:"), anything else = failure."""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

W_, H_, DEPTH, STRIPE, FRAMES_A, FRAMES_B, BATCH = 160, 96, 6, 8, tuple(range(1, 9)), tuple(range(9, 13)), 4


def main():
    mode, rank, world, device, id_file, out_path = sys.argv[1:7]
    rank, world, device = int(rank), int(world), int(device)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC for RCCL across processes, as bench.py sets for its ranks
    if mode == "torch":
        import torch   # maps PyTorch's own librccl and HIP runtime before the renderer library is loaded
        torch.zeros(1, device="cuda:%d" % device).sum().item()
    import numpy as np
    import webgpu_raytracer_amd as pkg
    from webgpu_raytracer_amd import renderer
    from webgpu_raytracer_amd.distributed import NativeShardedImage
    if mode != "torch":
        assert "torch" not in sys.modules, "the torch-free branch imported torch"

    try:
        if rank == 0:
            uid = renderer.dist_unique_id()
            with open(id_file + ".tmp", "wb") as f:
                f.write(uid)
            os.replace(id_file + ".tmp", id_file)
        else:
            deadline = time.time() + 120
            while not os.path.exists(id_file):
                if time.time() > deadline:
                    raise SystemExit("rank %d: no unique id file after 120 s" % rank)
                time.sleep(0.05)
            uid = open(id_file, "rb").read()
    except pkg.RendererError as e:
        print("RCCL_UNAVAILABLE: %s" % e)
        return 3

    bridge = pkg.WorldBridge()
    bridge.loadScene("cornell")
    r = pkg.WebGPURenderer(device)
    r.buildPipeline(DEPTH, 1)
    pkg.upload_scene(r, bridge, W_, H_)
    try:
        shard = NativeShardedImage(r, rank, world, STRIPE, unique_id=uid)
    except pkg.RendererError as e:
        if "(-6)" in str(e):   # RT_ERR_RCCL: the library or ncclCommInitRank
            print("RCCL_UNAVAILABLE: %s" % e)
            return 3
        raise
    rows = shard.owned_rows(H_)
    out = {}
    for k, frames in enumerate((FRAMES_A, FRAMES_B)):
        shard.render(frames, batch=BATCH)
        shard.gather(present=True)
        shard.synchronize()
        assert not r.readAccum()[~rows].any(), "rank wrote outside its stripes (or the gather touched the accumulator)"
        if rank == 0:
            out["acc%d" % k] = shard.read_image()
            out["rgba%d" % k] = r.captureFrame()["data"].copy()
    if rank == 0:
        np.savez(out_path, **out)
    print("RCCL_FILE_OK rank %d torch_loaded=%d" % (rank, int("torch" in sys.modules)))
    r.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
