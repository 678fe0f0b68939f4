#!/usr/bin/env python3
"""Device-memory leak check: 40 create / upload / render / GPU-BLAS-build / destroy cycles, free memory must not drift.
Every cycle the context is also a rank of a sharded image (rt_dist_init: blocks, display buffer, a resize, on every tenth
cycle an RCCL communicator of one rank), freed by rt_dist_shutdown on odd cycles and by rt_destroy alone on even ones.
Every cycle also runs one call each of the families that keep the most state of their own - a ray query, a probe gather, a
lightmap, a directional lightmap and a volume bake, with kernel timing on so that their events exist."""
import sys, ctypes
import os; R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import webgpu_raytracer_amd as W
hip = ctypes.CDLL("libamdhip64.so")
def free_mb():
    f, t = ctypes.c_size_t(), ctypes.c_size_t()
    hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t))
    return f.value / 2**20
b = W.WorldBridge(); b.loadScene("sponza_like")
r0 = W.WebGPURenderer(0); base = free_mb(); r0.destroy()
vals, warm = [], []
rays = np.zeros((4, 8), np.float32); rays[:, 1] = 1.0; rays[:, 3] = 1e30; rays[:, 4] = [1, -1, 0, 0]; rays[:, 6] = [0, 0, 1, -1]
filt = dict(plane_eps=0.02, max_dist=0.5, passes=1, step=1)
# 20 unmeasured cycles first: RCCL keeps some device memory for the life of the process once communicators have existed
# (observed: 240 MB less free after the second one, flat from there on), which is no leak of a context
for i in range(-20, 40):
    r = W.WebGPURenderer(0)
    r.buildPipeline(6, 1)
    W.upload_scene(r, b, 320, 180)
    r.computeBatch([1, 2, 3, 4]); r.compute(5); r.present(); r.captureFrame()
    b.setBlasBuilder(r); b.update(0.0); b.setBlasBuilder(None)
    r.setKernelTiming(True)
    r.traceRays(rays, stats=True); r.gatherProbes(rays, 2, 2, stats=True)
    r.bakeAtlasLightmap([(0, 0, 0, 8, 8)], 8, 8, 2, 2, denoise=filt, dilate=1, stats=True)
    r.bakeAtlasDirectionalLightmap([(0, 0, 0, 8, 8)], 8, 8, 2, 2, denoise=filt, dilate=1, stats=True)
    r.bakeVolume(W.renderer.volume_desc((-1, 0.5, -1), (2, 1, 2), (2, 2, 2)), 2, 2, stats=True)
    r.setKernelTiming(False)
    uid = None
    if i % 10 == 5:
        try: uid = W.renderer.dist_unique_id()
        except W.RendererError as e: print("no RCCL communicator in this cycle:", e)
    r.distInit(0, 1 if uid else 2, 8, uid)
    r.compute(6)
    if uid: r.gatherStripes()
    else: r.packStripes(); r.writeBlock(0, r.readBlock()); r.writeBlock(1, r.readBlock()); r.unpackStripes()
    r.updateScreenSize(400, 240); r.packStripes(); r.sync()
    if i % 2: r.distShutdown()
    r.destroy()
    if i % 10 == 9: (vals if i >= 0 else warm).append(free_mb())
print("free MB after every 10 create/destroy cycles:", [round(v) for v in vals], "baseline", round(base), "warm-up", [round(v) for v in warm])
assert abs(vals[-1] - vals[0]) < 64, "device memory is leaking"
print("no leak")
