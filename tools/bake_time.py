"""Stream time of the lightmap point pass (rt_bake_points_device) beside the gather it feeds, from one process.

Per scene (cornell, sponza_like): the instance that owns most triangles, a 1024 x 1024 atlas, and an override UV layout that
packs one triangle per cell of a ceil(sqrt(n)) grid (the triangle (0.11, 0.13) (0.89, 0.12) (0.12, 0.87) of its cell: 0.3 of
every used cell is covered).  An override layout is per vertex, and these meshes are indexed, so the tool first gives every
triangle corner a vertex of its own (positions, normals and uvs duplicated, topology rows renumbered; triangle order and BVH
untouched) - otherwise a shared vertex would stretch its triangles across cells.  For cornell also the scene's own uvs, where
every quad spans the whole atlas (36 triangles, each over half of it: the worst case for the owner pass).
  points   one rt_bake_points_device call with every output: owner pass, counts, scan, emit
  front    the same with cap = 0: owner pass, counts and scan only (emit = points - front)
  gather   rt_gather_irradiance_device on the points just made, depth 4, spp 16
  bake     points + gather of the same round: what a caller who chains the two sees
All on a torch side stream the context was given (rt_set_stream), timed with device events around each call; one warm-up,
5 rounds, every figure the median with (min .. max).  Nothing is gated on these numbers.
--atlas-form times the same bakes through rt_bake_atlas_points_device with the one whole-atlas entry {inst, 0, 0, W, H}, which
puts the entry staging, the item counts and their scan in front of the owner pass and runs every launch on the u64 owner map.

usage: python tools/bake_time.py [--out profiles/bake_rate.txt] [--scenes cornell,sponza_like] [--atlas-form]"""
import argparse
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import webgpu_raytracer_amd as W  # noqa: E402
from timing_util import fmt  # noqa: E402

SIZE, DEPTH, SPP, ROUNDS, SEED = 1024, 4, 16, 5, 5


def unindexed(bridge):
    """(vertices, normals, uvs, topology) with a vertex of its own for every triangle corner: vertex 3 k + j is corner j of
    triangle k"""
    topo = np.asarray(bridge.mesh_topology, np.uint32).reshape(-1, 20).copy()
    idx = topo[:, 0:3].reshape(-1)
    v = np.asarray(bridge.vertices, np.float32).reshape(-1, 4)[idx]
    n = np.asarray(bridge.normals, np.float32).reshape(-1, 4)[idx]
    uv = np.asarray(bridge.uvs, np.float32).reshape(-1, 2)[idx]
    topo[:, 0:3] = np.arange(len(idx), dtype=np.uint32).reshape(-1, 3)
    return (np.ascontiguousarray(a).reshape(-1) for a in (v, n, uv, topo))


def grid_uv(bridge, inst, topology):
    """one triangle of the instance per grid cell (the mesh has no shared vertices); vertices it does not use at (-1, -1)"""
    dc = np.asarray(bridge.draw_commands, np.uint32).reshape(-1, 4)[inst]
    first, count = int(dc[2]) // 3, int(dc[0]) // 3
    topo = topology.reshape(-1, 20)[first:first + count, 0:3]
    uv = np.full((topology.size // 20 * 3, 2), -1.0, np.float32)
    g = max(1, math.ceil(math.sqrt(max(count, 1))))
    j = np.arange(len(topo))
    cell = np.stack([j % g, j // g], axis=1).astype(np.float64)
    for k, corner in enumerate(((0.11, 0.13), (0.89, 0.12), (0.12, 0.87))):
        uv[topo[:, k]] = ((cell + np.array(corner)) / g).astype(np.float32)
    return uv


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", default="cornell,sponza_like")
    ap.add_argument("--atlas-form", action="store_true", help="bakeAtlasPointsDevice with one whole-atlas entry")
    args = ap.parse_args()
    texels = SIZE * SIZE
    lines = ["lightmap bake%s, %d x %d atlas; gather at depth %d, spp %d; Mtexels/s = 1e-6 * atlas texels / seconds of the point pass"
             % (" as a one-entry atlas bake" if args.atlas_form else "", SIZE, SIZE, DEPTH, SPP)]
    for scene in args.scenes.split(","):
        b = W.WorldBridge()
        b.loadScene(scene)
        r = W.WebGPURenderer(0)
        W.upload_scene(r, b, 16, 16)
        vertices, normals, uvs, topology = unindexed(b)
        r.updateCombinedGeometry(vertices, normals, uvs)
        r.updateBuffer("topology", topology)
        dc = np.asarray(b.draw_commands, np.uint32).reshape(-1, 4)
        inst = int(np.argmax(dc[:, 0]))
        layouts = [("grid layout", grid_uv(b, inst, topology))] + ([("scene uvs", None)] if scene == "cornell" else [])
        side = torch.cuda.Stream()
        r.setStream(side.cuda_stream)
        with torch.cuda.stream(side):
            d_points = torch.zeros((texels, 8), dtype=torch.float32, device="cuda")
            d_texels = torch.zeros(texels, dtype=torch.int32, device="cuda")
            d_count = torch.zeros(4, dtype=torch.int32, device="cuda")
            d_out = torch.zeros((texels, 4), dtype=torch.float32, device="cuda")

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side)
                fn()
                e1.record(side)
                e1.synchronize()
                return e0.elapsed_time(e1)

            for name, uv in layouts:
                d_uv = None if uv is None else torch.from_numpy(uv).cuda()
                uv_ptr = None if uv is None else d_uv.data_ptr()

                def point_pass(points_ptr, texels_ptr, cap):
                    if args.atlas_form:
                        r.bakeAtlasPointsDevice([(inst, 0, 0, SIZE, SIZE)], SIZE, SIZE, points_ptr, texels_ptr, cap,
                                                d_count.data_ptr(), atlas_uv_ptr=uv_ptr)
                    else:
                        r.bakePointsDevice(inst, SIZE, SIZE, points_ptr, texels_ptr, cap, d_count.data_ptr(), atlas_uv_ptr=uv_ptr)

                def points():
                    point_pass(d_points.data_ptr(), d_texels.data_ptr(), texels)

                def front():
                    point_pass(None, None, 0)

                timed(points)
                n = int(d_count[0])

                def gather():
                    r.gatherIrradianceDevice(d_points.data_ptr(), n, d_out.data_ptr(), DEPTH, SPP, SEED)

                timed(front)
                timed(gather)
                ms = {"points": [], "front": [], "gather": []}
                for _ in range(ROUNDS):
                    ms["points"].append(timed(points))
                    ms["front"].append(timed(front))
                    ms["gather"].append(timed(gather))
                p, f, g = (statistics.median(ms[k]) for k in ("points", "front", "gather"))
                lines.append("%s, instance %d (%d triangles), %s: %d of %d texels covered" % (scene, inst, int(dc[inst, 0]) // 3, name, n, texels))
                lines.append("  points (%s)          %s; %s" % ("items .. emit" if args.atlas_form else "owner .. emit", fmt(ms["points"]), fmt([texels / (v * 1e-3) * 1e-6 for v in ms["points"]], "Mtexels/s")))
                lines.append("  front (points without emit)     %s; emit = points - front = %.3f ms" % (fmt(ms["front"]), p - f))
                lines.append("  gather on those points          %s; the point pass is %.1f %% of points + gather" % (fmt(ms["gather"]), 100.0 * p / (p + g)))
                lines.append("  bake (points + gather, a round) %s" % fmt([a + b for a, b in zip(ms["points"], ms["gather"])]))
        r.setStream(None)
        r.destroy()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
