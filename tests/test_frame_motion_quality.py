"""The quality gate of frame motion on the CPU oracle and the model (no GPU): tests/random_scene.py's multi-instance scene at
64 x 64, eight frames of 1 spp with the accumulation reset every frame, one instance translated by about a third of a pixel per
frame (its TLAS rebuilt around it, so the instance array is re-sorted as it goes); the clean image is 512 spp at the last pose.
Over the pixels that show the moving instance in the last frame, the pre-filter integrated image of the motion rule is closer to
the clean image than the static rule's.

Measured, rgb RMSE over the 119 pixels of the moving instance: the raw frame 0.6594, the static rule 0.5805, the motion rule
0.3819 (52 pixels carry all eight frames, against 27).  With normal_cos = 0.9 on this scene's random normals the motion rule
accepts almost nothing (93 of 119 pixels at n = 1) and gives 0.5561 against the static rule's 0.5311: the limitation, not the
gate's case.  DESIGN.md 4.3d has both."""
import numpy as np

import frame_denoise_util as fu
import frame_motion_util as mu
import frame_temporal_util as tu
import random_scene as rs

SIZE, FRAMES, CLEAN_SPP, DEPTH = 64, 8, 512, 4
# normal_cos = -1: random_scene gives every vertex a RANDOM unit normal, so the shading normals of this scene say nothing about
# its surfaces, and the motion rule compares the previous triangle's GEOMETRIC normal with the previous frame's shading normal
# (the limitation the header states: normal_cos has to tolerate the angle between the two).  Both rules get the same descriptor;
# the plane test is what separates surfaces here.
T = dict(flags=0, max_history=32, var_history=4, normal_cos=-1.0, plane_eps=0.02)
D = dict(fu.CORNELL, flags=0)          # no demodulation: the integrated image is radiance, as the clean image is


def test_the_integrated_image_of_a_moving_instance_is_closer_to_the_clean_one(W, oracle_lib):
    b0 = rs.make(11, n_geoms=3, tris_per_geom=40, n_instances=6)
    o = oracle_lib.OracleRenderer()
    o.buildPipeline(DEPTH, 1)
    W.upload_scene(o, b0, SIZE, SIZE)
    o.compute(1)
    inst0 = fu.words(o.readGBuffer()[1][..., 3])[(np.ascontiguousarray(o.readGBuffer()[0]).view(np.uint32).reshape(SIZE, SIZE) >> 24) != 0]
    which = int(np.bincount(inst0).argmax())           # the instance that fills most of the view moves
    cam = np.asarray(b0.cameraData, np.float64)
    depth = np.asarray(b0.instances, np.float32).reshape(-1, 36)[which, 14] - cam[2]
    pixel = np.linalg.norm(cam[8:11]) / SIZE * depth / 3.0   # world width of a pixel at the instance (the image plane is 3 ahead)
    step = cam[8:11] / np.linalg.norm(cam[8:11]) * pixel / 3.0
    st_m, st_s = mu.History(), tu.History()
    for k in range(FRAMES):
        b, ids = mu.moved_random_scene(b0, which, step * k)
        mu.upload_frame(W, o, b, ids, SIZE, SIZE, k == 0)
        o.compute(k + 1)
        fr = fu.frame_of(o.readAccum(), o.readGBuffer(), o.readUniforms())
        _, integ_m, _, c = mu.call(fr, mu.scene_of(b, ids), D, dict(T, flags=mu.MOTION), st_m)
        _, integ_s, _ = tu.call(fr, D, T, st_s)
    moving = (fu.words(c[..., 7]) == which) & (fu.words(st_m.guide[..., 7]) != 0)
    clean = oracle_lib.OracleRenderer()
    clean.buildPipeline(DEPTH, 64)
    W.upload_scene(clean, b, SIZE, SIZE)
    for f in range(CLEAN_SPP // 64):
        clean.compute(f + 1)
    a = clean.readAccum()
    ref = a[..., :3] / a[..., 3:4]
    r_m, r_s = fu.rmse(integ_m[moving, :3], ref[moving]), fu.rmse(integ_s[moving, :3], ref[moving])
    r_1 = fu.rmse(fr.radiance()[moving], ref[moving])
    print("quality gate: %d pixels of the moving instance; rmse raw %.4f, static %.4f, motion %.4f; moved %d; n motion %s, n static %s"
          % (moving.sum(), r_1, r_s, r_m, (mu.status(c)[moving] == mu.MOVED).sum(), np.bincount(st_m.n()[moving].astype(int)).tolist(),
             np.bincount(st_s.n()[moving].astype(int)).tolist()))
    assert moving.sum() >= 100
    assert r_m < r_s
