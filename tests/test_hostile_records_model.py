"""Hostile triangle records (tests/hostile_records.py) on the CPU: the oracle and the radiance / gather models finish every
family, the pictures are not one NaN (at least half of the pixels of every family's picture are finite and lit), and every
hostile triangle is shaded at depth 0 by a centroid ray of the query set - so the GPU tests that compare with these models
(tests/test_gpu_hostile_records.py) compare something.  The radiance model is also built as a stand-alone program under
ASan, UBSan and the float-cast-overflow check and run on every family: the conversions and index arithmetic that shading does
on these words must be defined behaviour, since the kernels restate them."""
import os
import subprocess

import numpy as np
import pytest

import gather_util as gu
import hostile_records as hr
import model_build
import parity_util as pu
import radiance_util as ru

SIZES = ((37, 29), (24, 16))
DEPTH, FRAMES = 8, (1, 2, 3)
QUERY = (8, 2)            # (max_depth, spp) of the radiance queries
GATHER = (4, 2)


@pytest.mark.parametrize("scene", sorted(hr.SCENES))
def test_the_query_set_reaches_the_scene(W, oracle_lib, scene):
    p = hr.prepared(scene)
    n_tris = len(p.bridge.mesh_topology) // 20
    reached = len(set(p.ray_tri.tolist()))
    print(scene, "triangles", n_tris, "reached by a centroid ray", reached, "rays", len(p.rays),
          "may carry a hostile field", len(p.order), "their fewest pixels", sorted(p.pixels.values()))
    assert 2 * reached >= n_tris
    # every edit of every family finds a triangle of its own in the picture (of the texture words: every value)
    assert len(p.order) >= max(len(e) for e in hr.FAMILIES.values() if e)
    if scene == "one_leaf":
        assert pu.takes_wide_form(p.bridge)
    assert pu.dyn_lds(p.bridge) <= 64 * 1024, "the scene fits the forms that hold it in LDS"


@pytest.mark.parametrize("name", hr.NAMES)
@pytest.mark.parametrize("scene", sorted(hr.SCENES))
def test_the_models_finish_and_the_pictures_show_something(W, oracle_lib, scene, name):
    p = hr.prepared(scene)
    b, hostile = p.family(name)
    topo = hr.topology(b)
    if name == "plain_preserving":
        assert hr.is_plain(topo).all()
    for w, h in SIZES:
        # every hostile triangle is a depth-0 hit of every frame: what every frame form of the GPU tests shades
        cpu, per_frame = hr.frame_triangles(b, w, h, DEPTH, FRAMES)
        pixels = [min(f.get(t, 0) for f in per_frame) for t in hostile.tolist()]
        share = hr.good_share(cpu.readAccum())
        print("%s %s %dx%d finite and lit %.3f, fewest depth-0 pixels of each hostile triangle %s" % (scene, name, w, h, share, pixels))
        assert min(pixels) >= 1, (scene, name, w, h, hostile.tolist(), pixels)
        assert share >= 0.5, (scene, name, w, h, share)
    m = gu.model_for(W, b)
    out, counts = m.traceRadiance(p.rays, *QUERY, ru.SEED)
    res, hits, _ = m.gatherIrradiance(p.points, *GATHER, gu.SEED)
    print("%s %s radiance records with a NaN %d of %d, gather records %d of %d" % (
        scene, name, np.isnan(out).any(axis=1).sum(), len(out), np.isnan(res).any(axis=1).sum(), len(res)))
    # every hostile triangle is the first hit of a ray of the query set, and that ray shades it
    tri, _ = hr.first_hits(m, p.rays)
    assert np.array_equal(tri, p.ray_tri), "a hostile field moved a first hit"
    for t in hostile.tolist():
        own = np.flatnonzero(tri == t)
        assert own.size and (counts[own, 2] >= QUERY[1]).all(), (scene, name, t)


def _write(path, b, rays):
    os.makedirs(path)
    for fname, a, dt in (("vertices.f32", b.vertices, np.float32), ("normals.f32", b.normals, np.float32), ("uvs.f32", b.uvs, np.float32),
                         ("topology.u32", b.mesh_topology, np.uint32), ("tlas.f32", b.tlas, np.float32), ("blas.f32", b.blas, np.float32),
                         ("instances.f32", b.instances, np.float32), ("lights.u32", b.lights, np.uint32),
                         ("draw_commands.u32", b.draw_commands, np.uint32), ("camera.f32", b.cameraData, np.float32),
                         ("rays.f32", rays, np.float32)):
        np.ascontiguousarray(a, dt).tofile(os.path.join(path, fname))


def test_stand_alone_model_under_the_sanitizers(W, oracle_lib, tmp_path):
    """the radiance model's own main (frames 1-3 and a radiance query per family) built with ASan, UBSan and
    float-cast-overflow, on the CPU, on every family of both scenes"""
    exe = str(tmp_path / "radiance_model_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-DRADIANCE_MODEL_MAIN"]
    model_build.build(ru.SRC, exe, [f for f in ru.FLAGS if f not in ("-fPIC", "-O2")] + flags, program=True)
    for scene in sorted(hr.SCENES):
        p = hr.prepared(scene)
        tex = str(tmp_path / (scene + ".textures.u8"))
        np.ascontiguousarray(np.stack(p.bridge.textures), np.uint8).tofile(tex)
        dirs = []
        for name in hr.NAMES:
            b, _ = p.family(name)
            dirs.append(str(tmp_path / scene / name))
            _write(dirs[-1], b, p.rays)
        r = subprocess.run([exe, tex, "37", "29", str(DEPTH)] + dirs, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
        assert "hostile records ok" in r.stdout
