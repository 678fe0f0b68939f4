"""The reference model of the lightmap bakes (tests/model/bake_model.cpp, the texel rule of include/mi355rt.h restated in
f32) against an independent float64 numpy brute force that is texel-centric over all triangles, and against hand-worked
answers.  No GPU needed.

Owner maps must agree on every texel whose float64 distance to the nearest edge (segment) of any triangle of the instance is
>= MARGIN texel; nearer texels are exempt, and at most 1 % of the atlas may be exempt.

Tolerances of the point checks, per owner triangle, with u = 2^-23 (the spacing of f32 at 1), M the largest texel-space
coordinate difference among a, b, c and p, and A the (float64) doubled area:
  weights   8 u M^2 / |A|: an edge value is two differences, two products and one difference (three roundings of terms of
            size <= M^2 on top of the rounded inputs), then the division, then 1 - bu - bv.
  position  that times |V0| + |V1| + |V2| (the lengths of the world-space vertices), plus 4 ulp: four spacings of f32 at the
            largest coordinate of those vertices.
  uv        the same bound on the texel-space vertices: weight tolerance times (|a| + |b| + |c|) plus 4 ulp at their
            largest coordinate."""
import subprocess

import numpy as np
import pytest

import bake_util as bu
import model_build
import random_scene

MARGIN = 1e-4
U = 2.0 ** -23
SIZES = ((64, 64), (37, 19))


@pytest.fixture(scope="module")
def scenes(W):
    out = {}
    for seed in (1, 2, 3):
        b = random_scene.make(seed)
        out[seed] = (b, bu.model_for(W, b))
    return out


def arrays(bridge):
    topo = np.asarray(bridge.mesh_topology, np.uint32).reshape(-1, 20)
    pos = np.asarray(bridge.vertices, np.float32).reshape(-1, 4)
    nrm = np.asarray(bridge.normals, np.float32).reshape(-1, 4)
    inst = np.asarray(bridge.instances, np.float32).reshape(-1, 36)
    return topo, pos, nrm, inst


def edge(q, r, s):
    return (r[..., 0] - q[..., 0]) * (s[..., 1] - q[..., 1]) - (r[..., 1] - q[..., 1]) * (s[..., 0] - q[..., 0])


def seg_dist(p, q, r):
    """distance of the points p (n, 2) to the segment q r"""
    d = r - q
    L = float(d @ d)
    t = np.clip(((p - q) @ d) / L, 0.0, 1.0) if L > 0 else np.zeros(len(p))
    return np.linalg.norm(p - (q + t[:, None] * d), axis=1)


def brute_force(bridge, inst, width, height, uv):
    """float64, texel-centric: (owner (H, W) i64, distance of every centre to the nearest edge of any triangle (H, W),
    texel-space triangles {k: (a, b, c)})"""
    first, count = bu.instance_triangles(bridge, inst)
    topo = arrays(bridge)[0]
    xs, ys = np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5)
    p = np.stack([xs.ravel(), ys.ravel()], axis=1)
    owner = np.full(len(p), -1, np.int64)
    dist = np.full(len(p), np.inf)
    tris = {}
    scale = np.array([width, height], np.float64)
    for k in range(first, min(first + count, len(topo))):
        a, b, c = (uv[topo[k, j]].astype(np.float64) * scale for j in range(3))
        if not np.isfinite([a, b, c]).all():
            continue
        tris[k] = (a, b, c)
        for q, r in ((a, b), (b, c), (c, a)):
            dist = np.minimum(dist, seg_dist(p, q, r))
        A = edge(a, b, c)
        if A == 0:
            continue
        sg = 1.0 if A > 0 else -1.0
        inside = (sg * edge(a, b, p) >= 0) & (sg * edge(b, c, p) >= 0) & (sg * edge(c, a, p) >= 0)
        owner[(owner < 0) & inside] = k
    return owner.reshape(height, width), dist.reshape(height, width), tris


def check_owner(model_owner, owner64, dist):
    far = dist >= MARGIN
    assert (~far).sum() <= 0.01 * far.size, ("texels under the margin", int((~far).sum()), far.size)
    differ = model_owner != owner64
    assert not (differ & far).any(), ("owner maps differ away from every edge", np.argwhere(differ & far)[:8].tolist())
    return int(differ.sum()), int((~far).sum())


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_owner_map_and_points_against_float64(scenes, seed, size):
    bridge, model = scenes[seed]
    width, height = size
    topo, pos, nrm, inst_rows = arrays(bridge)
    uv = np.asarray(bridge.uvs, np.float32).reshape(-1, 2)
    for inst in range(len(inst_rows)):
        points, texels, owner, wts = model.bakePoints(inst, width, height, t_max=3.0, pad_base=11, weights=True)
        owner64, dist, tris = brute_force(bridge, inst, width, height, uv)
        print(seed, size, inst, "differing / under the margin:", check_owner(owner, owner64, dist), "covered", len(texels))
        # the output: ascending texel order, the covered texels, pads and t_max
        assert np.array_equal(texels, np.flatnonzero(owner.ravel() >= 0))
        assert np.array_equal(points.view(np.uint32)[:, 7], 11 + texels)
        assert (points[:, 3] == np.float32(3.0)).all()
        m = inst_rows[inst, 0:16].reshape(4, 4).T.astype(np.float64)   # column-major
        worst = 0.0
        for j, t in enumerate(texels.tolist()):
            k = int(owner.ravel()[t])
            if k != owner64.ravel()[t]:
                continue
            a, b, c = tris[k]
            p = np.array([t % width + 0.5, t // width + 0.5])
            A = edge(a, b, c)
            w64 = np.array([edge(c, a, p) / A, edge(a, b, p) / A])
            M = np.abs(np.array([b - a, c - a, c - b, p - a, p - b, p - c])).max()
            tol_w = 8 * U * M * M / abs(A)
            assert np.abs(wts[j].astype(np.float64) - w64).max() <= tol_w, (inst, t, k, wts[j], w64, tol_w)
            w3 = np.array([1.0 - w64[0] - w64[1], w64[0], w64[1]])
            v = pos[topo[k, 0:3], 0:3].astype(np.float64)
            V = v @ m[:3, :3].T + m[:3, 3]
            tol_p = tol_w * np.linalg.norm(V, axis=1).sum() + 4 * float(np.spacing(np.float32(np.abs(V).max())))
            err = np.abs(points[j, 0:3] - w3 @ V).max()
            worst = max(worst, err / tol_p)
            assert err <= tol_p, (inst, t, k, err, tol_p)
            # the uv the model's own weights reconstruct is the texel centre
            g = wts[j].astype(np.float64)
            rec = (1.0 - g[0] - g[1]) * a + g[0] * b + g[1] * c
            tol_uv = tol_w * (np.linalg.norm(a) + np.linalg.norm(b) + np.linalg.norm(c)) + \
                4 * float(np.spacing(np.float32(np.abs([a, b, c]).max())))
            assert np.abs(rec - p).max() <= tol_uv, (inst, t, k, rec, p, tol_uv)
        print("  largest position error / tolerance %.3f" % worst)
        norms = np.linalg.norm(points[:, 4:7].astype(np.float64), axis=1)
        assert np.abs(norms - 1.0).max() <= 4 * U if len(norms) else True


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_grid_layout_has_many_owners_and_gaps(scenes, seed):
    bridge, model = scenes[seed]
    for inst in range(len(arrays(bridge)[3])):
        uv = bu.grid_uv(bridge, inst)
        first, count = bu.instance_triangles(bridge, inst)
        for width, height in SIZES:
            points, texels, owner = model.bakePoints(inst, width, height, atlas_uv=uv)
            owner64, dist, _ = brute_force(bridge, inst, width, height, uv)
            check_owner(owner, owner64, dist)
            assert (owner < 0).mean() >= 0.2
            owners = np.unique(owner[owner >= 0])
            assert len(owners) >= 0.9 * count, (width, height, len(owners), count)
            assert owners.min() >= first and owners.max() < first + count


# ---- hand-worked cases (bake_util.hand_cases: the answers are written out there)
@pytest.mark.parametrize("name", sorted(bu.hand_cases()))
def test_hand_worked_cases(scenes, name):
    bridge, model = scenes[1]
    tri_uvs, width, height, want = bu.hand_cases()[name]
    first, _ = bu.instance_triangles(bridge, 0)
    want = np.asarray(want)
    want = np.where(want >= 0, want + first, -1)
    points, texels, owner = model.bakePoints(0, width, height, t_max=2.0, pad_base=5, atlas_uv=bu.hand_uv(bridge, 0, tri_uvs))
    assert owner.tolist() == want.tolist()
    assert np.array_equal(texels, np.flatnonzero(want.ravel() >= 0))
    assert np.array_equal(points.view(np.uint32)[:, 7], 5 + texels)
    assert (points[:, 3] == np.float32(2.0)).all()


def test_stand_alone_cases_under_the_sanitizers(tmp_path):
    """the model's own main (hand-worked cases on the restated rule) built with ASan and UBSan, on the CPU"""
    exe = str(tmp_path / "bake_model_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DBAKE_MODEL_MAIN"]
    model_build.build(bu.SRC, exe, [f for f in bu.ru.FLAGS if f not in ("-fPIC", "-O2")] + flags, program=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hand-worked cases ok" in r.stdout
