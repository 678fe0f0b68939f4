"""k_primary_visibility (csrc/k_prepare_primary.hip.h) once its walk keeps u and v of the accepted triangle test for the
surface block (trace_closest_uv, csrc/k_intersect.hip.h; every form), and once the LDS form of an unstriped dispatch of a
one-leaf scene stages the scene once per workgroup and casts `rounds` tiles per wave, with the camera constants, the TLAS
leaf and its instance rows read once per wave and the counters flushed once per wave (k_primary_visibility_tiles).

Everything stays bit for bit what the oracle computes: the three G-buffer planes, the accumulation buffer and the counters
(all six in the counting build, the three ray counters in the product build), for one frame per dispatch and batches of 2
and 4.  MI355RT_PRIMARY_ROUNDS, read once when a context is made, forces `rounds` to 1, 2, 3 and 16, so that images of a few
tiles run the loop, its partial last round and its idle waves; "auto" is what the planner chooses (1 at these sizes, and
with one round the form of one tile per wave runs).  Each launch says on stderr (MI355RT_DEBUG_SHAPE) which form it took,
with how many rounds and in what grid, and the test holds it to that.

Cornell: 8x8 (one tile, three idle waves), 5x3 (a partial tile), 9x9 (four tiles), 37x29 (20 tiles: not a multiple of
4 * rounds, the last workgroup has a partial round), 72x8 (9 tiles: a workgroup with one live wave in its last round), and
a view that sees background alone.  A striped rank in both stripe forms (tile-aligned, and per row, which cuts inside
tiles), the two-instance viewer_diamond (the TLAS walk; normals transformed per pixel) and a scene too large for LDS take
the forms of one tile per wave, whatever the knob says.  A textured instance under a rotation and a non-uniform scale
interpolates texture coordinates and normals with the kept u and v."""
import numpy as np
import pytest

import parity_util as pu
from test_gpu_background_tiles import _camera
from test_gpu_trip_surface import _textured

pytestmark = pytest.mark.gpu

FRAMES = (1, 2, 3, 4)
RAYS = pu.RAY_COUNTERS
SPP, DEPTH = 1, 2
# (scene, view, (w, h), stripes (rows, rank, count) or None)
CASES = [("cornell", "stock", (8, 8), None), ("cornell", "stock", (5, 3), None), ("cornell", "stock", (9, 9), None),
         ("cornell", "stock", (37, 29), None), ("cornell", "stock", (72, 8), None), ("cornell", "away", (37, 29), None),
         ("cornell", "stock", (37, 29), (8, 1, 3)), ("cornell", "stock", (37, 29), (1, 0, 2)),
         ("viewer_diamond", "stock", (9, 9), None), ("viewer_diamond", "stock", (40, 30), None),
         ("textured", "stock", (37, 29), None),
         ("viewer_diamond_1k", "stock", (37, 29), None)]   # 968 triangles: the global-memory form


def _case_id(c):
    scene, view, (w, h), st = c
    return "%s-%s-%dx%d-%s" % (scene, view, w, h, "x".join(map(str, st)) if st else "whole")


def _bridge(W, scene):
    return _textured(W) if scene == "textured" else pu.bridge_for(W, scene)


def _drive(r, W, b, case, batch, counting):
    scene, view, (w, h), stripes = case
    if stripes:
        r.setStripes(*stripes)
    r.buildPipeline(DEPTH, SPP)
    W.upload_scene(r, b, w, h)
    if view != "stock":
        r.updateSceneUniforms(_camera(b, view), 0, b.lightCount)
        r.resetAccumulation()
    if hasattr(r, "setCounting"):
        r.setCounting(counting)
    r.resetCounters()
    for i in range(0, len(FRAMES), batch):
        if batch == 1:
            r.compute(FRAMES[i])
        else:
            r.computeBatch(list(FRAMES[i:i + batch]))
    r.sync()


_oracle = {}   # case -> (accumulation buffer, G-buffer planes, counters): computed once, shared, left unchanged


def _reference(W, oracle_lib, case):
    key = _case_id(case)
    if key not in _oracle:
        scene, view, (w, h), stripes = case
        cpu = oracle_lib.OracleRenderer()
        _drive(cpu, W, _bridge(W, scene), case, 1, True)
        acc, gbuf = cpu.readAccum().copy(), [np.array(g).copy() for g in cpu.readGBuffer()]
        for a in [acc] + gbuf:
            a.setflags(write=False)
        bg = gbuf[2].reshape(h, w) >= 1.0
        if view == "away":
            assert bg.all()
        elif not stripes:
            assert not bg.all(), "the view sees nothing"
        _oracle[key] = (acc, gbuf, dict(cpu.getCounters()))
    return _oracle[key]


@pytest.mark.parametrize("rounds", [None, 1, 2, 3, 16], ids=["auto", "rounds1", "rounds2", "rounds3", "rounds16"])
@pytest.mark.parametrize("counting", [True, False], ids=["counting", "product"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_primary_tiles(W, oracle_lib, monkeypatch, capfd, case, counting, rounds):
    scene, view, (w, h), stripes = case
    want, gbuf, cc = _reference(W, oracle_lib, case)
    monkeypatch.setenv("MI355RT_DEBUG_SHAPE", "1")   # the launch says on stderr which form it took and how many rounds
    if scene == "viewer_diamond_1k":
        form, n_rounds = "global", 1
    elif scene == "viewer_diamond" or stripes:
        form, n_rounds = "LDS", 1
    else:
        n_rounds = rounds or 1
        form = "LDS many-tiles" if n_rounds > 1 else "LDS"
    tiles = -(-w // 8) * -(-h // 8) if not stripes else None
    if rounds is None:
        monkeypatch.delenv("MI355RT_PRIMARY_ROUNDS", raising=False)
    else:
        monkeypatch.setenv("MI355RT_PRIMARY_ROUNDS", str(rounds))
    owned = np.ones(h, bool)
    if stripes:
        rows, rank, count = stripes
        owned = (np.arange(h) // rows) % count == rank
    for batch in (1, 2, 4):
        r = W.WebGPURenderer(0)   # reads the knob
        try:
            capfd.readouterr()
            _drive(r, W, _bridge(W, scene), case, batch, counting)
            what = "batch of %d" % batch
            said = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[mi355rt] primary kernel:")]
            assert len(said) == len(FRAMES) // batch, said
            for line in said:
                assert "primary kernel: %s form, %d rounds, " % (form, n_rounds) in line, line
                if tiles:
                    per_wg = n_rounds * (1 if form == "global" else 4)
                    assert "grid %d x %d," % (-(-tiles // per_wg), batch) in line, line
            gc = r.getCounters()
            if counting:
                assert gc == cc, what
            else:
                assert {k: gc[k] for k in RAYS} == {k: cc[k] for k in RAYS}, what
            for name, g, c in zip(("albedo", "normal_id", "depth"), r.readGBuffer(), gbuf):
                g, c = np.asarray(g).reshape(h, w, -1)[owned], np.asarray(c).reshape(h, w, -1)[owned]
                assert np.array_equal(pu.bits(g), pu.bits(c)), pu.describe_mismatch("G-buffer %s, %s" % (name, what), g, c)
            part = r.readAccum()
            assert not part[~owned].any(), "the rank wrote outside its rows, " + what
            assert np.array_equal(pu.bits(part[owned]), pu.bits(want[owned])), \
                pu.describe_mismatch("accumulation buffer, " + what, part[owned], want[owned])
        finally:
            r.destroy()
