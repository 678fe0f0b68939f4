"""Hostile triangle records (tests/hostile_records.py: non-finite and out-of-range material words, roughness, ior, metallic,
albedo, emission, texture words, vertex uvs and vertex normals, one field per triangle, a family per scene) through every
shading form of the GPU, against the oracle and the radiance / gather models.  tests/test_hostile_records_model.py shows on
the CPU that these finish, that the pictures are lit, that every hostile triangle is a depth-0 hit of every frame at both
sizes (so every frame form below shades every hostile record) and that a query ray shades each of them at depth 0 too.  The
forms copy one per-path state machine by template; none of them had shaded such a record.

Frames (37 x 29 and 24 x 16, depth 8, frames 1-3): the persistent kernel with the scene in LDS and behind the L1, the
one-pixel-per-lane kernel, the batched wavefront form on single nodes and on child pairs, the batched persistent kernel
(on the one-leaf scene the product build takes the wide form; for the plain-preserving family its plain twin, and the generic
form with the choice switched off).  Every form runs in the counting build, where all six ray counters are compared, and the
batched forms in the product build as well, which keeps primary, extension and shadow rays only; the wide one-leaf form exists
in the product build alone (launch_plan.h persistent_shape), so it is the one form compared on three counters only.
Queries: traceRadiance on the centroid rays and gatherIrradiance on the points in front of their hits, in the LDS and the
global-memory form, counting and product build.  Accumulation buffers, query records and ray counters are compared bit for
bit; where the oracle or the model has a NaN, a NaN of any payload is accepted (radiance_util.check_records_against_model and
its twin parity_util.assert_accum_against_oracle)."""
import numpy as np
import pytest

import gather_util as gu
import hostile_records as hr
import parity_util as pu
import radiance_util as ru

pytestmark = pytest.mark.gpu

SIZES = ((37, 29), (24, 16))
DEPTH, FRAMES = 8, (1, 2, 3)
QUERY, GATHER = (8, 2), (4, 2)            # (max_depth, spp)
CASES = [(scene, name) for scene in sorted(hr.SCENES) for name in hr.NAMES]

# tag, MI355RT_NO_LDS_STAGING, kernel variant, walk of the wavefront form, frames per dispatch, counting build
FORMS = [
    ("persistent, LDS", None, 1, None, 1, True),
    ("persistent, global memory", "1", 1, None, 1, True),
    ("one pixel per lane", None, 0, None, 1, True),
    ("wavefront, single nodes, counting", None, 2, 0, 3, True),
    ("wavefront, single nodes, product", None, 2, 0, 3, False),
    ("wavefront, child pairs, counting", None, 2, 1, 3, True),
    ("wavefront, child pairs, product", None, 2, 1, 3, False),
    ("persistent, batched, counting", None, 1, None, 3, True),
    ("persistent, batched, product", None, 1, None, 3, False),
]

_oracles = {}


def _oracle(W, oracle_lib, scene, name, w, h):
    """the oracle's renderer after the frames of a family, made once and only read afterwards"""
    key = (scene, name, w, h)
    if key not in _oracles:
        cpu = oracle_lib.OracleRenderer()
        pu.drive(cpu, W, hr.prepared(scene).family(name)[0], w, h, DEPTH, 1, FRAMES, present=False)
        _oracles[key] = (cpu.readAccum(), cpu.getCounters())
    return _oracles[key]


def _render(W, monkeypatch, b, w, h, no_lds, variant, walk, batch, counting, plain_knob=None):
    """a context created AFTER the env knobs are set, after the frames"""
    for knob, value in (("MI355RT_NO_LDS_STAGING", no_lds), ("MI355RT_PLAIN_MATERIALS", plain_knob)):
        if value is None:
            monkeypatch.delenv(knob, raising=False)
        else:
            monkeypatch.setenv(knob, value)
    W._build.build_rt()
    r = W.WebGPURenderer(0)
    r.setKernelVariant(variant)
    if walk is not None:
        r.setWalk(walk)
    r.buildPipeline(DEPTH, 1)
    W.upload_scene(r, b, w, h)
    r.setCounting(counting)
    r.resetCounters()
    for i in range(0, len(FRAMES), batch):
        if batch == 1:
            r.compute(FRAMES[i])
        else:
            r.computeBatch(list(FRAMES[i:i + batch]))
    r.sync()
    return r


def _check_frames(r, want, counters, counting, what):
    pu.assert_accum_against_oracle(r.readAccum(), want, what, nan_as_class=True)
    got = r.getCounters()
    names = tuple(counters) if counting else pu.RAY_COUNTERS
    assert {k: got[k] for k in names} == {k: counters[k] for k in names}, what


@pytest.mark.parametrize("scene,name", CASES)
def test_frames_of_every_form_equal_the_oracle(W, oracle_lib, monkeypatch, scene, name):
    b, hostile = hr.prepared(scene).family(name)
    one_leaf = scene == "one_leaf"
    for w, h in SIZES:
        want, counters = _oracle(W, oracle_lib, scene, name, w, h)
        for tag, no_lds, variant, walk, batch, counting in FORMS:
            what = "%s %s %dx%d, %s" % (scene, name, w, h, tag)
            r = _render(W, monkeypatch, b, w, h, no_lds, variant, walk, batch, counting)
            try:
                if variant == 1:
                    wide = one_leaf and batch > 1 and not counting
                    assert r.debugPtLaunch()["threads"] == (512 if wide else 256), what
                    assert r.debugPtForm() == ("plain" if wide and name == "plain_preserving" else "generic"), what
                else:
                    assert r.debugPtForm() == "none", what
                _check_frames(r, want, counters, counting, what)
            finally:
                r.destroy()
        if one_leaf and name == "plain_preserving":
            what = "%s %s %dx%d, the generic twin of the plain form" % (scene, name, w, h)
            r = _render(W, monkeypatch, b, w, h, None, 1, None, 3, False, plain_knob="0")
            try:
                assert r.debugPtLaunch()["threads"] == 512 and r.debugPtForm() == "generic", what
                _check_frames(r, want, counters, False, what)
            finally:
                r.destroy()


@pytest.mark.parametrize("scene,name", CASES)
def test_queries_equal_the_models(W, monkeypatch, scene, name):
    p = hr.prepared(scene)
    b, hostile = p.family(name)
    m = gu.model_for(W, b)
    ref, counts = m.traceRadiance(p.rays, *QUERY, ru.SEED)
    gref, _, gcounts = m.gatherIrradiance(p.points, *GATHER, gu.SEED)
    for no_lds in (None, "1"):
        what = "%s %s no_lds=%s" % (scene, name, no_lds)
        if no_lds is None:
            monkeypatch.delenv("MI355RT_NO_LDS_STAGING", raising=False)
        else:
            monkeypatch.setenv("MI355RT_NO_LDS_STAGING", no_lds)
        W._build.build_rt()
        r = W.WebGPURenderer(0)
        try:
            W.upload_scene(r, b, 16, 16)
            res, st = r.traceRadiance(p.rays, *QUERY, ru.SEED, stats=True)
            assert st["lds"] == (1 if no_lds is None else 0), (what, st)
            ru.check_records_against_model(res, ref, what + ", radiance", nan_as_class=True, what="rays")
            ru.check_counts(st, counts, len(p.rays), QUERY[1], what + ", radiance")
            plain = r.traceRadiance(p.rays, *QUERY, ru.SEED)
            ru.check_records_against_model(plain, ref, what + ", radiance, product build", nan_as_class=True, what="rays")
            res, st = r.gatherIrradiance(p.points, *GATHER, gu.SEED, stats=True)
            assert st["lds"] == (1 if no_lds is None else 0), (what, st)
            gu.check_against_model(res, gref, what + ", gather", nan_as_class=True)
            gu.check_counts(st, gcounts, len(p.points), GATHER[1], what + ", gather")
            plain = r.gatherIrradiance(p.points, *GATHER, gu.SEED)
            gu.check_against_model(plain, gref, what + ", gather, product build", nan_as_class=True)
        finally:
            r.destroy()
