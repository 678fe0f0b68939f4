"""What the host works out about the materials of a topology upload (csrc/scene_facts.h) and what the launch planner makes
of it (csrc/launch_plan.h persistent_shape).  The plain form of the wide one-leaf path tracer is compiled without the GGX
and dielectric branches, the texture fetches and the emissive length, so a scene wrongly called plain is a wrong image: each
clause of the condition is tried here on its own, on both sides, with the values the kernel's own expressions turn on (a NaN
material word saturates to 0, a NaN texture index fails `> -0.5`, the emission is compared by its f32 length).
tests/model/scene_facts_check.cpp wraps the header; host compiler only, no GPU."""
import ctypes
import os

import numpy as np
import pytest

import model_build

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "webgpu-raytracer_amd", "csrc")
SRC = os.path.join(HERE, "model", "scene_facts_check.cpp")
LIB = os.path.join(HERE, "model", "_build", "libscene_facts_check.so")

UNKNOWN, NOT_PLAIN, PLAIN = 0, 1, 3   # known | plain << 1
f32 = np.float32


@pytest.fixture(scope="module")
def facts():
    flags = ["-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"]
    L = ctypes.CDLL(model_build.build(SRC, LIB, flags))
    L.sfc_max_tris.restype = ctypes.c_uint64
    L.sfc_eval.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    L.sfc_eval.restype = ctypes.c_int
    L.sfc_shape.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_int] * 3
    L.sfc_shape.restype = ctypes.c_int
    return L


def evaluate(L, topo):
    topo = np.ascontiguousarray(topo, dtype=np.float32).reshape(-1, 20)
    return L.sfc_eval(topo.ctypes.data_as(ctypes.c_void_p), len(topo))


def triangles(n=3):
    """n untextured Lambertian triangles without emission, as rows of 20 words (rt_topology)."""
    t = np.zeros((n, 20), np.float32)
    t.view(np.uint32)[:, 0:3] = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    t[:, 4:7] = 0.73
    t[:, 7] = 0.0                      # data0.w: material
    t[:, 8:12] = (0.0, 0.5, 1.5, 0.0)  # data1
    t[:, 12:16] = -1.0                 # data2: the four texture indices
    t[:, 19] = -1.0                    # data3.w: occlusion texture (no reader)
    return t


def with_(word, value, row=1):
    t = triangles()
    t[row, word] = value
    return t


def test_cornell_is_plain(W, facts):
    b = W.WorldBridge()
    b.loadScene("cornell")
    topo = np.asarray(b.mesh_topology, np.uint32).view(np.float32).reshape(-1, 20)
    assert len(topo) == 36
    assert sorted(set(topo[:, 7].tolist())) == [0.0, 3.0] and (topo[:, 12:16] == -1.0).all() and not topo[:, 16:19].any()
    assert evaluate(facts, topo) == PLAIN


@pytest.mark.parametrize("material", [1.0, 2.0, 4.0, 0.5, 1.5, 3.5, 1e9])
def test_another_material_is_not_plain(facts, material):
    assert evaluate(facts, with_(7, material)) == NOT_PLAIN


@pytest.mark.parametrize("material", [0.0, 3.0, 0.49, -0.0, -7.0, 2.5, 2.75, 3.25, float("nan"), float("-inf")])
def test_material_words_that_decode_to_0_or_3(facts, material):
    """u32(word + 0.5), saturating, NaN -> 0: the kernel's decode."""
    assert evaluate(facts, with_(7, material)) == PLAIN


@pytest.mark.parametrize("word", [12, 13, 14, 15])
def test_a_texture_index_is_not_plain(facts, word):
    assert evaluate(facts, with_(word, 0.0)) == NOT_PLAIN
    assert evaluate(facts, with_(word, 5.0, row=2)) == NOT_PLAIN
    assert evaluate(facts, with_(word, -0.25)) == NOT_PLAIN     # the test is `> -0.5`
    assert evaluate(facts, with_(word, -0.5)) == PLAIN
    assert evaluate(facts, with_(word, float("nan"))) == PLAIN  # NaN > -0.5 is false in the kernel too


def test_emission_counts_on_a_lambertian_triangle_only(facts):
    t = triangles()
    t[1, 16] = 0.5
    assert evaluate(facts, t) == NOT_PLAIN
    t[1, 7] = 3.0      # the same emission on a light
    assert evaluate(facts, t) == PLAIN
    t = triangles()
    t[2, 16:19] = float("nan")   # length NaN: `> 1e-4` is false
    assert evaluate(facts, t) == PLAIN


def test_emission_threshold(facts):
    """rt_length(e) > 1e-4f in f32: sqrt(x * x) of a single component, four ulps either side."""
    lim = f32(1e-4)
    above, below = lim + 4 * np.spacing(lim), lim - 4 * np.spacing(lim)
    assert np.sqrt(above * above, dtype=f32) > lim and not np.sqrt(below * below, dtype=f32) > lim
    for word in (16, 17, 18):
        assert evaluate(facts, with_(word, above)) == NOT_PLAIN
        assert evaluate(facts, with_(word, -above)) == NOT_PLAIN
        assert evaluate(facts, with_(word, below)) == PLAIN
    t = triangles()   # three components below the limit whose length is above it
    t[0, 16:19] = f32(7e-5)
    assert evaluate(facts, t) == NOT_PLAIN


def test_empty_topology_is_plain(facts):
    assert facts.sfc_eval(None, 0) == PLAIN


def test_an_upload_over_the_cap_is_not_scanned(facts):
    cap = int(facts.sfc_max_tris())
    # every triangle of an LDS-resident scene takes 16 slots of 16 bytes of the 64 KB (traversal, shading, topology record)
    assert cap == 64 * 1024 // 256
    assert evaluate(facts, triangles(cap)) == PLAIN
    assert evaluate(facts, triangles(cap + 1)) == UNKNOWN
    assert facts.sfc_eval(None, 263_000) == UNKNOWN   # the pointer is not followed


# (nodes, triangles, vertices) of Cornell and of two random one-leaf scenes, one on each side of the wide form's LDS line
@pytest.mark.parametrize("size", [(22, 36, 72), (26, 30, 90), (28, 45, 135)])
def test_the_planner_takes_the_plain_form_for_wide_launches_of_known_plain_scenes_only(facts, size):
    for frames in (1, 2, 32):
        for detailed in (0, 1):
            for f in (UNKNOWN, NOT_PLAIN, PLAIN, 2):   # 2: plain without known
                for knob in (0, 1):
                    got = facts.sfc_shape(*size, frames, detailed, f, knob)
                    assert got >= 0, "the facts changed the launch shape"
                    wide = bool(got & 1)
                    assert wide == (frames > 1 and not detailed and size[1] < 45)
                    assert bool(got & 2) == (wide and f == PLAIN and knob == 1)


def test_scene_facts_is_host_only():
    text = open(os.path.join(CSRC, "scene_facts.h")).read()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text
