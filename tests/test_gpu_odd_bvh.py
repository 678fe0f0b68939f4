"""The kernels on legal BVH arrays the builders never emit (tests/odd_bvh.py) against the oracle: every kernel form and
walk, the staging knobs and the product build, plus the arrays derived at upload (tnodes, pair records).

The item queue of the triangle flush, LDS staging, treelet order and the wavefront / product instances run only here;
tests/test_odd_bvh.py pins the walk logic on the host first (a layout the walk cannot leave would hang a kernel).
`empty_leaf_flush` is built so that a count-0 leaf that corrupts the flush's item queue changes the image."""
import numpy as np
import pytest

import odd_bvh
import parity_util as pu
from test_gpu_product_build import _check as check_product

pytestmark = pytest.mark.gpu

W_, H_, DEPTH, FRAMES = 64, 48, 6, (1, 2, 3)
# (cases, seed): every case alone, then combinations
SCENES = [((c,), 3 if c == "tiny_trees" else 2) for c in odd_bvh.CASES] + [
    (("empty_leaves", "loose_boxes", "single_child"), 5),
    (("raw_fallback_words", "degenerate_boxes", "unreachable_gaps"), 5),
    (("tiny_trees", "empty_leaves"), 7),                 # 24 instances of one single-leaf BLAS
    (("tiny_trees", "single_child"), 5),                 # three geometries, some single-leaf
    (("deep_comb", "empty_leaves", "single_child"), 5)]
IDS = ["+".join(c) for c, _ in SCENES]


def _scene(cs):
    cases, seed = cs
    return odd_bvh.make(seed, cases)


def _oracle(oracle_lib, W, b):
    cpu = oracle_lib.OracleRenderer()
    pu.drive(cpu, W, b, W_, H_, DEPTH, 1, FRAMES, present=False)
    return cpu


def _gpu(W, b, variant, walk=None, counting=True):
    r = W.WebGPURenderer(0)
    r.setKernelVariant(variant)
    if walk is not None:
        r.setWalk(walk)
    r.buildPipeline(DEPTH, 1)
    W.upload_scene(r, b, W_, H_)
    r.setCounting(counting)
    r.resetCounters()
    for f in FRAMES:            # one compute() per frame: variant 0 (one pixel per lane) takes no batches
        r.compute(f)
    r.sync()
    return r


def _check_counting(gpu, cpu):
    """accumulation, G-buffer, uniforms and all six counters; then present(): RGBA8 output and history"""
    pu.assert_parity(gpu, cpu, check_output=False)
    gpu.present()
    cpu.present()
    pu.assert_parity(gpu, cpu, check_output=True, check_counters=False)


@pytest.mark.parametrize("cases", SCENES, ids=IDS)
@pytest.mark.parametrize("variant,walk", [(0, None), (1, None), (2, 0), (2, 1)])
def test_counting_build_parity(W, oracle_lib, cases, variant, walk):
    b = _scene(cases)
    cpu = _oracle(oracle_lib, W, b)
    r = _gpu(W, b, variant, walk)
    try:
        _check_counting(r, cpu)
    finally:
        r.destroy()


@pytest.mark.parametrize("cases", SCENES, ids=IDS)
@pytest.mark.parametrize("env,value,variant", [("MI355RT_NO_LDS_STAGING", "1", 1), ("MI355RT_NO_LDS_STAGING", "1", 2),
                                               ("MI355RT_TREELET_MAX", "8", 1), ("MI355RT_TREELET_MAX", "8", 2)])
def test_staging_knobs_keep_parity(W, oracle_lib, monkeypatch, cases, env, value, variant):
    """records read through the L1 (no LDS staging), or only the first 8 traversal nodes staged: the treelet prefix cuts
    through the trees, combs and gaps of these arrays"""
    monkeypatch.setenv(env, value)
    b = _scene(cases)
    cpu = _oracle(oracle_lib, W, b)
    r = _gpu(W, b, variant)
    try:
        _check_counting(r, cpu)
    finally:
        r.destroy()


@pytest.mark.parametrize("cases", SCENES, ids=IDS)
@pytest.mark.parametrize("variant,walk", [(1, None), (2, 0), (2, 1)])
def test_product_build_parity(W, oracle_lib, cases, variant, walk):
    b = _scene(cases)
    cpu = _oracle(oracle_lib, W, b)
    r = _gpu(W, b, variant, walk, counting=False)
    try:
        check_product(r, cpu)
    finally:
        r.destroy()


@pytest.mark.parametrize("cases", SCENES, ids=IDS)
def test_derived_arrays(W, gpu_renderer, cases):
    """tnodes follow the original skips (unreachable ranges and single-child nodes included) and the pair records equal
    tests/pair_layout.py byte for byte (empty slots of single-child nodes included)"""
    b = _scene(cases)
    r = gpu_renderer
    r.buildPipeline(4, 1)
    W.upload_scene(r, b, 32, 16)
    pu.check_traversal_nodes(r, b)
    pu.check_pair_records(r, b)
