"""The block primitives of csrc/k_block_scan.hip.h by themselves: block_count, block_rank, block_scan_inclusive and
array_scan_exclusive (the u32 one through rtk::k_scan_counts), each behind a trivial kernel of a small library of its own
(tests/model/scan_check.hip, built with the product's compiler and flags), against numpy's cumsum / count_nonzero, exactly.

The shapes are the smallest at which each can go wrong: several waves and several blocks, a last block that is not full, two
calls in a row on the same scratch (the leading barrier), arrays of fewer elements than threads, of exactly as many, and of
more (a run per thread, trailing threads without one), 64-bit sums that pass 2^32."""
import ctypes
import os

import numpy as np
import pytest

import model_build

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "model", "scan_check.hip")
RANK, INCLUSIVE, ARRAY_U32, ARRAY_U64 = 0, 1, 2, 3
TOTAL_SEPARATE, TOTAL_BEHIND, TOTAL_NULL = 0, 1, 2


@pytest.fixture(scope="module")
def device(W):
    build = W._build
    L = ctypes.CDLL(model_build.build(SRC, os.path.join(HERE, "model", "_build", "libscan_check.so"),
                                      list(build.HIP_FLAGS) + ["-I", build.CSRC], build.HIPCC))
    L.scan_check.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    L.scan_check.restype = ctypes.c_int
    return L


def run(device, op, threads, total_mode, n, data, n_out, dtype=np.uint32):
    data = np.ascontiguousarray(data, dtype=dtype)
    out = np.zeros(n_out, dtype=dtype)
    rc = device.scan_check(op, threads, total_mode, n, data.ctypes.data, out.ctypes.data)
    assert rc == 0, "scan_check(op %d, %d threads, n %d): HIP error %d" % (op, threads, n, rc)
    return out


def flag_patterns(T, n):
    rng = np.random.default_rng(20240 + T)
    pats = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternating": np.arange(n) % 2 == 0,
            "half": rng.random(n) < 0.5, "sparse": rng.random(n) < 1.0 / 64}
    for k in (0, 63, 64, T - 1, T):
        pats["one_at_%d" % k] = np.arange(n) == k
    return pats


@pytest.mark.parametrize("pattern", ["none", "all", "one_at_0", "one_at_63", "one_at_64", "one_at_last", "one_at_T", "alternating",
                                     "half", "sparse"])
@pytest.mark.parametrize("T", [256, 1024])
def test_block_rank_and_count(device, T, pattern):
    """3 blocks over n = 3 T - 5 flags: ranks and totals of flag and of !flag (second call on the same s_wave), and
    block_count of either against the same totals."""
    n, blocks = 3 * T - 5, 3
    key = {"one_at_last": "one_at_%d" % (T - 1), "one_at_T": "one_at_%d" % T}.get(pattern, pattern)
    flag = flag_patterns(T, n)[key]
    out = run(device, RANK, T, 0, n, flag.astype(np.uint32), 2 * n + 4 * blocks)
    padded = np.zeros(blocks * T, bool)
    padded[:n] = flag
    inside = np.arange(blocks * T) < n
    for which, f in ((0, padded), (1, inside & ~padded)):
        per_block = f.reshape(blocks, T)
        want_rank = (np.cumsum(per_block, axis=1) - per_block).reshape(-1)[:n]
        want_total = np.count_nonzero(per_block, axis=1)
        assert np.array_equal(out[which * n:(which + 1) * n], want_rank), (T, pattern, which)
        totals = out[2 * n:].reshape(blocks, 4)
        assert np.array_equal(totals[:, which], want_total), (T, pattern, which, totals)
        assert np.array_equal(totals[:, 2 + which], want_total), (T, pattern, which, totals)


@pytest.mark.parametrize("T", [256, 1024])
def test_block_scan_inclusive_twice_on_one_scratch(device, T):
    v = np.random.default_rng(7 + T).integers(0, 1025, size=2 * T, dtype=np.uint32)
    out = run(device, INCLUSIVE, T, 0, 0, v, 2 * T + 2)
    want0, want1 = np.cumsum(v[:T], dtype=np.uint32), np.cumsum(v[T:], dtype=np.uint32)
    assert np.array_equal(out[:T], want0)
    assert np.array_equal(out[T:2 * T], want1)
    assert (out[2 * T], out[2 * T + 1]) == (want0[-1], want1[-1])   # s[T - 1] after either call


SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3073, 65536, 65537]   # 65536: the blocks of a 2^24-texel atlas
_values = {}


def values(dtype, n):
    """the seeded input of a size, made once: u32 in [0, 1024] (sums below 2^32), u64 up to 2^40 (sums pass 2^32)"""
    if (dtype, n) not in _values:
        hi = 1025 if dtype == np.uint32 else (1 << 40) + 1
        v = np.random.default_rng(n + (0 if dtype == np.uint32 else 99991)).integers(0, hi, size=n, dtype=dtype)
        v.setflags(write=False)
        _values[(dtype, n)] = v
    return _values[(dtype, n)]


@pytest.mark.parametrize("total_mode", [TOTAL_SEPARATE, TOTAL_BEHIND, TOTAL_NULL], ids=["separate", "behind", "null"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op,dtype", [(ARRAY_U32, np.uint32), (ARRAY_U64, np.uint64)], ids=["u32_k_scan_counts", "u64"])
def test_array_scan_exclusive(device, op, dtype, n, total_mode):
    v = values(dtype, n)
    mark_behind, mark_separate = dtype(0xA5A5A5A5), dtype(0x5A5A5A5A)
    data = np.concatenate([v, np.array([mark_behind, mark_separate], dtype=dtype)])
    out = run(device, op, 1024, total_mode, n, data, n + 2, dtype)
    total = v.sum(dtype=dtype)
    assert np.array_equal(out[:n], np.cumsum(v, dtype=dtype) - v), (n, total_mode)
    assert out[n] == (total if total_mode == TOTAL_BEHIND else mark_behind), (n, total_mode)   # untouched unless it is the total
    assert out[n + 1] == (total if total_mode == TOTAL_SEPARATE else mark_separate), (n, total_mode)
    if dtype == np.uint64 and n >= 65536:
        assert int(total) >= 1 << 32   # a truncation to 32 bits would show
