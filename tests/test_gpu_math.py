"""The DEVICE compilation of include/mi355rt_math.h equals the HOST compilation, bit for bit, over whole input spaces.

The oracle and every tests/model/*.cpp compile the header for the host, the kernels for gfx950; parity of rendered images
only visits a sliver of either (angles in [0, 2 pi], pow on [0, 1], ...).  Here each function of the header is run on the
GPU over the enumeration of tests/model/math_inputs.h (all 2^32 inputs of the one-operand functions; exponent classes x
hashed mantissas and every pair of special values for the others) by a small library of its own, built with the product's
compiler and flags (tests/model/math_check.hip), and its checksum is compared with the host's (tests/model/math_ref.cpp).
One differing result word moves the checksum by delta * (2 k + 1) mod 2^64 with 0 < |delta| < 2^32, which is never 0.
rcp / sqrt / rsqrt / div by themselves stay with tests/test_gpu_ieee.py.

The kernels' RNG (init_rng / rand_pcg of csrc/k_common.hip.h, device-only code) rides along: 2^20 (pixel, frame) pairs and
all 2^32 states against the oracle's own Oracle::init_rng / rand_pcg, through bulk exports of the oracle library."""
import pytest

import math_util as M

pytestmark = pytest.mark.gpu

# The host side of a 2^32 sweep is the slow one (results that underflow cost the CPU a microcode assist each): the ops
# below are cut into this many equal index ranges, one case each.  Checksums add, so nothing is thinned.
PARTS = {"sincos": 16, "exp": 16, "pow22": 4, "log": 2, "unorm8": 2}
SIZES = {"f16_to_f32": 1 << 16, "pow2i": 254, "min": M.GENERAL + 17 ** 2, "max": M.GENERAL + 17 ** 2, "clamp": M.GENERAL + 17 ** 3,
         "mix": M.GENERAL + 17 ** 3, "pow": 16 + 512, "rgbe8": 1 << 24, "resize_coord": 15 * 1024, "bilinear_u8": 1 << 24,
         "init_rng": 1 << 20, "rand_pcg": 1 << 32}


def _size(op):
    if op in SIZES:
        return SIZES[op]
    return (1 << 32) if M.OP[op] <= M.OP["abs_sat"] else M.VEC_NARROW + (1 << 20)


def _cases():
    out = []
    for op in M.OPS:
        size, parts = _size(op), PARTS.get(op, 1)
        assert size % parts == 0
        out += [pytest.param(op, k * (size // parts), size // parts, id="%s-%d" % (op, k) if parts > 1 else op) for k in range(parts)]
    return out


@pytest.fixture(scope="module")
def device(W):
    return M.bind_check(M.build_check(W._build))


def test_sizes_are_the_headers(device):
    R = M.ref()
    assert all(R.math_ref_op_size(M.OP[op]) == _size(op) for op in M.OPS)


@pytest.mark.parametrize("op,first,count", _cases())
def test_device_equals_host(device, op, first, count):
    rep = M.device_check(device, op, first, count)
    want_sum, want_n = M.ref_sweep(op, first, count)
    assert rep.n == count
    if (rep.checksum, rep.in_domain) != (want_sum, want_n):
        pytest.fail("device checksum %016x over %d inputs, host %016x over %d; %s"
                    % (rep.checksum, rep.in_domain, want_sum, want_n, M.first_difference(device, op, first, count)))


def test_ranges_add(device):
    """How a longer sweep is chunked, and what first_difference relies on; also across the edge of the rt_sincos domain
    (biased exponent 157 | 158), where one half contributes and the other does not."""
    for op, first, count in (("exp", 0x3F000000, 1 << 22), ("sincos", (158 << 23) - (1 << 20), 1 << 21)):
        whole = M.device_check(device, op, first, count)
        a = M.device_check(device, op, first, count // 2)
        b = M.device_check(device, op, first + count // 2, count // 2)
        assert (a.checksum + b.checksum) % (1 << 64) == whole.checksum
        assert a.in_domain + b.in_domain == whole.in_domain
        assert (whole.checksum, whole.in_domain) == M.ref_sweep(op, first, count)
    assert (a.in_domain, b.in_domain) == (count // 2, 0)


EXP_HI, EXP_LO = M.f32_bits(88.72283905206835), M.f32_bits(-87.33654475055310898657)   # rt_exp: inf above, 0 below
NAMED = {
    "sincos": [0x00000000, 0x80000000, 0x00000001, (158 << 23) - 1, 0x80000000 | ((158 << 23) - 1), 158 << 23, 0x4014C969, 0x4018CE5F,
               0x40C90FDB],
    "exp": [0x00000000, 0x80000000, EXP_HI, EXP_HI + 1, EXP_HI - 1, EXP_LO, EXP_LO + 1, EXP_LO - 1, 0x428CCE63, 0x7FC00000],
    "log": [0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x3FB4DE30, 0x7F7FFFFF, 0x7F800000, 0x00000000, 0x80000000, 0xBF800000],
    "pow22": [0x00000000, 0x80000000, 0x3F800000, 0x3EA8F07D, 0x35944E0F],
    "floor": [0x80000000, 0xBF000000, 0x4B000001, 0xCB000001, 0x3F7FFFFF],
    "f2u32_sat": [0x4F800000, 0x4F7FFFFF, 0xBF800000, 0x7FC00000, 0x7F800000],
    "f2i32_sat": [0x4F000000, 0x4EFFFFFF, 0xCF000000, 0xCF000001, 0x7FC00000],
    "f32_to_f16": [0x477FE000, 0x477FF000, 0x477FEFFF, 0x33000000, 0x33000001, 0x387FE000, 0x7FA00000, 0x80000000],   # 65504, 65520, ...
    "unorm8": [0x3B008081, 0x3F7FFFFF, 0x7FC00000, 0xBF800000, 0x3F000000],
    "abs_sat": [0x80000000, 0xFFC00000, 0x7FA00000, 0x3F800001, 0x80000001],
    "f16_to_f32": [0x0000, 0x8000, 0x0001, 0x03FF, 0x0400, 0x7BFF, 0x7C00, 0x7E00, 0xFC01],
    "pow2i": [0, 126, 253],
    "min": [M.GENERAL + 0 + 17 * 1, M.GENERAL + 1 + 17 * 0, M.GENERAL + 16 + 17 * 8, M.GENERAL + 8 + 17 * 16, M.GENERAL + 14 + 17 * 16],
    "max": [M.GENERAL + 0 + 17 * 1, M.GENERAL + 1 + 17 * 0, M.GENERAL + 16 + 17 * 8, M.GENERAL + 8 + 17 * 16, M.GENERAL + 14 + 17 * 16],
    "clamp": [M.GENERAL + 16 + 17 * 0 + 289 * 8, M.GENERAL + 8 + 17 * 14 + 289 * 9, 5],
    "mix": [M.GENERAL + 12 + 17 * 13 + 289 * 8, 4, 5],
    "pow": list(range(16)) + [16, 527],
    "dot": [0, M.VEC_NARROW, M.VEC_NARROW + (255 << 12)],
    "normalize": [0, M.VEC_NARROW, M.VEC_NARROW + (255 << 12)],
    "refract": [0, 1, M.VEC_NARROW + 5],
    "div3z": [3, 11, M.VEC_NARROW + 3],
    "mat_mul_point": [0, M.VEC_NARROW + (0x9F << 12)],
    "rgbe8": [0, 31 << 16, 32 << 16, 253 << 16, 254 << 16, (255 << 16) + 77],
    "resize_coord": [0, 1023, 9 * 1024 + 511, 14 * 1024, 14 * 1024 + 1023],
    "bilinear_u8": [0, 1, 2, 77],
    "init_rng": [0, 1, 2, 5, (1 << 20) - 1],
    "rand_pcg": [0x00000000, 0xFFFFFFFF, 0x0FFFFFFF, 0xF0000000, 0x9E3779B9],
}


@pytest.mark.parametrize("op", sorted(NAMED))
def test_single_inputs_read_back(device, op):
    """value[] of a one-index call holds the device's result words (what a bisection ends with): equal to the host's at
    named inputs — zeros, the edge of the sincos domain, the inputs of the worst measured errors, both thresholds of rt_exp,
    the smallest subnormal into rt_log, 65504 / 65520 into rt_f32_to_f16, NaN and sNaN operands."""
    for i in NAMED[op]:
        rep = M.device_check(device, op, i, 1)
        host = M.ref_value(op, i)
        assert rep.in_domain == (1 if host else 0), (op, i)
        assert [M.canon(op, w) for w in rep.value[:len(host)]] == [M.canon(op, w) for w in host], \
            "%s at index %d (operands %s): device %s, host %s" % (op, i, ["%08x" % w for w in M.ref_operands(op, i)],
                                                                  ["%08x" % w for w in rep.value[:len(host)]], ["%08x" % w for w in host])
