"""The host compilation of include/mi355rt_math.h, pinned over whole input spaces (no GPU needed), and the machinery that
compares it with the device compilation (tests/test_gpu_math.py) shown to be able to see what it is for.

  * accuracy: every f32 of each function's domain against double-precision libm, asserted at the measured maximum rounded
    up in the third digit (the table is in the docstrings below and in DESIGN.md section 4.1);
  * g++ and ROCm's clang++ compile the header to the same results (checksums over the reduced enumeration of
    tests/model/math_ref.cpp: every exponent class of every op, about 2^12 samples each);
  * the same enumeration runs clean as a stand-alone program under the undefined-behaviour sanitizer, which is what fixes
    the rt_sincos domain at |x| < 2^31;
  * a build that contracts a * b + c into fma changes the checksum of every op that has such an expression: the inputs can
    see a dropped -ffp-contract=off;
  * the input sets reach the branches they are meant to reach;
  * the device side compiles for gfx950 with the product flags and keeps everything in registers.
"""
import os
import subprocess

import pytest

import math_util as M


F32_ONE = 0x3F800000
TWO_PI_BITS = 0x40C90FDB                           # RT_TWO_PI
EXP_LO_BITS = M.f32_bits(-87.33654475055310898657)      # rt_exp returns 0 below this f32
EXP_HI_BITS = M.f32_bits(88.72283905206835)             # and inf above this one
CHUNK = 1 << 28                    # a sweep is cut into ranges of this many inputs, one test case each


def _ranges(first, last):
    """[first, last] in bit patterns as (first, count) chunks."""
    out, lo = [], first
    while lo <= last:
        n = min(CHUNK, last - lo + 1)
        out.append((lo, n))
        lo += n
    return out


def _max_over(fn, ranges):
    best = (-1.0, 0)
    for lo, n in ranges:
        mx, arg, _ = M.accuracy(fn, lo, n)
        print("%s [%08x, +%d): max %.4g at %08x" % (fn, lo, n, mx, arg))
        best = max(best, (mx, arg))
    return best


# ------------------------------------------------------------------------------------------------- accuracy, exhaustive
# Measured at the commit that added this file: g++ 11 -O2 -ffp-contract=off -fno-fast-math, glibc 2.35 libm in double.
#   rt_sincos   every f32 in [0, RT_TWO_PI]             max |sin err| 6.957e-8 (x = 0x4014c969), max |cos err| 7.773e-8 (0x4018ce5f)
#   rt_exp      every f32 in [-87.33654, 88.72283]      max 0.9903 ulp (x = 0x428cce63)
#   rt_log      every positive finite f32               max 0.8337 ulp (x = 0x3fb4de30)
#   rt_pow(x, f32(1 / 2.2))   every f32 in [0, 1]       max abs err 7.095e-8
# ulp(v) is the f32 spacing in the binade of the libm value v: 2^(floor(log2 |v|) - 23), 2^-149 below 2^-126.
@pytest.mark.parametrize("first,count", _ranges(0, TWO_PI_BITS))
@pytest.mark.parametrize("fn,bound", [("sin", 6.96e-8), ("cos", 7.78e-8)])
def test_sincos_accuracy_over_a_turn(fn, bound, first, count):
    mx, arg = _max_over(fn, [(first, count)])
    assert mx <= bound, "%s: %.4g at x = %08x" % (fn, mx, arg)


@pytest.mark.parametrize("first,count", _ranges(0, EXP_HI_BITS) + _ranges(0x80000000, EXP_LO_BITS))
def test_exp_accuracy_in_ulp(first, count):
    mx, arg = _max_over("exp", [(first, count)])
    assert mx <= 0.991, "exp: %.4g ulp at x = %08x" % (mx, arg)


@pytest.mark.parametrize("first,count", _ranges(1, 0x7F7FFFFF))
def test_log_accuracy_in_ulp(first, count):
    mx, arg = _max_over("log", [(first, count)])
    assert mx <= 0.834, "log: %.4g ulp at x = %08x" % (mx, arg)


@pytest.mark.parametrize("first,count", _ranges(0, F32_ONE))
def test_pow_gamma_accuracy(first, count):
    mx, arg = _max_over("pow", [(first, count)])
    assert mx <= 7.10e-8, "pow: %.4g at x = %08x" % (mx, arg)


def test_unorm8_of_pow_gamma_disagreements():
    """rt_unorm8(rt_pow(x, f32(1 / 2.2))) over every f32 in [0, 1] against floor(255 pow + 0.5) in double: exactly 409 inputs
    land on the other side of a rounding boundary, each by one code."""
    total, worst = 0, 0.0
    for lo, n in _ranges(0, F32_ONE):
        cnt, arg, aux = M.accuracy("unorm8_pow", lo, n)
        print("unorm8_pow [%08x, +%d): %d disagreements, first at %08x, largest %g" % (lo, n, cnt, arg, aux))
        total += int(cnt)
        worst = max(worst, aux)
    assert total == 409 and worst == 1.0, (total, worst)


def _f16c():
    try:
        with open("/proc/cpuinfo") as f:
            return " f16c" in f.read()
    except OSError:
        return False


@pytest.mark.skipif(not _f16c(), reason="no F16C on this CPU: no independent f16 conversion to compare with")
@pytest.mark.parametrize("first,count", _ranges(0, 0xFFFFFFFF))
def test_f32_to_f16_equals_the_cpu_instruction(first, count):
    """All 2^32 inputs against VCVTPS2PH, round to nearest even (any NaN = any NaN)."""
    got = M.accuracy("f32_to_f16", first, count)
    assert got is not None and got[0] == 0, "%d differences, first at %08x" % (got[0], got[1])


@pytest.mark.skipif(not _f16c(), reason="no F16C on this CPU: no independent f16 conversion to compare with")
def test_f16_to_f32_equals_the_cpu_instruction():
    got = M.accuracy("f16_to_f32", 0, 1 << 16)
    assert got is not None and got[0] == 0, "%d differences, first at %04x" % (got[0], got[1])


# ------------------------------------------------------------------------------------------------- the enumeration itself
def test_op_table_matches_the_header():
    R = M.ref()
    assert [R.math_ref_op_name(k).decode() for k in range(R.math_ref_op_count())] == M.OPS
    assert all(1 <= R.math_ref_op_results(k) <= 8 for k in range(len(M.OPS)))


def _reduced(L):
    return {op: L.math_ref_reduced_checksum(M.OP[op], M.threads()) for op in M.OPS}


@pytest.fixture(scope="module")
def reduced_gxx():
    return _reduced(M.ref())


def test_two_host_compilers_agree(reduced_gxx):
    if not os.path.exists(M.ROCM_CLANGXX):
        pytest.skip("%s not found" % M.ROCM_CLANGXX)
    other = _reduced(M.bind_ref(M.build_ref("libmath_ref_clang.so", compiler=M.ROCM_CLANGXX)))
    assert other == reduced_gxx, [op for op in M.OPS if other[op] != reduced_gxx[op]]


def test_enumeration_is_defined_behaviour(reduced_gxx):
    """The stand-alone program under -fsanitize=undefined,float-cast-overflow exits 0 and prints the checksums of the plain
    build: inside the stated domains (rt_sincos: |x| < 2^31) no conversion or shift of the header is undefined."""
    exe = M.build_ref("math_ref_ubsan", extra=["-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all"], program=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {line.split()[0]: int(line.split()[1], 16) for line in r.stdout.splitlines()}
    assert got == reduced_gxx


def _has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return " fma " in f.read()
    except OSError:
        return False


@pytest.mark.skipif(not _has_fma(), reason="no FMA on this CPU")
def test_sweep_sees_contraction():
    """-ffp-contract=fast -mfma moves the checksum of every op that holds an a * b + c.  Both builds are ROCm's clang++, the
    compiler family of the device side: g++ 11 fuses the scalar expressions but leaves rt_mix3's alone (its products pass
    through rt3 temporaries), so with g++ that op's checksum stays put whatever the inputs are."""
    if not os.path.exists(M.ROCM_CLANGXX):
        pytest.skip("%s not found" % M.ROCM_CLANGXX)
    plain = _reduced(M.bind_ref(M.build_ref("libmath_ref_clang.so", compiler=M.ROCM_CLANGXX)))
    fused = _reduced(M.bind_ref(M.build_ref("libmath_ref_clang_fma.so", compiler=M.ROCM_CLANGXX, extra=["-ffp-contract=fast", "-mfma"])))
    blind = [op for op in ("sincos", "exp", "log", "mix", "dot", "cross", "normalize", "reflect", "refract", "mix3", "mat_mul_point",
                           "mat_mul_dir", "vec_mul_mat_dir") if fused[op] == plain[op]]
    assert not blind, "inputs that cannot tell a fused multiply-add: %s" % blind


def _stats(op, first, count):
    import ctypes
    out = (ctypes.c_uint64 * 8)()
    M.ref().math_ref_stats(M.OP[op], first, count, out)
    return list(out)


@pytest.mark.parametrize("part,want", enumerate([1 << 29, 1 << 29, 30 << 23, 0] * 2))
def test_sincos_domain_size(part, want):
    """Biased exponents 0 .. 157 of both signs, zeros and denormals included: 2 * 158 * 2^23 inputs, counted in eight ranges."""
    assert M.ref().math_ref_in_domain(M.OP["sincos"], part << 29, 1 << 29, M.threads()) == want
    assert sum([1 << 29, 1 << 29, 30 << 23, 0] * 2) == 2 * 158 * (1 << 23)


def test_refract_inputs_take_both_branches():
    n = 1 << 22
    below, above, nan = _stats("refract", 0, n)[:3]                       # from the narrow block: unit-length i and n
    assert below >= n // 10 and above >= n // 10, (below, above, nan)


def test_rgbe8_inputs_reach_every_early_out():
    size = M.ref().math_ref_op_size(M.OP["rgbe8"])
    nonzero, off, tiny, clamped = _stats("rgbe8", 0, size)[:4]
    assert nonzero >= size // 2 and tiny > 0 and clamped > 0, (nonzero, off, tiny, clamped)
    assert abs(off - size // 16) < size // 256, off                       # w == -1 in 1 of 16


@pytest.mark.parametrize("op", ["min", "max"])
def test_min_max_inputs_come_in_both_orders(op):
    lt, gt, general, _ = _stats(op, 0, 1 << 24)[:4]                       # 16 of the 256 classes: one exponent of a, every exponent of b
    lt2, gt2, general2, _ = _stats(op, 0x99 << 20, 1 << 20)[:4]           # equal exponents: sign and mantissa decide
    assert min(lt, gt) * 4 >= general and min(lt2, gt2) * 4 >= general2, (op, lt, gt, general, lt2, gt2, general2)
    specials = M.ref().math_ref_op_size(M.OP[op]) - M.GENERAL
    assert specials == M.N_SPECIAL ** 2 and _stats(op, M.GENERAL, specials)[3] == specials
    assert len({tuple(M.ref_operands(op, M.GENERAL + k)) for k in range(specials)}) == specials   # every ordered pair


def test_pow_table_reaches_every_early_return():
    zp, zz, zn, one, general = _stats("pow", 0, M.ref().math_ref_op_size(M.OP["pow"]))[:5]
    assert zp >= 2 and zz >= 2 and zn >= 2 and one >= 8 and general >= 200, (zp, zz, zn, one, general)


def test_rng_host_side_is_the_oracles(oracle_lib):
    """The bulk RNG exports of the oracle library (the host side of init_rng / rand_pcg in tests/test_gpu_math.py) are its
    one-at-a-time functions, summed the way the device sums."""
    import ctypes
    L = oracle_lib.lib()
    first, count = 0xFFFFFF00, 256                                        # up to the last state
    want = 0
    for s in range(first, first + count):
        state = ctypes.c_uint32(s)
        r = L.oracle_rand_pcg(ctypes.byref(state))
        want += M.f32_bits(r) * (2 * (2 * s) + 1) + state.value * (2 * (2 * s + 1) + 1)
    assert M.ref_sweep("rand_pcg", first, count) == (want % (1 << 64), count)
    assert M.ref_sweep("rand_pcg", first, count + 5) == (want % (1 << 64), count)      # past the end: nothing more
    pixel, frame = M.rng_pairs(1000, 64)
    want = sum(L.oracle_init_rng(pixel[k], frame[k]) * (2 * (1000 + k) + 1) for k in range(64))
    assert M.ref_sweep("init_rng", 1000, 64) == (want % (1 << 64), 64)
    assert [M.ref_value("init_rng", 1000 + k)[0] for k in range(3)] == [L.oracle_init_rng(pixel[k], frame[k]) for k in range(3)]
    pairs = set(zip(*(list(a) for a in M.rng_pairs(0, 1 << 16))))
    assert len(pairs) > 60000 and any(f > 1 << 31 for _, f in pairs) and any(p < 16 for p, _ in pairs)


# ------------------------------------------------------------------------------------------------- the device side builds
def test_device_side_compiles_without_scratch(tmp_path):
    """math_check.hip for gfx950 with the product's flags: it compiles and no check kernel spills (a kernel that spills is
    not running the register-resident code the renderer runs).  Read from the compiler's resource remarks."""
    import kernel_report
    import webgpu_raytracer_amd as W
    if kernel_report.hipcc_missing():
        pytest.skip(kernel_report.hipcc_missing())
    for want in ("-ffp-contract=off", "-fno-fast-math", "-O3", "--offload-arch=gfx950"):
        assert want in W._build.HIP_FLAGS
    kernels = kernel_report.compile_report(M.CHECK_SRC, tmp_path, (M.INCLUDE, M.CSRC))
    checks = {n: res for n, res in kernels.items() if "k_math_check" in n}
    assert len(checks) == len(M.OPS), sorted(kernels)
    for name, res in checks.items():
        assert res["ScratchSize [bytes/lane]"] == 0 and res["VGPRs Spill"] == 0, (name, res)
