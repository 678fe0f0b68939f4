"""Builds and binds the two sides of the math-header check (tests/model/math_inputs.h):

  tests/model/_build/libmath_ref.so     g++    tests/model/math_ref.cpp    the HOST compilation of include/mi355rt_math.h
  tests/model/_build/libmath_check.so   hipcc  tests/model/math_check.hip  the gfx950 compilation, with the product's flags

and names the first index at which the two disagree (first_difference).  Used by tests/test_math_model.py (CPU) and
tests/test_gpu_math.py (GPU)."""
import ctypes
import os
import struct

import model_build

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
MODEL = os.path.join(HERE, "model")
BUILD = os.path.join(MODEL, "_build")
CSRC = os.path.join(REPO, "webgpu-raytracer_amd", "csrc")
INCLUDE = os.path.join(REPO, "include")
REF_SRC = os.path.join(MODEL, "math_ref.cpp")
CHECK_SRC = os.path.join(MODEL, "math_check.hip")
ROCM_CLANGXX = "/opt/rocm/llvm/bin/clang++"
HOST_FLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-pthread"]

# the ops of tests/model/math_inputs.h in their order (test_math_model.py checks this list against the library's)
OPS = ["sincos", "exp", "log", "pow22", "floor", "f2u32_sat", "f2i32_sat", "f32_to_f16", "unorm8", "abs_sat", "f16_to_f32", "pow2i",
       "min", "max", "clamp", "mix", "pow", "dot", "cross", "length", "normalize", "reflect", "refract", "mix3", "minmax3", "clamp3",
       "div3s", "div3z", "rcp3", "div_pi3", "div33", "mat_mul_point", "mat_mul_dir", "vec_mul_mat_dir", "rgbe8", "resize_coord",
       "bilinear_u8", "init_rng", "rand_pcg"]
RNG_OPS = ("init_rng", "rand_pcg")   # device-only functions of csrc/k_common.hip.h: their host side is the oracle library
OP = {name: k for k, name in enumerate(OPS)}
ACC = {"sin": 0, "cos": 1, "exp": 2, "log": 3, "pow": 4, "unorm8_pow": 5, "f32_to_f16": 6, "f16_to_f32": 7}
GENERAL = 1 << 28       # min / max / clamp / mix: indices below are the hashed classes, the specials block follows
N_SPECIAL = 17
VEC_NARROW = 1 << 24
INTEGER_OPS = ("f2u32_sat", "f2i32_sat", "f32_to_f16", "unorm8", "rgbe8", "resize_coord", "bilinear_u8") + RNG_OPS   # not floats


def f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def canon(op, word):
    """A result word as the checksum sees it: every NaN of a float result is one NaN."""
    return 0x7FC00000 if op not in INTEGER_OPS and (word & 0x7FFFFFFF) > 0x7F800000 else word


class Report(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("in_domain", ctypes.c_uint64), ("checksum", ctypes.c_uint64), ("value", ctypes.c_uint32 * 8)]


def threads():
    return min(16, len(os.sched_getaffinity(0)))


def build_ref(name="libmath_ref.so", compiler=model_build.CXX, extra=(), program=False):
    """math_ref.cpp as a shared library, or with program=True as the stand-alone program with its own main()."""
    kind = ["-DMATH_REF_MAIN"] if program else ["-shared", "-fPIC"]
    return model_build.build(REF_SRC, os.path.join(BUILD, name), HOST_FLAGS + list(extra) + kind, compiler, program)


def check_flags(flags):
    return list(flags) + ["-I", INCLUDE, "-I", CSRC]


def build_check(build):
    """math_check.hip with exactly the product's compiler and flags (`build` is webgpu_raytracer_amd._build)."""
    try:
        return model_build.build(CHECK_SRC, os.path.join(BUILD, "libmath_check.so"), check_flags(build.HIP_FLAGS), build.HIPCC)
    except FileNotFoundError:
        raise RuntimeError("hipcc not found at %s: the device side of the math check cannot be built" % build.HIPCC)


def bind_ref(path):
    L = ctypes.CDLL(path)
    u64, u32p = ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)
    L.math_ref_op_count.restype = ctypes.c_int
    L.math_ref_op_name.argtypes = [ctypes.c_int]
    L.math_ref_op_name.restype = ctypes.c_char_p
    L.math_ref_op_results.argtypes = [ctypes.c_int]
    L.math_ref_op_results.restype = ctypes.c_int
    L.math_ref_op_size.argtypes = [ctypes.c_int]
    L.math_ref_op_size.restype = u64
    for f in (L.math_ref_checksum, L.math_ref_in_domain):
        f.argtypes = [ctypes.c_int, u64, u64, ctypes.c_int]
        f.restype = u64
    L.math_ref_sweep.argtypes = [ctypes.c_int, u64, u64, ctypes.c_int, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.math_ref_sweep.restype = None
    for f in (L.math_ref_value, L.math_ref_operands):
        f.argtypes = [ctypes.c_int, u64, u32p]
        f.restype = ctypes.c_int
    L.math_ref_rng_pairs.argtypes = [u64, u64, u32p, u32p]
    L.math_ref_rng_pairs.restype = None
    L.math_ref_reduced_checksum.argtypes = [ctypes.c_int, ctypes.c_int]
    L.math_ref_reduced_checksum.restype = u64
    L.math_ref_stats.argtypes = [ctypes.c_int, u64, u64, ctypes.POINTER(u64)]
    L.math_ref_stats.restype = None
    L.math_ref_accuracy.argtypes = [ctypes.c_int, u64, u64, ctypes.c_int, ctypes.POINTER(ctypes.c_double), u32p,
                                    ctypes.POINTER(ctypes.c_double)]
    L.math_ref_accuracy.restype = ctypes.c_int
    return L


_ref = None


def ref():
    global _ref
    if _ref is None:
        _ref = bind_ref(build_ref())
    return _ref


def bind_check(path):
    L = ctypes.CDLL(path)
    L.math_check.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(Report)]
    L.math_check.restype = ctypes.c_int
    return L


def device_check(D, op, first, count):
    rep = Report()
    rc = D.math_check(OP[op], first, count, ctypes.byref(rep))
    assert rc == 0, "math_check(%s, %d, %d): HIP error %d" % (op, first, count, rc)
    return rep


def rng_pairs(first, count):
    pixel, frame = (ctypes.c_uint32 * count)(), (ctypes.c_uint32 * count)()
    ref().math_ref_rng_pairs(first, count, pixel, frame)
    return pixel, frame


def _oracle():
    import oracle_lib
    return oracle_lib.lib()


def _rng_sweep(op, first, count):
    """The host side of the two RNG ops: Oracle::init_rng / rand_pcg through the oracle library's bulk exports."""
    import numpy as np
    if op == "rand_pcg":
        count = max(0, min(first + count, 1 << 32) - first)
        return _oracle().oracle_rand_pcg_checksum(first, count, threads()), count
    count = max(0, min(first + count, 1 << 20) - first)
    if count == 0:
        return 0, 0
    pixel, frame = rng_pairs(first, count)
    out = (ctypes.c_uint32 * count)()
    _oracle().oracle_init_rng_array(pixel, frame, count, out)
    k = np.arange(first, first + count, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int((np.frombuffer(out, dtype=np.uint32).astype(np.uint64) * (k * np.uint64(2) + np.uint64(1))).sum(dtype=np.uint64)), count


def ref_sweep(op, first, count):
    """(checksum, in-domain count) of the host side over [first, first + count)."""
    if op in RNG_OPS:
        return _rng_sweep(op, first, count)
    s, n = ctypes.c_uint64(), ctypes.c_uint64()
    ref().math_ref_sweep(OP[op], first, count, threads(), ctypes.byref(s), ctypes.byref(n))
    return s.value, n.value


def ref_value(op, i):
    if op == "init_rng":
        pixel, frame = rng_pairs(i, 1)
        return [_oracle().oracle_init_rng(pixel[0], frame[0])] if i < (1 << 20) else []
    if op == "rand_pcg":
        state = ctypes.c_uint32(i & 0xFFFFFFFF)
        r = _oracle().oracle_rand_pcg(ctypes.byref(state))
        return [f32_bits(r), state.value] if i < (1 << 32) else []
    w = (ctypes.c_uint32 * 8)()
    n = ref().math_ref_value(OP[op], i, w)
    return list(w[:n])


def ref_operands(op, i):
    if op == "init_rng":
        pixel, frame = rng_pairs(i, 1)
        return [pixel[0], frame[0]]
    if op == "rand_pcg":
        return [i & 0xFFFFFFFF]
    o = (ctypes.c_uint32 * 28)()
    n = ref().math_ref_operands(OP[op], i, o)
    return list(o[:n])


def accuracy(fn, first, count):
    """(max error or count, input bits where, auxiliary figure) of math_ref_accuracy; None if this host has no F16C."""
    mx, arg, aux = ctypes.c_double(), ctypes.c_uint32(), ctypes.c_double()
    rc = ref().math_ref_accuracy(ACC[fn], first, count, threads(), ctypes.byref(mx), ctypes.byref(arg), ctypes.byref(aux))
    if rc == -2:
        return None
    assert rc == 0
    return mx.value, arg.value, aux.value


def first_difference(D, op, first, count):
    """The first index of [first, first + count) whose device results differ from the host's, as a message.  Checksums add
    over index ranges, so this halves the range: at most 33 more device calls, and only after a mismatch."""
    lo, n = first, count
    while n > 1:
        half = n // 2
        rep = device_check(D, op, lo, half)
        if (rep.checksum, rep.in_domain) == ref_sweep(op, lo, half):
            lo, n = lo + half, n - half
        else:
            n = half
    rep = device_check(D, op, lo, 1)
    host = ref_value(op, lo)
    dev = list(rep.value[:max(len(host), 1)]) if rep.in_domain else []
    words = lambda ws: " ".join("%08x" % w for w in ws) or "(outside the domain)"
    return "%s: first difference at index %d: operands %s; device %s; host %s" % (op, lo, words(ref_operands(op, lo)), words(dev), words(host))
