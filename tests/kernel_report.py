"""The one compile-and-parse path of the compiler's resource report (hipcc -Rpass-analysis=kernel-resource-usage): VGPRs,
SGPRs, spills, scratch, waves per SIMD and LDS of every kernel of a source, keyed by the kernel's readable name
(`rtk::k_ray_query<true, false, 3>`).  tests/test_kernel_budgets.py holds the library's report to tests/kernel_budgets.py,
tools/kernel_resources.py prints it, and the tests that compile a source of their own call compile_report.  Device code only,
no assembly is read, no GPU and no external demangler needed.  Where hipcc is absent compile_report raises; the tests ask
hipcc_missing() first and skip."""
import os
import re
import subprocess

import webgpu_raytracer_amd as W

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "webgpu-raytracer_amd", "csrc")
_reports = {}   # (kernel_source_hash(), extra flags) -> report: the library's sources compile once per process


def readable_name(mangled):
    """`_ZN3rtk11k_ray_queryILb1ELb0ELi3EEEv...` -> `rtk::k_ray_query<true, false, 3>`: the mangled prefix is `_Z`, one
    `<len><name>` component or `N` and several, an optional `I...E` list of literal template arguments (Lb0E / Lb1E, Li<n>E,
    Lj<n>E) and, for a nested name, `E`; the parameter types behind it are ignored.  A name without `_Z` (extern "C") is
    its own readable name; anything else this cannot parse is a ValueError."""
    if not mangled.startswith("_Z"):
        if re.fullmatch(r"[A-Za-z_]\w*", mangled):
            return mangled
        raise ValueError("not a kernel name: %r" % mangled)
    nested = mangled.startswith("_ZN")
    pos, parts, args = (3 if nested else 2), [], None
    while True:
        m = re.compile(r"\d+").match(mangled, pos)
        if not m:
            break
        pos = m.end() + int(m.group())
        if pos > len(mangled):
            raise ValueError("component runs past the end of %r" % mangled)
        parts.append(mangled[m.end():pos])
        if not nested:
            break
    if not parts:
        raise ValueError("no name component in %r" % mangled)
    if mangled.startswith("I", pos):
        args, pos = [], pos + 1
        while not mangled.startswith("E", pos):
            m = re.compile(r"L([bij])(n?\d+)E").match(mangled, pos)
            if not m:
                raise ValueError("template argument at %d of %r is no bool, int or unsigned literal" % (pos, mangled))
            kind, digits = m.groups()
            if kind == "b" and digits not in ("0", "1"):
                raise ValueError("bool literal %s in %r" % (digits, mangled))
            args.append(("false", "true")[int(digits)] if kind == "b" else digits.replace("n", "-") + ("u" if kind == "j" else ""))
            pos = m.end()
        pos += 1
    if nested:
        if not mangled.startswith("E", pos):
            raise ValueError("nested name of %r does not close at %d" % (mangled, pos))
    return "::".join(parts) + ("<%s>" % ", ".join(args) if args is not None else "")


def parse_report(stderr):
    """{readable name: {remark key: value}} of the remarks in a compiler's stderr.  Numeric values are ints, `Dynamic Stack`
    stays a string, and the mangled name is kept as entry["mangled"] for messages."""
    kernels, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            mangled = text.split(":", 1)[1].strip()
            cur = kernels.setdefault(readable_name(mangled), {"mangled": mangled})
            assert cur["mangled"] == mangled, "two kernels read as %s: %s, %s" % (readable_name(mangled), cur["mangled"], mangled)
        elif cur is not None and ":" in text:
            k, v = (s.strip() for s in text.split(":", 1))
            cur[k] = int(v) if re.fullmatch(r"-?\d+", v) else v
    return kernels


def hipcc_missing():
    """Why no report can be compiled here, or None."""
    return None if os.path.exists(W._build.HIPCC) else "hipcc not found at %s" % W._build.HIPCC


def compile_report(source, workdir, include_dirs=(), extra_flags=(), timeout=None):
    """The resource report of `source` compiled for gfx950 with the product's flags (`_build.HIP_FLAGS` without -shared and
    -fPIC), device code only; the object file goes to `workdir`."""
    hipcc = W._build.HIPCC
    if hipcc_missing():
        raise FileNotFoundError(hipcc_missing())
    flags = [f for f in W._build.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [hipcc] + flags + list(extra_flags) + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage"]
    for d in include_dirs:
        cmd += ["-I", str(d)]
    cmd += ["-o", os.path.join(str(workdir), os.path.basename(str(source)) + ".o"), str(source)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]
    return parse_report(r.stderr)


def library_report(workdir, extra_flags=()):
    """compile_report of the library (csrc/rt_api.hip), once per process and state of the kernel sources."""
    key = (W._build.kernel_source_hash(), tuple(extra_flags))
    if key not in _reports:
        _reports[key] = compile_report(os.path.join(CSRC, "rt_api.hip"), workdir, (W._build.INCLUDE,), extra_flags)
    return _reports[key]

