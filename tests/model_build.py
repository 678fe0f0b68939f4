"""The one recipe by which the tests build their CPU model libraries and stand-alone check programs (tests/model/*.cpp,
math_check.hip): is the target stale? compile to a name of this process's own, rename into place.  What a target depends on
comes from the compiler (-MMD -MF <out>.d), never from a list kept by hand, and the command is part of freshness: the argv is
stored beside the target (<out>.cmd), as webgpu-raytracer_amd/_build.py stores the flags of the product library."""
import json
import os
import re
import subprocess

CXX = "g++"   # the host compiler of the models


def parse_depfile(text):
    """the prerequisites a make-syntax depfile names: continuation lines joined, `\\ ` a space inside a name, `$$` a dollar"""
    deps = []
    for rule in text.replace("\\\n", " ").splitlines():
        names = re.split(r":(?=\s|$)", rule, maxsplit=1)[-1]
        deps += [n.replace("\\ ", " ").replace("\\#", "#").replace("$$", "$") for n in re.findall(r"(?:\\.|\S)+", names)]
    return deps


def _fresh(out, cmd):
    """the target, its depfile and its command exist, the command is this one, and every file the depfile names exists and is
    no newer than the target (a header that is gone, or a tree that came from another path, is stale, not an error)"""
    try:
        built = os.stat(out).st_mtime_ns
        with open(out + ".cmd") as f:
            if json.load(f) != cmd:
                return False
        with open(out + ".d") as f:
            return all(os.stat(d).st_mtime_ns <= built for d in parse_depfile(f.read()))
    except (OSError, ValueError):
        return False


def build(src, out, flags, compiler=CXX, program=False):
    """Compile `src` to `out` with `compiler` and `flags` (a library's hold -shared, a program's do not) unless `out` is fresh;
    -> out.  Parallel test processes each compile to a name of their own and the renames are atomic, the target last; on a
    failure the temporaries go, the previous target stays and CalledProcessError propagates."""
    assert program != ("-shared" in flags), "a library is linked with -shared, a program with its own main is not"
    cmd = [compiler] + list(flags) + ["-MMD", "-MF", out + ".d", "-o", out, src]
    if _fresh(out, cmd):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = "%s.tmp.%d" % (out, os.getpid())
    try:
        subprocess.run([{out: tmp, out + ".d": tmp + ".d"}.get(a, a) for a in cmd], check=True)
        with open(tmp + ".cmd", "w") as f:
            json.dump(cmd, f)
        for ext in (".d", ".cmd", ""):
            os.replace(tmp + ext, out + ext)
    finally:
        for ext in (".d", ".cmd", ""):
            if os.path.exists(tmp + ext):
                os.remove(tmp + ext)
    return out
