"""The build recipe of the CPU model libraries (tests/model_build.py) on tiny sources of its own: a .cpp that includes a.h,
which includes b.h.  What makes a target stale (a newer header however deep, a header that is gone, another command), what
does not (a header the source no longer includes), what a failed build leaves behind, a program beside the libraries, and
the depfile parser on make syntax no compiler here happens to emit.  Host compiler only, no GPU."""
import ctypes
import os
import subprocess

import pytest

import model_build

FLAGS = ["-O0", "-shared", "-fPIC"]
WITH_HEADERS = '#include "a.h"\nextern "C" int answer() { return A + B; }\n'
WITHOUT = 'extern "C" int answer() { return 7; }\n'


@pytest.fixture
def tree(tmp_path):
    (tmp_path / "b.h").write_text("#define B 2\n")
    (tmp_path / "a.h").write_text('#include "b.h"\n#define A 40\n')
    (tmp_path / "m.cpp").write_text(WITH_HEADERS)
    return tmp_path, str(tmp_path / "m.cpp"), str(tmp_path / "out" / "libm.so")


def identity(path):
    st = os.stat(path)
    return st.st_ino, st.st_mtime_ns


def later_than(target, path, seconds=2):
    t = os.stat(target).st_mtime + seconds
    os.utime(path, (t, t))


def test_builds_and_loads_then_leaves_a_fresh_target_alone(tree):
    _, src, out = tree
    assert model_build.build(src, out, FLAGS) == out
    assert ctypes.CDLL(out).answer() == 42
    before = identity(out)
    assert model_build.build(src, out, FLAGS) == out
    assert identity(out) == before


def test_a_newer_header_of_a_header_rebuilds(tree):
    d, src, out = tree
    before = identity(model_build.build(src, out, FLAGS))
    (d / "b.h").write_text("#define B 3\n")
    later_than(out, d / "b.h")
    assert identity(model_build.build(src, out, FLAGS))[0] != before[0]
    assert ctypes.CDLL(out).answer() == 43


def test_a_header_no_longer_included_may_go(tree):
    d, src, out = tree
    before = identity(model_build.build(src, out, FLAGS))
    (d / "m.cpp").write_text(WITHOUT)
    later_than(src, out, seconds=-2)      # the target is older than its source, and the next one will not be
    rebuilt = identity(model_build.build(src, out, FLAGS))
    assert rebuilt[0] != before[0]
    os.remove(d / "a.h")
    assert identity(model_build.build(src, out, FLAGS)) == rebuilt


def test_a_deleted_header_the_depfile_names_is_stale_not_an_error(tree):
    d, src, out = tree
    before = identity(model_build.build(src, out, FLAGS))
    (d / "m.cpp").write_text(WITHOUT)
    later_than(out, src, seconds=-2)      # the source is no newer than the target: only the missing header says stale
    os.remove(d / "a.h")
    assert "a.h" in open(out + ".d").read()
    assert identity(model_build.build(src, out, FLAGS))[0] != before[0]
    assert ctypes.CDLL(out).answer() == 7


def test_another_flag_rebuilds(tree):
    _, src, out = tree
    before = identity(model_build.build(src, out, FLAGS))
    assert identity(model_build.build(src, out, FLAGS + ["-DX=1"]))[0] != before[0]
    again = identity(out)
    assert identity(model_build.build(src, out, FLAGS + ["-DX=1"])) == again


def test_a_failed_build_leaves_the_previous_target_and_nothing_else(tree):
    d, src, out = tree
    model_build.build(src, out, FLAGS)
    before = open(out, "rb").read()
    (d / "m.cpp").write_text("this is not C++\n")
    later_than(out, src)
    with pytest.raises(subprocess.CalledProcessError):
        model_build.build(src, out, FLAGS)
    assert open(out, "rb").read() == before
    assert sorted(os.listdir(os.path.dirname(out))) == ["libm.so", "libm.so.cmd", "libm.so.d"]


def test_a_program_runs(tree):
    d, _, out = tree
    (d / "p.cpp").write_text('#include "a.h"\nint main() { return A + B - 42; }\n')
    exe = model_build.build(str(d / "p.cpp"), os.path.join(os.path.dirname(out), "p"), ["-O0"], program=True)
    assert subprocess.run([exe], timeout=60).returncode == 0


def test_depfile_syntax():
    text = "out/lib\\ m.so: src/m.cpp \\\n /some\\ where/a.h \\\n  b.h\\\n c$$d.h\n"
    assert model_build.parse_depfile(text) == ["src/m.cpp", "/some where/a.h", "b.h", "c$d.h"]
    assert model_build.parse_depfile("m.o:\n") == []
    assert model_build.parse_depfile("m.o: a.h\n\na.h:\n") == ["a.h"]
