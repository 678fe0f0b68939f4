"""The owners of the host API's HIP resources (csrc/device_owned.h): device buffers, events, event pairs, streams and pinned
host blocks.  rt_destroy and the failure paths of rt_create are `delete` and nothing else, so a wrong owner is a leak or a
double free in every context.  tests/model/owned_check.cpp includes the header unchanged over stand-ins for the HIP names,
backed by malloc / free and counting calls, and checks every owner: an empty one frees nothing, destruction and a repeated
reset() free once, moves transfer ownership and free the overwritten target once, nothing copies, a deque of pairs balances,
and members go in reverse order of declaration.  It is a program of its own, built with the host compiler and the address and
undefined-behaviour sanitizers linked in, and run once (no GPU)."""
import os
import subprocess

import model_build

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "webgpu-raytracer_amd", "csrc")
SRC = os.path.join(HERE, "model", "owned_check.cpp")
EXE = os.path.join(HERE, "model", "_build", "owned_check")


def test_every_owner_under_the_sanitizers():
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
             "-static-libasan", "-static-libubsan"]
    run = subprocess.run([model_build.build(SRC, EXE, flags, program=True)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip().splitlines()[-1] == "owned_check: every check held, 0 live", run.stdout


def test_the_header_is_host_only():
    """device_owned.h includes no HIP header: the stand-ins of owned_check.cpp are all it sees there."""
    text = open(os.path.join(CSRC, "device_owned.h")).read()
    assert "#include <hip" not in text and "#include \"hip" not in text
    assert "__device__" not in text and "__global__" not in text
