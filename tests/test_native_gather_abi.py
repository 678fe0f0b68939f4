"""CPU-side checks of the sharded-image entry points (rt_dist_*, include/mi355rt.h): exported and bound, RCCL loaded at
run time only (never a NEEDED entry; a missing library is an error code with a message, not an abort), and the two copy
kernels of csrc/k_stripes.hip.h compile for gfx950 without scratch.  No GPU needed."""
import ctypes
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rt_dist_unique_id rt_dist_init rt_dist_shutdown rt_dist_block_bytes rt_pack_stripes rt_dist_read_block "
               "rt_dist_write_block rt_unpack_stripes rt_gather_stripes rt_read_display").split()


def test_new_symbols_are_exported_bound_and_wrapped(W):
    W._build.build_rt()
    from webgpu_raytracer_amd import renderer, distributed
    L = renderer.load_library()
    for n in NEW_SYMBOLS:
        assert n in renderer.EXPORTED_SYMBOLS and getattr(L, n).argtypes is not None, n
    for m in ("distInit", "distShutdown", "distBlockBytes", "packStripes", "readBlock", "writeBlock", "unpackStripes",
              "gatherStripes", "readDisplay"):
        assert callable(getattr(W.WebGPURenderer, m)), m
    for m in ("render", "gather", "read_image", "synchronize", "wire_bytes_per_rank"):
        assert callable(getattr(distributed.NativeShardedImage, m)), m
    blob = open(W._build.RT_LIB, "rb").read()
    assert b"k_pack_stripes" in blob and b"k_unpack_stripes" in blob
    # a NULL context is refused, not dereferenced
    assert L.rt_dist_block_bytes(None) == 0
    for n in ("rt_dist_shutdown", "rt_pack_stripes", "rt_unpack_stripes", "rt_gather_stripes"):
        assert getattr(L, n)(None) == -1, n
    assert L.rt_dist_init(None, 0, 1, 8, None) == -1 and L.rt_dist_unique_id(None) == -1


def test_rccl_is_not_a_link_dependency(W):
    W._build.build_rt()
    from webgpu_raytracer_amd import renderer
    needed = renderer._elf_dynamic_strings(W._build.RT_LIB, (1,))[1]
    assert needed and not [n for n in needed if "rccl" in n.lower() or "nccl" in n.lower()], needed
    if W._build.build_node_addon():
        needed = renderer._elf_dynamic_strings(W._build.NODE_ADDON, (1,))[1]
        assert not [n for n in needed if "rccl" in n.lower()], needed


def test_missing_rccl_is_an_error_code_with_a_message(W, tmp_path):
    """MI355RT_RCCL names a file that is no library: rt_dist_unique_id returns RT_ERR_RCCL, the message names the file, the
    process lives on and the rest of the library still answers.  A fresh process: the library is resolved once per process."""
    W._build.build_rt()
    bad = tmp_path / "librccl_missing.so"
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from webgpu_raytracer_amd import renderer as R\n"
            "L = R.load_library()\n"
            "import ctypes; buf = ctypes.create_string_buffer(128)\n"
            "print('RC', L.rt_dist_unique_id(buf)); print('MSG', L.rt_last_error(None).decode())\n"
            "print('RC2', L.rt_dist_unique_id(buf)); print('COUNT', L.rt_device_count() >= 0)\n" % REPO)
    env = dict(os.environ, MI355RT_RCCL=str(bad))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "RC -6" in out.stdout and "RC2 -6" in out.stdout and "COUNT True" in out.stdout
    assert "librccl_missing.so" in out.stdout and "MI355RT_RCCL" in out.stdout


def test_copy_kernels_use_no_scratch(W, tmp_path):
    """hipcc -Rpass-analysis=kernel-resource-usage on the two kernels alone (the header stands on its own)."""
    import kernel_report
    if kernel_report.hipcc_missing():
        pytest.skip(kernel_report.hipcc_missing())
    src = tmp_path / "stripes.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include "k_stripes.hip.h"\n')
    kernels = kernel_report.compile_report(src, tmp_path, (os.path.join(REPO, "webgpu-raytracer_amd", "csrc"),), timeout=300)
    for want in ("k_pack_stripes", "k_unpack_stripes"):
        names = [n for n in kernels if want in n]
        assert len(names) == 1, sorted(kernels)
        res = kernels[names[0]]
        print(want, res)
        assert res["ScratchSize [bytes/lane]"] == 0 and res["VGPRs Spill"] == 0, res
        assert res["VGPRs"] <= 32, res   # a streaming copy: full occupancy
