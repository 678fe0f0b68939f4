"""Register budget of the wide one-leaf kernel.  k_pathtrace_persistent_wide (csrc/k_pathtrace.hip.h) is the one-leaf-TLAS LDS
form of the product build in 512-thread workgroups, compiled for RT_PT_WIDE_WAVES = 6 waves per SIMD, which leaves it 80
VGPRs.  It does not fit them yet: it spills to scratch, and measures faster than the 5-wave form all the same (DESIGN.md
section 4.1).  This reads the compiler's resource report (tests/test_kernel_resources.py) and holds the kernel at 6 waves and
at most the scratch it has now, so that a change which adds spills shows up here.  No GPU needed; skipped where hipcc is
absent."""
from test_kernel_resources import resource_report

WIDE = "_ZN3rtk27k_pathtrace_persistent_wide"
SCRATCH_CEILING = 64   # bytes per lane at this commit


def test_wide_one_leaf_kernel_holds_six_waves(tmp_path):
    kernels = resource_report(tmp_path)
    names = [n for n in kernels if n.startswith(WIDE)]
    assert len(names) == 1, sorted(kernels)
    res = kernels[names[0]]
    assert int(res["Occupancy [waves/SIMD]"]) >= 6, res
    assert int(res["VGPRs"]) <= 80, res
    assert int(res["ScratchSize [bytes/lane]"]) <= SCRATCH_CEILING, res
