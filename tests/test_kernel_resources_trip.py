"""Register budget of the wide one-leaf kernel after the trip was reordered (csrc/k_pathtrace_persistent.hip.h: one surface
pass per trip at the head of the shade section, the camera read as new where a sample starts, the instance index read from
the TLAS leaf).  The surface frame then lives inside one section of the trip and no longer across the walks, and the kernel
spills less: this holds k_pathtrace_persistent_wide at the scratch it has at this commit and at 6 waves per SIMD, so that a
change which brings the spills back shows up here (tests/test_kernel_resources_wide.py keeps the older, wider ceiling).
Reads the compiler's resource report of tests/test_kernel_resources.py.  No GPU needed; skipped where hipcc is absent."""
from test_kernel_resources import resource_report

WIDE = "_ZN3rtk27k_pathtrace_persistent_wide"
SCRATCH_CEILING = 28   # bytes per lane at this commit (44 at its parent)


def test_wide_one_leaf_kernel_scratch_after_the_one_pass_trip(tmp_path):
    kernels = resource_report(tmp_path)
    names = [n for n in kernels if n.startswith(WIDE)]
    assert len(names) == 1, sorted(kernels)
    res = kernels[names[0]]
    assert int(res["Occupancy [waves/SIMD]"]) >= 6, res
    assert int(res["VGPRs"]) <= 80, res
    assert int(res["ScratchSize [bytes/lane]"]) <= SCRATCH_CEILING, res
