"""Scratch of the wide one-leaf kernel with the per-triangle world records.  Reading the geometric normal and light_pdf's
area and normal from records made at upload time (k_prepare_world_tris) took about 500 instructions out of
k_pathtrace_persistent_wide and, with them, four of its spilled values: 23 VGPR spills and 44 bytes of scratch per lane,
where the kernel had 27 and 48 (tests/test_kernel_resources_wide.py allows 64, its figure of two changes earlier).  This
holds the kernel at the 44 bytes it has now, so that the next change sees it move.  No GPU needed; skipped where hipcc is
absent."""
from test_kernel_resources import resource_report
from test_kernel_resources_wide import WIDE

SCRATCH_CEILING = 44   # bytes per lane at this commit


def test_wide_one_leaf_kernel_keeps_its_scratch(tmp_path):
    kernels = resource_report(tmp_path)
    names = [n for n in kernels if n.startswith(WIDE)]
    assert len(names) == 1, sorted(kernels)
    res = kernels[names[0]]
    assert int(res["Occupancy [waves/SIMD]"]) >= 6, res
    assert int(res["ScratchSize [bytes/lane]"]) <= SCRATCH_CEILING, res
