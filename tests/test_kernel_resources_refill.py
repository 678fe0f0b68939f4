"""Register budget of the three one-leaf instances of the persistent path tracer after the tile prepass
(csrc/k_pathtrace_persistent.hip.h, PREPASS: the depth test of a tile's 64 slots at ticket time, the live slots kept as a
lane mask in two scalar registers, the tile's origin packed into one).  Earlier builds of the prepass broke every register
ceiling; this one ends at the parent commit's VGPR counts and scratch on all three instances (the wide form ships with it,
the two 256-thread forms keep the cursor and the parent's code), and this file holds them there:
k_pathtrace_persistent_wide<0,1,1> 80 VGPRs and 28 bytes per lane at 6 waves per SIMD, k_pathtrace_persistent<0,1,1> 90 and
0 at 5 waves, k_pathtrace_persistent<1,1,1> (the counting build) 95 and 0 at the 5 waves the compiler reports for it.
Whether the refill loop of the wide kernel is free of vector loads is not checked here: telling the loop's head and the
ticket branch apart in the assembly needs the compiler's block numbering, which changes with every edit of the kernel.
Reads the compiler's resource report of tests/test_kernel_resources.py.  No GPU needed; skipped where hipcc is absent."""
import pytest

from test_kernel_resources import resource_report

# mangled prefix -> (VGPRs, scratch bytes per lane, waves per SIMD) at this commit; VGPRs and scratch are the parent's too
ONE_LEAF = {
    "_ZN3rtk27k_pathtrace_persistent_wideILb0ELb1ELb1E": (80, 28, 6),
    "_ZN3rtk22k_pathtrace_persistentILb0ELb1ELb1E": (90, 0, 5),
    "_ZN3rtk22k_pathtrace_persistentILb1ELb1ELb1E": (95, 0, 5),
}


@pytest.mark.parametrize("prefix", sorted(ONE_LEAF))
def test_one_leaf_instances_hold_their_registers_with_the_tile_prepass(tmp_path, prefix):
    vgprs, scratch, waves = ONE_LEAF[prefix]
    kernels = resource_report(tmp_path)
    names = [n for n in kernels if n.startswith(prefix)]
    assert len(names) == 1, sorted(kernels)
    res = kernels[names[0]]
    assert int(res["VGPRs"]) <= vgprs, res
    assert int(res["ScratchSize [bytes/lane]"]) <= scratch, res
    assert int(res["Occupancy [waves/SIMD]"]) >= waves, res
