"""Register budget of the plain form of the wide one-leaf path tracer (k_pathtrace_persistent_plain, csrc/k_pathtrace.hip.h:
shade_bounce and setup_surface without the GGX and dielectric branches, the texture fetches and the emissive length, for
scenes the host has seen to hold untextured Lambertian triangles and lights only).  The generic wide form spills 13 VGPRs to
28 bytes of scratch per lane at its 80-VGPR budget, and 19 of its scratch loads and stores lie inside the trip loop; without
the registers of the code it never runs, the plain form holds 80 VGPRs with no VGPR spill and no scratch at 6 waves per SIMD.
This holds it there.  Reads the compiler's resource report of tests/test_kernel_resources.py.  No GPU needed; skipped where
hipcc is absent."""
from test_kernel_resources import resource_report

PLAIN = "_ZN3rtk28k_pathtrace_persistent_plain"
WIDE = "_ZN3rtk27k_pathtrace_persistent_wide"


def _one(kernels, prefix):
    names = [n for n in kernels if n.startswith(prefix)]
    assert len(names) == 1, sorted(kernels)
    return names[0], kernels[names[0]]


def test_plain_form_is_the_product_one_leaf_instance_alone(tmp_path):
    name, _ = _one(resource_report(tmp_path), PLAIN)
    assert name.startswith(PLAIN + "ILb0ELb1ELb1E"), name


def test_plain_form_runs_at_six_waves_without_scratch(tmp_path):
    _, res = _one(resource_report(tmp_path), PLAIN)
    assert int(res["Occupancy [waves/SIMD]"]) >= 6, res
    assert int(res["VGPRs"]) <= 80, res
    assert int(res["VGPRs Spill"]) == 0, res
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res


def test_plain_form_shares_the_wide_forms_launch(tmp_path):
    """The host launches either kernel with the same workgroups and dynamic LDS: neither may have static LDS of its own,
    and both must fit six waves per SIMD."""
    kernels = resource_report(tmp_path)
    for prefix in (PLAIN, WIDE):
        _, res = _one(kernels, prefix)
        assert int(res["LDS Size [bytes/block]"]) == 0, res
        assert int(res["Occupancy [waves/SIMD]"]) >= 6, res
