"""Register budget of the probe-visibility kernels (k_visibility_rays / _texels / _tiles and k_volume_sample_visible,
csrc/k_volume_visibility.hip.h): each exists once in the compiler's resource report of the gfx950 code object, uses no scratch
memory, spills no VGPR and declares no LDS, and the sampler - eight lanes per point, the hot one - reaches the waves per SIMD
its VGPR count implies (512 registers per lane and SIMD, allocated in steps of 8, at most 8 waves): nothing else, an LDS
allocation or a launch bound, holds it lower.  The count itself is recorded in DESIGN.md section 4.1p, not gated.  The ray work
of a bake is the ray query's, which tests/test_kernel_resources_ray_query.py holds to its budget.  No GPU needed."""
import pytest

from test_kernel_resources import resource_report

KERNELS = ("k_visibility_rays", "k_visibility_texels", "k_volume_sample_visible", "k_visibility_tiles")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("volume_visibility_resources"))


def _one(kernels, name):
    names = [n for n in kernels if n.startswith("_ZN3rtk%d%sE" % (len(name), name))]
    assert len(names) == 1, (name, sorted(kernels))
    return kernels[names[0]]


@pytest.mark.parametrize("name", KERNELS)
def test_visibility_kernel_has_no_scratch_no_spills_and_no_lds(kernels, name):
    res = _one(kernels, name)
    print(name, res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0, res
    assert int(res["LDS Size [bytes/block]"]) == 0, res


def test_the_visible_sampler_runs_at_the_occupancy_of_its_registers(kernels):
    res = _one(kernels, "k_volume_sample_visible")
    vgprs = int(res["VGPRs"]) + int(res.get("AGPRs", 0))
    allocated = max(8, (vgprs + 7) // 8 * 8)
    implied = min(8, 512 // allocated)
    print("k_volume_sample_visible: VGPRs", vgprs, "allocated", allocated, "waves per SIMD", res["Occupancy [waves/SIMD]"])
    assert int(res["Occupancy [waves/SIMD]"]) == implied, res
