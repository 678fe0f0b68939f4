"""Register budget of the irradiance-volume kernels (k_volume_probes / _finish / _sample / _layers, csrc/k_volume.hip.h): each
exists once in the compiler's resource report of the gfx950 code object, uses no scratch memory, spills no VGPR and declares no
LDS.  The path work of a bake is the probe gather's, which tests/test_kernel_resources_probe.py and _radiance.py hold to their
budgets.  No GPU needed."""
import pytest

from test_kernel_resources import resource_report

KERNELS = ("k_volume_probes", "k_volume_finish", "k_volume_sample", "k_volume_layers")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("volume_resources"))


@pytest.mark.parametrize("name", KERNELS)
def test_volume_kernel_has_no_scratch_no_spills_and_no_lds(kernels, name):
    names = [n for n in kernels if n.startswith("_ZN3rtk%d%sE" % (len(name), name))]
    assert len(names) == 1, (name, sorted(kernels))
    res = kernels[names[0]]
    print(name, res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0, res
    assert int(res["LDS Size [bytes/block]"]) == 0, res
