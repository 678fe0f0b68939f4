"""Register budget of the kernels that call the block primitives of csrc/k_block_scan.hip.h (force-inlined templates: bloat
would show here): each exists in the compiler's resource report exactly once, uses no scratch memory and spills no VGPR.
No GPU needed."""
import pytest

from test_kernel_resources import resource_report

# (namespace, kernel, template arguments as mangled, or "" for a plain function)
KERNELS = (("rtk", "k_treelet_count", ""), ("rtk", "k_treelet_number", ""), ("rtk", "k_treelet_pick", "ILi0EE"),
           ("rtk", "k_treelet_pick", "ILi1EE"), ("rtk", "k_pair_count", ""), ("rtk", "k_pair_number", ""), ("rtk", "k_scan_counts", ""),
           ("bvhb", "k_scan_blocks", ""), ("bvhb", "k_scan_top", ""), ("bvhb", "k_scan_apply", ""), ("bvhb", "k_big_plan", ""),
           ("wu", "k_emissive_apply", ""))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("scan_resources"))


@pytest.mark.parametrize("ns,name,targs", KERNELS, ids=["%s::%s%s" % k for k in KERNELS])
def test_scan_kernel_has_no_scratch_and_no_spills(kernels, ns, name, targs):
    prefix = "_ZN%d%s%d%s%s" % (len(ns), ns, len(name), name, targs or "E")
    names = [n for n in kernels if n.startswith(prefix)]
    assert len(names) == 1, (prefix, sorted(kernels))
    res = kernels[names[0]]
    print(name, res)
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    assert int(res["VGPRs Spill"]) == 0, res
