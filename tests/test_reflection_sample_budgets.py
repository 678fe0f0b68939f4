"""The resource budget of the reflection sampler's kernels.  The sampler is a translation unit of its own
(csrc/reflection_sample.hip), so its kernels are not in the report of csrc/rt_api.hip that tests/test_kernel_budgets.py
reads; this module compiles that unit with the product's flags (tests/kernel_report.py) and holds its report with the same
checker (kernel_budgets.violations): exactly the two instantiations, no spill, no scratch, no LDS, all inlined, and the
VGPR counts of the resource table of DESIGN.md 4.1q.  The library's own report neither gains nor loses a kernel by it.
No GPU needed; skipped where hipcc is absent, as the library's budgets are."""
import os
import re

import pytest

import kernel_budgets as B
import kernel_report as K

KERNELS = ["rtk::k_reflection_sample<false>", "rtk::k_reflection_sample<true>"]
# one thread per query with eight 16-byte taps in flight wants every wave it can get: 64 VGPRs are eight waves per SIMD
LIMITS = dict(B.CLEAN, lds_eq=0, waves_eq=8, no_dynamic_stack=True)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if K.hipcc_missing():
        pytest.skip(K.hipcc_missing())
    return K.compile_report(os.path.join(K.CSRC, "reflection_sample.hip"), tmp_path_factory.mktemp("reflection_sample"),
                            (K.W._build.INCLUDE,))


def test_the_unit_holds_exactly_the_two_forms(report):
    assert sorted(report) == KERNELS


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_is_within_its_budget(report, name):
    assert B.violations(LIMITS, report[name]) == [], report[name]


def test_vgprs_are_the_ones_design_md_states(report):
    design = open(os.path.join(K.REPO, "DESIGN.md")).read()
    section = design[design.index("### 4.1q"):]
    for name in KERNELS:
        m = re.search(r"^\| `%s` \| (\d+) \|" % re.escape(name[len("rtk::"):]), section, flags=re.M)
        assert m, "DESIGN.md 4.1q has no resource row for " + name
        assert report[name][B.FIELDS["vgprs"]] == int(m.group(1)), (name, report[name], m.group(1))


def test_the_library_report_does_not_hold_them(tmp_path_factory):
    """they are held here and nowhere else: a kernel of this family in the library's report would want a row there"""
    if K.hipcc_missing():
        pytest.skip(K.hipcc_missing())
    library = K.library_report(tmp_path_factory.mktemp("kernel_budgets"))
    assert not [n for n in library if "k_reflection_sample" in n]
    assert "reflection_sample.hip" in K.W._build.RT_SOURCES
