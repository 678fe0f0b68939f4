"""Every kernel of the library against its resource budget (tests/kernel_budgets.py) in the compiler's resource report for
gfx950 (tests/kernel_report.py): one compile of the library with the product flags, device code only.  The rows, the relations
between kernels of one report, completeness (every kernel has a row or a reason to have none, every row a kernel), and the
checker itself on fabricated entries.  No GPU needed; the tests that read the report are skipped where hipcc is absent.
The test_kernel_resources_*.py beside this file hold nothing of their own: they keep older test names and call in here."""
import os
import re

import pytest

import kernel_budgets as B
import kernel_report as K


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if K.hipcc_missing():
        pytest.skip(K.hipcc_missing())
    return K.library_report(tmp_path_factory.mktemp("kernel_budgets"))


@pytest.fixture(scope="module")
def design():
    return open(os.path.join(K.REPO, "DESIGN.md")).read()


def family(report, pattern):
    return sorted(n for n in report if B.matching(n, [pattern]))


def check_row(report, row):
    """every kernel the row names (at least one) is within the row's limits"""
    names = family(report, row)
    assert names, "no kernel in the report is named %s" % row
    for name in names:
        bad = B.violations(B.ROWS[row], report[name])
        assert not bad, "%s breaks %s\nrow: %s\nmeasured: %s\nwhy: %s" % (name, bad, B.ROWS[row], report[name], B.ROWS[row]["why"])


def check_family(report, pattern):
    assert family(report, pattern) == sorted(B.FAMILIES[pattern]), pattern


def check_twins(report, kernel=None):
    """the kernel (or every kernel of TWINS) is no worse than its twin in the fields TWINS names"""
    twins = [t for t in B.TWINS if kernel in (None, t[0])]
    assert twins, kernel
    for name, twin, fields in twins:
        for field in fields:
            got, ref = report[name][B.FIELDS[field]], report[twin][B.FIELDS[field]]
            assert (got >= ref if field == "waves" else got <= ref), (field, name, report[name], twin, report[twin])


@pytest.mark.parametrize("row", sorted(B.ROWS))
def test_kernel_is_within_its_budget(report, row):
    check_row(report, row)


def test_families_have_exactly_their_instantiations(report):
    for pattern in B.FAMILIES:
        check_family(report, pattern)


def test_kernels_are_no_worse_than_their_twins(report):
    check_twins(report)


def test_figures_are_the_ones_design_md_states(report, design):
    for name, field, op, row, section in B.DESIGN_FIGURES:
        m = re.search(row, design[design.index(section):] if section else design, flags=re.M)
        assert m, "DESIGN.md has no resource row for " + name
        got, stated = report[name][B.FIELDS[field]], int(m.group(1))
        assert (got == stated if op == "eq" else 0 < got <= stated), (name, field, got, stated)
    for s in (1, 2, 3, 4):   # the window of each spacing: (32 + 4 S) * (8 + 4 S) cells of twelve words
        assert report["rtk::k_frame_pass_lds<%d>" % s][B.FIELDS["lds"]] == (32 + 4 * s) * (8 + 4 * s) * 48


def test_waves_are_what_the_registers_imply(report):
    for name in B.IMPLIED_WAVES:
        res = report[name]
        allocated = max(8, (res["VGPRs"] + res.get("AGPRs", 0) + 7) // 8 * 8)
        assert res[B.FIELDS["waves"]] == min(8, 512 // allocated), (name, res)


def test_every_kernel_has_one_row_or_one_reason_and_every_row_a_kernel(report):
    patterns = list(B.ROWS) + list(B.REFERENCES) + list(B.UNBUDGETED)
    assert len(set(patterns)) == len(patterns)
    for name in report:
        assert len(B.matching(name, patterns)) == 1, (name, B.matching(name, patterns))
    for pattern in patterns:
        assert family(report, pattern), "no kernel in the report is named %s" % pattern
    held = [n for names in B.FAMILIES.values() for n in names] + [t[0] for t in B.TWINS] + [f[0] for f in B.DESIGN_FIGURES]
    for name in held + B.IMPLIED_WAVES:
        assert B.matching(name, B.ROWS), name + " is held by a relation and has no row"
    for _, twin, _ in B.TWINS:
        assert B.matching(twin, B.REFERENCES), twin + " is measured against and is no reference"
    budgeted, reference = (sum(1 for n in report if B.matching(n, which)) for which in (B.ROWS, B.REFERENCES))
    print("kernels %d = budgeted %d + reference only %d + unbudgeted %d"
          % (len(report), budgeted, reference, len(report) - budgeted - reference))


# ------------------------------------------------------------------------------------- the checker, on fabricated entries
ENTRY = {"mangled": "_ZN3rtk6k_fakeEv", "VGPRs": 80, "AGPRs": 0, "TotalSGPRs": 96, "VGPRs Spill": 19, "SGPRs Spill": 5,
         "ScratchSize [bytes/lane]": 44, "Occupancy [waves/SIMD]": 6, "LDS Size [bytes/block]": 160 * 1024 // 3,
         "Dynamic Stack": "False"}
# kind -> (the bound ENTRY meets exactly, the entries one unit past it)
AT_THE_LIMIT = {
    "vgprs_max": (80, [{"VGPRs": 81}]), "vgprs_eq": (80, [{"VGPRs": 81}, {"VGPRs": 79}]), "sgprs_max": (96, [{"TotalSGPRs": 97}]),
    "vgpr_spill_max": (19, [{"VGPRs Spill": 20}]), "sgpr_spill_max": (5, [{"SGPRs Spill": 6}]),
    "scratch_max": (44, [{"ScratchSize [bytes/lane]": 45}]), "waves_min": (6, [{"Occupancy [waves/SIMD]": 5}]),
    "waves_eq": (6, [{"Occupancy [waves/SIMD]": 5}, {"Occupancy [waves/SIMD]": 7}]),
    "lds_eq": (54613, [{"LDS Size [bytes/block]": 54612}, {"LDS Size [bytes/block]": 54614}]),
    "lds_max": (54613, [{"LDS Size [bytes/block]": 54614}]), "lds_min_blocks_per_cu": (3, [{"LDS Size [bytes/block]": 54614}]),
    "no_dynamic_stack": (True, [{"Dynamic Stack": "True"}]),
}


def test_the_checker_tests_cover_every_limit_kind_and_every_kind_in_the_table():
    assert sorted(AT_THE_LIMIT) == sorted(B.KINDS)
    assert {k for row in B.ROWS.values() for k in row} <= set(B.KINDS) | {"why"}
    with pytest.raises(KeyError):
        B.violations({"agprs_max": 0}, ENTRY)


@pytest.mark.parametrize("kind", B.KINDS)
def test_checker_passes_at_the_limit_and_fails_one_unit_over(kind):
    bound, over = AT_THE_LIMIT[kind]
    assert B.violations({kind: bound}, ENTRY) == []
    for change in over:
        bad = B.violations({kind: bound}, dict(ENTRY, **change))
        assert len(bad) == 1 and kind in bad[0], (change, bad)


def test_zero_means_none():
    zero = dict(ENTRY, **{"VGPRs Spill": 0, "SGPRs Spill": 0, "ScratchSize [bytes/lane]": 0, "LDS Size [bytes/block]": 0})
    assert B.violations(dict(B.CLEAN, lds_eq=0), zero) == []
    assert len(B.violations(dict(B.CLEAN, lds_eq=0), ENTRY)) == 4
    assert len(B.violations(dict(lds_min_blocks_per_cu=1), zero)) == 1   # a kernel that lost its LDS is not within it


def test_readable_names_and_names_that_do_not_parse():
    assert K.readable_name("_ZN3rtk11k_ray_queryILb1ELb0ELi3EEEvPKfPfi") == "rtk::k_ray_query<true, false, 3>"
    assert K.readable_name("_ZN4bvhb7k_levelILi256ELb0EEEvPi") == "bvhb::k_level<256, false>"
    assert K.readable_name("_ZN3rtk14k_encode_atlasEPKfPfi") == "rtk::k_encode_atlas"
    assert K.readable_name("_ZN3rtk6k_fakeILj7ELin1EEEvv") == "rtk::k_fake<7u, -1>"
    assert K.readable_name("_Z12k_math_checkILi3EEvyyP11math_report") == "k_math_check<3>"
    assert K.readable_name("k_plain_c") == "k_plain_c"
    for bad in ("_ZN3rtk11k_ray", "_ZN3rtk11k_ray_queryILb2EEEvv", "_ZN3rtk11k_ray_queryIfEEvv", "_ZN3rtk11k_ray_queryILb1E",
                "_ZN3rtk11k_ray_queryPf", "_Z", "_ZNK3rtk1fEv", "not a name"):
        with pytest.raises(ValueError):
            K.readable_name(bad)


def test_parse_report_converts_numbers_once_and_keeps_the_mangled_name():
    remark = "k.hip:1:1: remark: %s [-Rpass-analysis=kernel-resource-usage]\n"
    text = "".join(remark % t for t in ("Function Name: _ZN3rtk6k_fakeEv", "    VGPRs: 80", "    Dynamic Stack: False",
                                        "    LDS Size [bytes/block]: 0"))
    assert K.parse_report(text) == {"rtk::k_fake": {"mangled": "_ZN3rtk6k_fakeEv", "VGPRs": 80, "Dynamic Stack": "False",
                                                    "LDS Size [bytes/block]": 0}}
    with pytest.raises(ValueError):
        K.parse_report(remark % "Function Name: _ZN3rtk6k_fakeIfEEvv")
