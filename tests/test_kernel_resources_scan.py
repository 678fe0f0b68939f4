"""The callers of the block primitives of csrc/k_block_scan.hip.h under their older test names.  Nothing is stated here: every bound and every kernel name is in tests/kernel_budgets.py and
every check in tests/test_kernel_budgets.py.  One pull request may retire only so many tests, so these names stay until the
next one deletes this file; a new kernel gets a row in the table, not a test here."""
import pytest

from test_kernel_budgets import check_row, report  # noqa: F401 (report is a fixture)

# the older case name -> the row
KERNELS = {"rtk::k_treelet_count": "rtk::k_treelet_count", "rtk::k_treelet_number": "rtk::k_treelet_number",
           "rtk::k_treelet_pickILi0EE": "rtk::k_treelet_pick<0>", "rtk::k_treelet_pickILi1EE": "rtk::k_treelet_pick<1>",
           "rtk::k_pair_count": "rtk::k_pair_count", "rtk::k_pair_number": "rtk::k_pair_number", "rtk::k_scan_counts": "rtk::k_scan_counts",
           "bvhb::k_scan_blocks": "bvhb::k_scan_blocks", "bvhb::k_scan_top": "bvhb::k_scan_top", "bvhb::k_scan_apply": "bvhb::k_scan_apply",
           "bvhb::k_big_plan": "bvhb::k_big_plan", "wu::k_emissive_apply": "wu::k_emissive_apply"}


@pytest.mark.parametrize("row", KERNELS.values(), ids=list(KERNELS))
def test_scan_kernel_has_no_scratch_and_no_spills(report, row):
    check_row(report, row)
