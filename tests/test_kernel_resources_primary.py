"""The forms of k_primary_visibility under their older test names.  Nothing is stated here: every bound and every kernel name is in tests/kernel_budgets.py and
every check in tests/test_kernel_budgets.py.  One pull request may retire only so many tests, so these names stay until the
next one deletes this file; a new kernel gets a row in the table, not a test here."""
import pytest

from test_kernel_budgets import check_family, check_row, report  # noqa: F401 (report is a fixture)

FORMS = {"global": "rtk::k_primary_visibility<false, false>", "lds": "rtk::k_primary_visibility<false, true>",
         "lds_tiles": "rtk::k_primary_visibility_tiles<false>", "global_counting": "rtk::k_primary_visibility<true, false>",
         "lds_counting": "rtk::k_primary_visibility<true, true>", "lds_tiles_counting": "rtk::k_primary_visibility_tiles<true>"}


def test_the_primary_kernel_has_these_six_forms(report):
    check_family(report, "rtk::k_primary_visibility<*>")
    check_family(report, "rtk::k_primary_visibility_tiles<*>")


@pytest.mark.parametrize("form", ["lds_tiles", "lds"])
def test_lds_product_forms_fit_eight_waves_without_spills(report, form):
    check_row(report, FORMS[form])


@pytest.mark.parametrize("form", ["global", "global_counting", "lds_counting", "lds_tiles_counting"])
def test_the_other_forms_keep_eight_waves(report, form):
    check_row(report, FORMS[form])
