"""The irradiance-gather kernels (k_irradiance_gather<DETAIL, LDS>) under their older test names.  Nothing is stated here: every bound and every kernel name is in tests/kernel_budgets.py and
every check in tests/test_kernel_budgets.py.  One pull request may retire only so many tests, so these names stay until the
next one deletes this file; a new kernel gets a row in the table, not a test here."""
import pytest

from test_kernel_budgets import check_family, check_twins, report  # noqa: F401 (report is a fixture)


def test_all_four_instantiations_exist(report):
    check_family(report, "rtk::k_irradiance_gather<*>")


@pytest.mark.parametrize("lds", ["false", "true"], ids=["False", "True"])
@pytest.mark.parametrize("detail", ["false", "true"], ids=["False", "True"])
def test_gather_kernel_budget_against_its_twin(report, detail, lds):
    check_twins(report, "rtk::k_irradiance_gather<%s, %s>" % (detail, lds))
