"""The ray-query kernels (k_ray_query<ANY, DETAIL, FORM>) under their older test names.  Nothing is stated here: every bound and every kernel name is in tests/kernel_budgets.py and
every check in tests/test_kernel_budgets.py.  One pull request may retire only so many tests, so these names stay until the
next one deletes this file; a new kernel gets a row in the table, not a test here."""
import pytest

import kernel_budgets as B
from test_kernel_budgets import check_family, check_twins, report  # noqa: F401 (report is a fixture)


def test_all_twenty_instantiations_exist(report):
    check_family(report, "rtk::k_ray_query<*>")


@pytest.mark.parametrize("form", range(5))
@pytest.mark.parametrize("detail", ["false", "true"], ids=["False", "True"])
@pytest.mark.parametrize("any_hit", ["false", "true"], ids=["False", "True"])
def test_ray_query_kernel_budget(report, any_hit, detail, form):
    name = "rtk::k_ray_query<%s, %s, %d>" % (any_hit, detail, form)
    assert not B.violations(B.ROWS["rtk::k_ray_query<*>"], report[name]), report[name]
    check_twins(report, name)
