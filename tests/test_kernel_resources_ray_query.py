"""Register budget of the ray-query kernels (k_ray_query<ANY, DETAIL, FORM>, csrc/k_rayquery.hip.h): all 20 instantiations
exist, none spills or uses scratch memory, and each runs at no fewer waves per SIMD than the wavefront trace kernel of the
same form (k_wf_trace / k_wf_trace_pairs<ANY, DETAIL, LDS, 256[, RAYREG]>) in the same compiler report.  No GPU needed."""
import pytest

from test_kernel_resources import resource_report

# FORM -> the wavefront kernel of the same form: (pairs, LDS, RAYREG)
FORMS = {0: (False, True, False), 1: (False, False, False), 2: (False, False, True), 3: (True, True, False), 4: (True, False, False)}


def _b(x):
    return "Lb1E" if x else "Lb0E"


def _wf_name(any_hit, detail, pairs, lds, rayreg):
    if pairs:
        return "_ZN3rtk16k_wf_trace_pairsI%s%s%sLi256EEE" % (_b(any_hit), _b(detail), _b(lds))
    return "_ZN3rtk10k_wf_traceI%s%s%sLi256E%sEE" % (_b(any_hit), _b(detail), _b(lds), _b(rayreg))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return resource_report(tmp_path_factory.mktemp("rq_resources"))


def _one(kernels, prefix):
    names = [n for n in kernels if n.startswith(prefix)]
    assert len(names) == 1, (prefix, names)
    return kernels[names[0]]


def test_all_twenty_instantiations_exist(kernels):
    assert len([n for n in kernels if n.startswith("_ZN3rtk11k_ray_queryI")]) == 20


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("detail", [False, True])
@pytest.mark.parametrize("any_hit", [False, True])
def test_ray_query_kernel_budget(kernels, any_hit, detail, form):
    res = _one(kernels, "_ZN3rtk11k_ray_queryI%s%sLi%dEEE" % (_b(any_hit), _b(detail), form))
    assert int(res["VGPRs Spill"]) == 0, res
    assert int(res["SGPRs Spill"]) == 0, res
    assert int(res["ScratchSize [bytes/lane]"]) == 0, res
    wf = _one(kernels, _wf_name(any_hit, detail, *FORMS[form]))
    assert int(res["Occupancy [waves/SIMD]"]) >= int(wf["Occupancy [waves/SIMD]"]), (res, wf)
