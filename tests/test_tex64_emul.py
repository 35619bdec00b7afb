"""The texture MLP and grid encoding against float64, per element and at their edges, on the host emulation of csrc/texmlp.hip (CPU twins of
tests/test_gpu_tex64.py; the cases, the float64 references and the rules live in tests/tex64_cases.py)."""
import pytest

import tex64_cases as TC

_id = lambda t: t.replace(' ', '-')
CASES = [t for g in TC.GROUPS for t in TC.tags(g, 'cpu')]


@pytest.mark.parametrize('tag', CASES, ids=[_id(t) for t in CASES])
def test_emul_tex64_routes_vs_float64(emul, tag):
    TC.run_case(emul, tag)


@pytest.mark.parametrize('group', TC.GROUPS)
def test_emul_tex64_decade_bands_within_three_times_the_float32_reference(emul, group):
    TC.check_group(emul, group)


def test_tex64_inputs_have_the_edges_they_claim():
    TC.check_inputs()


def test_tex64_band_exceptions_stay_below_the_h2_ceiling():
    for (group, tensor), (tops, bar, _) in TC.BAND_RATIO.items():
        assert TC.RATIO < bar <= TC.H2_CEILING and tensor.split('/')[0].split('@')[0] in TC.H2_TENSORS
        for top in tops:
            assert TC.band_bar(group, tensor, top) == bar
    assert TC.band_bar('tails', 'out/1', -1) == TC.RATIO
