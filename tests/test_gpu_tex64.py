"""The texture MLP and grid encoding against float64, per element and at their edges, on the MI355X (the cases, the float64 references and the
rules live in tests/tex64_cases.py).  The persistent loops run at the real grid caps here; D3H_TEX_GRID_CAP is never set."""
import pytest

import tex64_cases as TC

pytestmark = pytest.mark.gpu

_id = lambda t: t.replace(' ', '-')
CASES = [t for g in TC.GROUPS for t in TC.tags(g, 'cuda')]
assert not any(TC.SPECS[t].get('cap') for t in CASES)


@pytest.mark.parametrize('tag', CASES, ids=[_id(t) for t in CASES])
def test_gpu_tex64_routes_vs_float64(gpu, tag):
    TC.run_case(gpu, tag)


@pytest.mark.parametrize('group', TC.GROUPS)
def test_gpu_tex64_decade_bands_within_three_times_the_float32_reference(gpu, group):
    TC.check_group(gpu, group)
