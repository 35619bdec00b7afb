"""Marching-tets gradients against float64 and the edges of its ordered compaction, on the MI355X (the cases, the float64 reference and the
bars live in tests/mtets64_cases.py)."""
import pytest

import mtets64_cases as MC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('body,spec', MC.MODES, ids=MC.MODE_IDS)
@pytest.mark.parametrize('name', MC.LATTICE)
def test_gpu_mtets64_lattice_forward_and_vjp_vs_float64(gpu, name, body, spec):
    MC.run_lattice(gpu, name, body, spec)


@pytest.mark.parametrize('body,spec', MC.MODES, ids=MC.MODE_IDS)
def test_gpu_mtets64_output_subsets_differentiated_alone(gpu, body, spec):
    MC.run_subsets(gpu, body, spec)


@pytest.mark.parametrize('body', [False, True], ids=['garment', 'body'])
def test_gpu_mtets64_empty_extraction_and_its_neighbours(gpu, body):
    MC.run_empty(gpu, body)


@pytest.mark.parametrize('group', ['regular', 'degenerate', 'subsets'])
def test_gpu_mtets64_decade_bands_within_three_times_the_float32_oracle(gpu, group):
    MC.check_group(gpu, group)


def test_gpu_mtets64_soup_reaches_every_reachable_row_of_the_case_tables(gpu):
    MC.check_tables(gpu)


@pytest.mark.parametrize('nt', MC.BOUNDARY_NT)
def test_gpu_mtets64_soup_sizes_at_wave_and_workgroup_boundaries(gpu, nt):
    MC.check_boundary(gpu, nt)


@pytest.mark.parametrize('kind', ['every', 'last', 'ends'])
def test_gpu_mtets64_soup_crossing_density(gpu, kind):
    MC.check_density(gpu, kind)


@pytest.mark.parametrize('body', [False, True], ids=['garment', 'body'])
@pytest.mark.parametrize('name', list(MC.SCAN))
def test_gpu_mtets64_scan_paths_forward_and_one_backward(gpu, name, body):
    MC.check_scan(gpu, name, body)
    MC.check_bands(gpu, f'scan-{name}')
