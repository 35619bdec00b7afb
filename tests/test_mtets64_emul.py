"""Marching-tets gradients against float64 and the edges of its ordered compaction, on the host emulation of csrc/marching_tets.hip (CPU twins
of tests/test_gpu_mtets64.py; the cases, the float64 reference and the bars live in tests/mtets64_cases.py).  Of the scan-path soups the
emulation runs the garment pass of `per2` (262 401 tets, 19 s); its body pass (22 s), `segments` (2 097 452 tets) and `edges` (2.16 M edges:
more than a minute each) belong to the GPU file alone."""
import pytest

import mtets64_cases as MC


@pytest.mark.parametrize('body,spec', MC.MODES, ids=MC.MODE_IDS)
@pytest.mark.parametrize('name', MC.LATTICE)
def test_emul_mtets64_lattice_forward_and_vjp_vs_float64(emul, name, body, spec):
    MC.run_lattice(emul, name, body, spec)


@pytest.mark.parametrize('body,spec', MC.MODES, ids=MC.MODE_IDS)
def test_emul_mtets64_output_subsets_differentiated_alone(emul, body, spec):
    MC.run_subsets(emul, body, spec)


@pytest.mark.parametrize('body', [False, True], ids=['garment', 'body'])
def test_emul_mtets64_empty_extraction_and_its_neighbours(emul, body):
    MC.run_empty(emul, body)


@pytest.mark.parametrize('group', ['regular', 'degenerate', 'subsets'])
def test_emul_mtets64_decade_bands_within_three_times_the_float32_oracle(emul, group):
    MC.check_group(emul, group)


def test_emul_mtets64_soup_reaches_every_reachable_row_of_the_case_tables(emul):
    MC.check_tables(emul)


@pytest.mark.parametrize('nt', MC.BOUNDARY_NT)
def test_emul_mtets64_soup_sizes_at_wave_and_workgroup_boundaries(emul, nt):
    MC.check_boundary(emul, nt)


@pytest.mark.parametrize('kind', ['every', 'last', 'ends'])
def test_emul_mtets64_soup_crossing_density(emul, kind):
    MC.check_density(emul, kind)


def test_emul_mtets64_scan_two_entries_per_thread(emul):
    MC.check_scan(emul, 'per2', False)
    MC.check_bands(emul, 'scan-per2')


def test_mtets64_band_merging_on_synthetic_counts():
    rows = MC.merged_bands({MC.ZERO_BAND: [10, 1.0, 1.0, 0.0], -3: [100, 1.0, 1.0, 1.0], -2: [5, 1.0, 1.0, 1.0], -1: [70, 1.0, 1.0, 1.0], 0: [3, 1.0, 1.0, 1.0]})
    assert [(lab, r[0]) for lab, r in rows] == [('0 .. 1e-2', 110), ('1e-2 .. 1e1', 78)]
    assert MC.merged_bands({2: [3, 1.0, 1.0, 1.0]})[0][1][0] == 3
