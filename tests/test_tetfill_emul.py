"""d3h.tetfill -- the lattice clipped by the linear interpolant of a signed distance, script/get_tet_smpl.py and the FLAGS.tet_smpl start-up of
HmSDFTetsGeometry -- on the host emulation of the kernel sources (CPU twins of tests/test_gpu_tetfill.py; the restatement, the cases and the
check functions live in tests/tetfill_cases.py)."""
import pytest

import tetfill_cases as TC
import tetfill_startup_cases as TS


@pytest.mark.parametrize('name', TC.CASES)
def test_the_restatement_gives_the_counts_of_the_table_and_a_conforming_solid(name):
    TC.check_restatement_counts(name)


@pytest.mark.parametrize('name', TC.CASES)
def test_emul_clip_is_the_restatement_and_marching_tets_cut_vertices(emul, name):
    TC.check_case(emul, name)


@pytest.mark.parametrize('name', TC.CASES)
def test_emul_clip_of_negatively_oriented_parents(emul, name):
    TC.check_flipped(emul, name)


@pytest.mark.parametrize('name', ('sphere4', 'torus12'))
def test_emul_clip_counts_a_zero_of_the_field_as_inside(emul, name):
    TC.check_zeros(emul, name)


def test_emul_clip_all_outside_and_all_inside(emul):
    TC.check_all_outside_all_inside(emul)


@pytest.mark.parametrize('T', (0, 1, 255, 256, 257))
def test_emul_clip_of_a_tet_soup(emul, T):
    TC.check_soup(emul, T)


def test_emul_clip_interface(emul):
    TC.check_interface(emul)


@pytest.mark.parametrize('name', ('icosphere', 'capsule'))
def test_emul_fill_mesh(emul, name):
    TC.check_fill_mesh(emul, name)


def test_emul_get_tet_mesh_writes_the_reference_files(emul, tmp_path):
    TC.check_get_tet_mesh(emul, tmp_path)


def test_emul_startup_builds_the_body_tet_mesh(emul, tmp_path):
    TS.check_startup_attributes(emul, tmp_path)


@pytest.mark.parametrize('fused', (False, True), ids=('adam', 'fused'))
def test_emul_smpl_msdf_is_unchanged_by_a_step(emul, fused):
    TS.check_step_leaves_smpl_msdf(emul, fused)


def test_emul_checkpoint_round_trip_restores_smpl_msdf(emul, tmp_path):
    TS.check_checkpoint(emul, tmp_path)


def test_emul_flag_absent_changes_nothing(emul):
    TS.check_flag_absent(emul)
