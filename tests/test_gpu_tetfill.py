"""d3h.tetfill -- the lattice clipped by the linear interpolant of a signed distance, script/get_tet_smpl.py and the FLAGS.tet_smpl start-up of
HmSDFTetsGeometry -- on the MI355X (GPU twins of tests/test_tetfill_emul.py; the restatement, the cases and the
check functions live in tests/tetfill_cases.py)."""
import pytest

import tetfill_cases as TC
import tetfill_startup_cases as TS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', TC.CASES)
def test_gpu_clip_is_the_restatement_and_marching_tets_cut_vertices(gpu, name):
    TC.check_case(gpu, name)


@pytest.mark.parametrize('name', TC.CASES)
def test_gpu_clip_of_negatively_oriented_parents(gpu, name):
    TC.check_flipped(gpu, name)


@pytest.mark.parametrize('name', ('sphere4', 'torus12'))
def test_gpu_clip_counts_a_zero_of_the_field_as_inside(gpu, name):
    TC.check_zeros(gpu, name)


def test_gpu_clip_all_outside_and_all_inside(gpu):
    TC.check_all_outside_all_inside(gpu)


@pytest.mark.parametrize('T', (0, 1, 255, 256, 257))
def test_gpu_clip_of_a_tet_soup(gpu, T):
    TC.check_soup(gpu, T)


def test_gpu_clip_interface(gpu):
    TC.check_interface(gpu)


@pytest.mark.parametrize('name', ('icosphere', 'capsule'))
def test_gpu_fill_mesh(gpu, name):
    TC.check_fill_mesh(gpu, name)


def test_gpu_get_tet_mesh_writes_the_reference_files(gpu, tmp_path):
    TC.check_get_tet_mesh(gpu, tmp_path)


def test_gpu_startup_builds_the_body_tet_mesh(gpu, tmp_path):
    TS.check_startup_attributes(gpu, tmp_path)


@pytest.mark.parametrize('fused', (False, True), ids=('adam', 'fused'))
def test_gpu_smpl_msdf_is_unchanged_by_a_step(gpu, fused):
    TS.check_step_leaves_smpl_msdf(gpu, fused)


def test_gpu_checkpoint_round_trip_restores_smpl_msdf(gpu, tmp_path):
    TS.check_checkpoint(gpu, tmp_path)


def test_gpu_flag_absent_changes_nothing(gpu):
    TS.check_flag_absent(gpu)
