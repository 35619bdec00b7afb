"""Stage hand-off, second half -- winding-signed distance, collision push, edge-split refinement, relaxation, watertight extraction -- on the
host emulation of the kernel sources (CPU twins of tests/test_gpu_handoff.py; the check functions, the yardsticks and the mesh generators live in
tests/handoff_cases.py)."""
import pytest
import torch

import handoff_cases as HC


@pytest.mark.parametrize('name', tuple(HC.WSDF_MESHES))
def test_emul_mesh_wsdf_equals_the_float64_yardstick(emul, name):
    HC.check_wsdf(emul, name)


@pytest.mark.parametrize('name', tuple(HC.WSDF_MESHES))
def test_emul_mesh_wsdf_sign_equals_the_float64_yardstick(emul, name):
    HC.check_wsdf_sign(emul, name)


def test_emul_mesh_wsdf_at_the_tile_and_block_edges(emul):
    HC.check_wsdf_tile_and_block_edges(emul)


def test_emul_mesh_wsdf_null_outputs_zero_queries_and_bad_arguments(emul):
    HC.check_wsdf_edges_of_the_interface(emul)


def test_emul_collision_push_counts_and_positions(emul):
    HC.check_push(emul)


def test_emul_refine_one_triangle_all_patterns_and_rotations(emul):
    HC.check_refine_single_triangle_patterns(emul)


def test_emul_refine_shared_edges_degenerate_faces_ties_and_no_ops(emul):
    HC.check_refine_small_cases(emul)


@pytest.mark.parametrize('dtype', (torch.int32, torch.int64), ids=('i32', 'i64'))
def test_emul_refine_strip_of_257(emul, dtype):
    HC.check_refine_strip(emul, dtype)


@pytest.mark.parametrize('masked', (False, True), ids=('all', 'disc'))
def test_emul_refine_jittered_sheet_three_rounds(emul, masked):
    HC.check_refine_sheet(emul, masked)


def test_emul_refine_many_faces_on_one_edge(emul):
    HC.check_refine_contended(emul)


def test_emul_refine_rejects_bad_indices_and_arguments(emul):
    HC.check_refine_rejects(emul)


def test_emul_relax_equals_the_float64_yardstick_and_keeps_fixed_vertices(emul):
    HC.check_relax(emul)


def test_emul_relax_obeys_the_maximum_principle(emul):
    HC.check_relax_maximum_principle(emul)


@pytest.mark.parametrize('name', ('cylinder', 'capsule'))
def test_emul_watertight_closes_an_open_mesh(emul, name):
    HC.check_watertight(emul, name)


def test_emul_script_functions_equal_their_numpy_restatements(emul, tmp_path):
    HC.check_script_functions(emul, tmp_path)


def test_emul_process_body_msdf_distance_bodyedge_on_a_capsule(emul, tmp_path):
    HC.check_whole_function(emul, tmp_path)
