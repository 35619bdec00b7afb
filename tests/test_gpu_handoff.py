"""Stage hand-off, second half -- winding-signed distance, collision push, edge-split refinement, relaxation, watertight extraction -- on the
MI355X (GPU twins of tests/test_handoff_emul.py; the check functions, the yardsticks and the mesh generators live in tests/handoff_cases.py).
The emulator runs the threads of a launch one after another: the book, fan and strip cases test the lock-free edge inserts only here."""
import pytest
import torch

import handoff_cases as HC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', tuple(HC.WSDF_MESHES))
def test_gpu_mesh_wsdf_equals_the_float64_yardstick(gpu, name):
    HC.check_wsdf(gpu, name)


@pytest.mark.parametrize('name', tuple(HC.WSDF_MESHES))
def test_gpu_mesh_wsdf_sign_equals_the_float64_yardstick(gpu, name):
    HC.check_wsdf_sign(gpu, name)


def test_gpu_mesh_wsdf_at_the_tile_and_block_edges(gpu):
    HC.check_wsdf_tile_and_block_edges(gpu)


def test_gpu_mesh_wsdf_null_outputs_zero_queries_and_bad_arguments(gpu):
    HC.check_wsdf_edges_of_the_interface(gpu)


def test_gpu_collision_push_counts_and_positions(gpu):
    HC.check_push(gpu)


def test_gpu_refine_one_triangle_all_patterns_and_rotations(gpu):
    HC.check_refine_single_triangle_patterns(gpu)


def test_gpu_refine_shared_edges_degenerate_faces_ties_and_no_ops(gpu):
    HC.check_refine_small_cases(gpu)


@pytest.mark.parametrize('dtype', (torch.int32, torch.int64), ids=('i32', 'i64'))
def test_gpu_refine_strip_of_257(gpu, dtype):
    HC.check_refine_strip(gpu, dtype)


@pytest.mark.parametrize('masked', (False, True), ids=('all', 'disc'))
def test_gpu_refine_jittered_sheet_three_rounds(gpu, masked):
    HC.check_refine_sheet(gpu, masked)


def test_gpu_refine_many_faces_on_one_edge(gpu):
    HC.check_refine_contended(gpu)


def test_gpu_refine_rejects_bad_indices_and_arguments(gpu):
    HC.check_refine_rejects(gpu)


def test_gpu_relax_equals_the_float64_yardstick_and_keeps_fixed_vertices(gpu):
    HC.check_relax(gpu)


def test_gpu_relax_obeys_the_maximum_principle(gpu):
    HC.check_relax_maximum_principle(gpu)


@pytest.mark.parametrize('name', ('cylinder', 'capsule'))
def test_gpu_watertight_closes_an_open_mesh(gpu, name):
    HC.check_watertight(gpu, name)


def test_gpu_script_functions_equal_their_numpy_restatements(gpu, tmp_path):
    HC.check_script_functions(gpu, tmp_path)


def test_gpu_process_body_msdf_distance_bodyedge_on_a_capsule(gpu, tmp_path):
    HC.check_whole_function(gpu, tmp_path)
