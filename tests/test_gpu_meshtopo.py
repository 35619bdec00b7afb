"""Stage hand-off topology -- connected components, vertex weld, open edges, script/connet_face_head.py -- on the MI355X (GPU twins of
tests/test_meshtopo_emul.py; the check functions, the yardsticks and the mesh generators live in tests/meshtopo_cases.py).  The emulator runs
the threads of a launch one after another: the strip, fan and one-point cases test the lock-free updates only here."""
import pytest
import torch

import meshtopo_cases as MC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', MC.CC_CASES)
def test_gpu_components_equal_the_union_find_yardstick(gpu, name):
    MC.check_components(gpu, name)


def test_gpu_components_ranked_and_faces_grouped_as_the_reference_does(gpu):
    MC.check_rank_and_faces(gpu)


def test_gpu_a_face_index_out_of_range_is_reported(gpu):
    MC.check_components_reject_bad_index(gpu)


@pytest.mark.parametrize('dtype', (torch.float64, torch.float32), ids=('f64', 'f32'))
@pytest.mark.parametrize('name', MC.WELD_CASES)
def test_gpu_weld_equals_the_dict_yardstick(gpu, name, dtype):
    MC.check_weld(gpu, name, dtype)


@pytest.mark.parametrize('dtype', (torch.float64, torch.float32), ids=('f64', 'f32'))
def test_gpu_weld_in_the_smallest_legal_table(gpu, dtype):
    MC.check_weld_forced_table(gpu, dtype)


def test_gpu_weld_refuses_a_table_that_is_too_small(gpu):
    MC.check_weld_table_too_small(gpu)


def test_gpu_merge_and_repair(gpu):
    MC.check_merge_and_repair(gpu)


def test_gpu_open_vertices(gpu):
    MC.check_open_edges(gpu)


def test_gpu_peel_open_faces(gpu):
    MC.check_peel(gpu)


def test_gpu_open_vertices_reproduce_the_golden(gpu):
    MC.check_open_edges_golden(gpu)


@pytest.mark.parametrize('name', ('a', 'b', 'c'))
def test_gpu_process_close_hole_reproduces_the_golden(gpu, name, tmp_path):
    MC.check_close_hole(gpu, name, tmp_path)


def test_gpu_obj_reader_and_writer(gpu, tmp_path):
    MC.check_obj_reader(gpu, tmp_path)


def test_gpu_entry_points_validate_their_arguments(gpu):
    MC.check_entry_points_validate(gpu)
