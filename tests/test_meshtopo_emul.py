"""Stage hand-off topology -- connected components, vertex weld, open edges, script/connet_face_head.py -- on the host emulation of the kernel
sources (CPU twins of tests/test_gpu_meshtopo.py; the check functions, the yardsticks and the mesh generators live in tests/meshtopo_cases.py)."""
import pytest
import torch

import meshtopo_cases as MC


@pytest.mark.parametrize('name', MC.CC_CASES)
def test_emul_components_equal_the_union_find_yardstick(emul, name):
    MC.check_components(emul, name)


def test_emul_components_ranked_and_faces_grouped_as_the_reference_does(emul):
    MC.check_rank_and_faces(emul)


def test_emul_a_face_index_out_of_range_is_reported(emul):
    MC.check_components_reject_bad_index(emul)


@pytest.mark.parametrize('dtype', (torch.float64, torch.float32), ids=('f64', 'f32'))
@pytest.mark.parametrize('name', MC.WELD_CASES)
def test_emul_weld_equals_the_dict_yardstick(emul, name, dtype):
    MC.check_weld(emul, name, dtype)


@pytest.mark.parametrize('dtype', (torch.float64, torch.float32), ids=('f64', 'f32'))
def test_emul_weld_in_the_smallest_legal_table(emul, dtype):
    MC.check_weld_forced_table(emul, dtype)


def test_emul_weld_refuses_a_table_that_is_too_small(emul):
    MC.check_weld_table_too_small(emul)


def test_emul_merge_and_repair(emul):
    MC.check_merge_and_repair(emul)


def test_emul_open_vertices(emul):
    MC.check_open_edges(emul)


def test_emul_peel_open_faces(emul):
    MC.check_peel(emul)


def test_emul_open_vertices_reproduce_the_golden(emul):
    MC.check_open_edges_golden(emul)


@pytest.mark.parametrize('name', ('a', 'b', 'c'))
def test_emul_process_close_hole_reproduces_the_golden(emul, name, tmp_path):
    MC.check_close_hole(emul, name, tmp_path)


def test_emul_obj_reader_and_writer(emul, tmp_path):
    MC.check_obj_reader(emul, tmp_path)


def test_emul_entry_points_validate_their_arguments(emul):
    MC.check_entry_points_validate(emul)


def test_script_is_a_namespace_package_merged_with_other_roots(tmp_path):
    MC.check_script_namespace(tmp_path)
