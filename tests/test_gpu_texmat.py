"""The 2-D material path -- tangents, the per-pixel material lookup, the texture-map branch of render_mesh, the OBJ round trip -- on the MI355X
(GPU twins of tests/test_texmat_emul.py; the check functions, the yardsticks and the parity rule live in tests/texmat_cases.py)."""
import pytest

import texmat_cases as TC

pytestmark = pytest.mark.gpu


def test_gpu_tangents_match_the_upstream_run(gpu):
    TC.check_tangents_golden(gpu)


def test_gpu_tangents_of_posed_frames(gpu):
    TC.check_tangents_batched(gpu)


def test_gpu_tangents_gradient(gpu):
    TC.check_tangents_gradient(gpu)


def test_gpu_mesh_helpers(gpu, tmp_path):
    TC.check_mesh_helpers(gpu, tmp_path)


@pytest.mark.parametrize('boundary', ('wrap', 'clamp'))
def test_gpu_lookup_matches_the_restatement_and_the_composed_route(gpu, boundary):
    TC.check_lookup(gpu, boundary)


def test_gpu_lookup_makes_gradient_buffers_only_where_asked(gpu):
    TC.check_lookup_grad_buffers(gpu)


def test_gpu_lookup_of_nothing(gpu):
    TC.check_lookup_empty(gpu)


def test_gpu_lookup_entry_points_validate_their_arguments(gpu):
    TC.check_lookup_entry_points_validate(gpu)


def test_gpu_export_renders_as_what_was_baked(gpu):
    TC.check_export_renders_as_baked(gpu)


def test_gpu_branch_buffers_and_normals(gpu):
    TC.check_branch_buffers(gpu)


def test_gpu_perturbed_normal_smoothness(gpu):
    TC.check_perturbed_nrm_grad(gpu)


@pytest.mark.parametrize('fused', (True, False), ids=('fused', 'composed'))
def test_gpu_map_gradients(gpu, fused):
    TC.check_branch_gradients(gpu, fused)


def test_gpu_position_gradient_takes_the_composed_route(gpu):
    TC.check_position_gradient(gpu)


def test_gpu_branch_options_and_errors(gpu):
    TC.check_branch_options(gpu)


def test_gpu_obj_round_trip(gpu, tmp_path):
    TC.check_round_trip(gpu, tmp_path)


def test_gpu_mlp_branch_is_unchanged(gpu):
    TC.check_mlp_branch_unchanged(gpu)
