"""The 2-D material path -- tangents, the per-pixel material lookup, the texture-map branch of render_mesh, the OBJ round trip -- on the host
emulation of the kernel sources (CPU twins of tests/test_gpu_texmat.py; the check functions, the yardsticks and the parity rule live in
tests/texmat_cases.py)."""
import pytest

import texmat_cases as TC


def test_emul_tangents_match_the_upstream_run(emul):
    TC.check_tangents_golden(emul)


def test_emul_tangents_of_posed_frames(emul):
    TC.check_tangents_batched(emul)


def test_emul_tangents_gradient(emul):
    TC.check_tangents_gradient(emul)


def test_emul_mesh_helpers(emul, tmp_path):
    TC.check_mesh_helpers(emul, tmp_path)


@pytest.mark.parametrize('boundary', ('wrap', 'clamp'))
def test_emul_lookup_matches_the_restatement_and_the_composed_route(emul, boundary):
    TC.check_lookup(emul, boundary)


def test_emul_lookup_makes_gradient_buffers_only_where_asked(emul):
    TC.check_lookup_grad_buffers(emul)


def test_emul_lookup_of_nothing(emul):
    TC.check_lookup_empty(emul)


def test_emul_lookup_entry_points_validate_their_arguments(emul):
    TC.check_lookup_entry_points_validate(emul)


def test_emul_export_renders_as_what_was_baked(emul):
    TC.check_export_renders_as_baked(emul)


def test_emul_branch_buffers_and_normals(emul):
    TC.check_branch_buffers(emul)


def test_emul_perturbed_normal_smoothness(emul):
    TC.check_perturbed_nrm_grad(emul)


@pytest.mark.parametrize('fused', (True, False), ids=('fused', 'composed'))
def test_emul_map_gradients(emul, fused):
    TC.check_branch_gradients(emul, fused)


def test_emul_position_gradient_takes_the_composed_route(emul):
    TC.check_position_gradient(emul)


def test_emul_branch_options_and_errors(emul):
    TC.check_branch_options(emul)


def test_emul_obj_round_trip(emul, tmp_path):
    TC.check_round_trip(emul, tmp_path)


def test_emul_mlp_branch_is_unchanged(emul):
    TC.check_mlp_branch_unchanged(emul)
