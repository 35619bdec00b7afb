"""The general fused MLP on the host emulation of the kernel sources (CPU twins of tests/test_gpu_fusedmlp.py; the check functions and the
float64 restatement live in tests/fusedmlp_cases.py)."""
import pytest

import fusedmlp_cases as FC


@pytest.mark.parametrize('shape', FC.SHAPES, ids=lambda s: '-'.join(str(v) for v in s))
def test_emul_fusedmlp_shape_matrix(emul, shape):
    FC.check_shape(emul, shape)


def test_emul_fusedmlp_row_counts_and_one_workgroup_walking_every_tile(emul):
    FC.check_row_counts(emul, n_walk=1000)


def test_emul_fusedmlp_hidden_activations(emul):
    FC.check_hidden_activations(emul)


def test_emul_fusedmlp_output_activations_with_mask_affine_map_and_gradient_scale(emul):
    FC.check_output_activations(emul)


def test_emul_fusedmlp_weight_gradients_accumulate_and_the_input_gradient_is_overwritten(emul):
    FC.check_accumulation(emul)


def test_emul_fusedmlp_configurations_are_validated_before_any_launch(emul, monkeypatch):
    FC.check_validation(emul, monkeypatch)


def test_emul_tcnn_network_and_network_with_input_encoding(emul):
    FC.check_shim(emul)


def test_emul_mlptexture_routes_general_networks_through_the_fused_mlp(emul, monkeypatch):
    FC.check_texture(emul, monkeypatch, 400)
