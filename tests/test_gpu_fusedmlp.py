"""The general fused MLP on the MI355X (the check functions and the float64 restatement live in tests/fusedmlp_cases.py)."""
import pytest

import fusedmlp_cases as FC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('shape', FC.SHAPES + [FC.SHAPE_GPU_ONLY], ids=lambda s: '-'.join(str(v) for v in s))
def test_gpu_fusedmlp_shape_matrix(gpu, shape):
    FC.check_shape(gpu, shape)


def test_gpu_fusedmlp_row_counts_and_one_workgroup_walking_every_tile(gpu):
    FC.check_row_counts(gpu, n_walk=200003)


def test_gpu_fusedmlp_hidden_activations(gpu):
    FC.check_hidden_activations(gpu)


def test_gpu_fusedmlp_output_activations_with_mask_affine_map_and_gradient_scale(gpu):
    FC.check_output_activations(gpu)


def test_gpu_fusedmlp_weight_gradients_accumulate_and_the_input_gradient_is_overwritten(gpu):
    FC.check_accumulation(gpu)


def test_gpu_fusedmlp_configurations_are_validated_before_any_launch(gpu, monkeypatch):
    FC.check_validation(gpu, monkeypatch)


def test_gpu_tcnn_network_and_network_with_input_encoding(gpu):
    FC.check_shim(gpu)


def test_gpu_mlptexture_routes_general_networks_through_the_fused_mlp(gpu, monkeypatch):
    FC.check_texture(gpu, monkeypatch, 40000)
