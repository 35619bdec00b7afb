"""Layered rendering -- the blend step of peeled layers, render_mesh(num_layers > 1) with the opacity in kd's fourth channel, the transparent export and
its OBJ round trip -- on the MI355X (GPU twins of tests/test_layers_emul.py; the check functions, the yardsticks and the parity rule live in
tests/layers_cases.py)."""
import pytest

import layers_cases as LC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('layer', (0, 1, 2))
def test_gpu_step_matches_the_restatement(gpu, layer):
    LC.check_kernel(gpu, layer)


def test_gpu_step_without_alpha(gpu):
    LC.check_kernel(gpu, 1, use_alpha=False)


def test_gpu_step_writes_only_the_gradients_asked_for(gpu):
    LC.check_null_gradient_outputs(gpu)


def test_gpu_step_over_nothing_is_the_identity(gpu):
    LC.check_nothing_covered(gpu)


def test_gpu_step_wrapper_refuses_too_many_channels(gpu):
    LC.check_channel_limit(gpu)


def test_gpu_step_entry_points_validate_their_arguments(gpu):
    LC.check_entry_points_validate(gpu)


@pytest.mark.parametrize('with_msdf', (False, True), ids=('buffers', 'buffers+msdf'))
def test_gpu_layered_render_matches_the_restatement_on_both_routes(gpu, with_msdf):
    LC.check_render_buffers(gpu, with_msdf)


@pytest.mark.parametrize('fused', (True, False), ids=('fused', 'composed'))
def test_gpu_layered_map_gradients(gpu, fused):
    LC.check_map_gradients(gpu, fused)


@pytest.mark.parametrize('fused', (True, False), ids=('fused', 'composed'))
def test_gpu_layered_position_gradient(gpu, fused):
    LC.check_position_gradient(gpu, fused)


def test_gpu_layered_render_is_exact_where_it_must_be(gpu):
    LC.check_exactness(gpu)


def test_gpu_layered_options_and_errors(gpu):
    LC.check_options_and_errors(gpu)


def test_gpu_transparent_export_options(gpu):
    LC.check_export_options(gpu)


def test_gpu_transparent_obj_round_trip(gpu, tmp_path):
    LC.check_round_trip(gpu, tmp_path)
