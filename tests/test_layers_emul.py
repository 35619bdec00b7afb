"""Layered rendering -- the blend step of peeled layers, render_mesh(num_layers > 1) with the opacity in kd's fourth channel, the transparent export and
its OBJ round trip -- on the host emulation of the kernel sources (the check functions, the yardsticks and the parity rule live in
tests/layers_cases.py; tests/test_gpu_layers.py runs the same checks on the MI355X)."""
import pytest

import layers_cases as LC


@pytest.mark.parametrize('layer', (0, 1, 2))
def test_step_matches_the_restatement(emul, layer):
    LC.check_kernel(emul, layer)


def test_step_without_alpha(emul):
    LC.check_kernel(emul, 1, use_alpha=False)


def test_step_writes_only_the_gradients_asked_for(emul):
    LC.check_null_gradient_outputs(emul)


def test_step_over_nothing_is_the_identity(emul):
    LC.check_nothing_covered(emul)


def test_step_wrapper_refuses_too_many_channels(emul):
    LC.check_channel_limit(emul)


def test_step_entry_points_validate_their_arguments(emul):
    LC.check_entry_points_validate(emul)


@pytest.mark.parametrize('with_msdf', (False, True), ids=('buffers', 'buffers+msdf'))
def test_layered_render_matches_the_restatement_on_both_routes(emul, with_msdf):
    LC.check_render_buffers(emul, with_msdf)


@pytest.mark.parametrize('fused', (True, False), ids=('fused', 'composed'))
def test_layered_map_gradients(emul, fused):
    LC.check_map_gradients(emul, fused)


@pytest.mark.parametrize('fused', (True, False), ids=('fused', 'composed'))
def test_layered_position_gradient(emul, fused):
    LC.check_position_gradient(emul, fused)


def test_layered_render_is_exact_where_it_must_be(emul):
    LC.check_exactness(emul)


def test_layered_options_and_errors(emul):
    LC.check_options_and_errors(emul)


def test_transparent_export_options(emul):
    LC.check_export_options(emul)


def test_transparent_obj_round_trip(emul, tmp_path):
    LC.check_round_trip(emul, tmp_path)
