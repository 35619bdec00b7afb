"""The BSDF and cube-map entry points of render.renderutils on the MI355X (GPU twins of
tests/test_renderutils_emul.py, same shapes; the check functions, the parity rule and the brute-force cube-map yardstick live in tests/renderutils_cases.py)."""
import pytest

import renderutils_cases as RC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', list(RC.CASES))
def test_gpu_bsdf_output_and_gradients_match_the_reference_twin(gpu, case):
    RC.check_parity(gpu, case)


@pytest.mark.parametrize('case', list(RC.CASES))
def test_gpu_bsdf_use_python_matches_the_twin_and_the_kernels(gpu, case):
    RC.check_python_twin(gpu, case)


def test_gpu_bsdf_masked_pixels_and_clamped_parameters_get_exact_zeros(gpu):
    RC.check_exact_zeros(gpu)


def test_gpu_pbr_specular_degenerate_rows_are_finite(gpu):
    RC.check_degenerate_rows_are_finite(gpu)


def test_gpu_bsdf_broadcast_and_non_contiguous_inputs(gpu):
    RC.check_layouts(gpu)


def test_gpu_pbr_bsdf_skips_the_gradients_nobody_needs(gpu):
    RC.check_skipped_gradients(gpu)


@pytest.mark.parametrize('roughness', RC.CUBE_ROUGHNESS)
@pytest.mark.parametrize('N', RC.CUBE_NS)
def test_gpu_cubemap_filters_match_the_sum_over_all_texel_pairs(gpu, N, roughness):
    RC.check_cubemap(gpu, N, roughness)


@pytest.mark.parametrize('N,roughness', RC.CUBE_PATCHED)
def test_gpu_cubemap_filters_with_several_patches_per_face(gpu, N, roughness):
    RC.check_cubemap(gpu, N, roughness)


def test_gpu_cubemap_identity_and_row_sum_properties(gpu):
    RC.check_cubemap_properties(gpu)


def test_gpu_cubemap_backward_is_reproducible(gpu):
    RC.check_cubemap_backward_is_reproducible(gpu)


def test_gpu_cubemap_shapes_are_validated(gpu):
    RC.check_cubemap_validation(gpu)
