"""The BSDF and cube-map entry points of render.renderutils on the host emulation of the kernel sources (CPU twins of
tests/test_gpu_renderutils.py; the check functions, the parity rule and the brute-force cube-map yardstick live in tests/renderutils_cases.py)."""
import pytest

import renderutils_cases as RC


@pytest.mark.parametrize('case', list(RC.CASES))
def test_emul_bsdf_output_and_gradients_match_the_reference_twin(emul, case):
    RC.check_parity(emul, case)


@pytest.mark.parametrize('case', list(RC.CASES))
def test_emul_bsdf_use_python_matches_the_twin_and_the_kernels(emul, case):
    RC.check_python_twin(emul, case)


def test_emul_bsdf_masked_pixels_and_clamped_parameters_get_exact_zeros(emul):
    RC.check_exact_zeros(emul)


def test_emul_pbr_specular_degenerate_rows_are_finite(emul):
    RC.check_degenerate_rows_are_finite(emul)


def test_emul_bsdf_broadcast_and_non_contiguous_inputs(emul):
    RC.check_layouts(emul)


def test_emul_pbr_bsdf_skips_the_gradients_nobody_needs(emul):
    RC.check_skipped_gradients(emul)


@pytest.mark.parametrize('roughness', RC.CUBE_ROUGHNESS)
@pytest.mark.parametrize('N', RC.CUBE_NS)
def test_emul_cubemap_filters_match_the_sum_over_all_texel_pairs(emul, N, roughness):
    RC.check_cubemap(emul, N, roughness)


@pytest.mark.parametrize('N,roughness', RC.CUBE_PATCHED)
def test_emul_cubemap_filters_with_several_patches_per_face(emul, N, roughness):
    RC.check_cubemap(emul, N, roughness)


def test_emul_cubemap_identity_and_row_sum_properties(emul):
    RC.check_cubemap_properties(emul)


def test_emul_cubemap_backward_is_reproducible(emul):
    RC.check_cubemap_backward_is_reproducible(emul)


def test_emul_cubemap_shapes_are_validated(emul):
    RC.check_cubemap_validation(emul)


def test_cubemap_patch_cones_hold_every_texel_of_their_patch():
    RC.check_patch_cones()
