"""render.optixutils -- BVH occlusion, environment shading, denoiser, the shim -- on the host emulation of the kernel sources (CPU twins of
tests/test_gpu_optixutils.py; the check functions, the yardsticks and the parity rule live in tests/optixutils_cases.py)."""
import pytest

import optixutils_cases as OC


@pytest.mark.parametrize('name', OC.MESHES)
def test_emul_occlusion_matches_the_float64_test_over_all_triangles(emul, name):
    OC.check_occlusion(emul, name)


def test_emul_occlusion_honours_tmin_and_tmax(emul):
    OC.check_occlusion_range(emul)


def test_emul_occlusion_arguments_are_validated(emul):
    OC.check_occlusion_validation(emul)


@pytest.mark.parametrize('shadow_scale', (1.0, 0.5))
@pytest.mark.parametrize('n', (1, 3))
@pytest.mark.parametrize('BSDF', OC.BSDFS)
def test_emul_env_shade_outputs_and_gradients_match_the_yardstick(emul, BSDF, n, shadow_scale):
    OC.check_shade_parity(emul, BSDF, n, shadow_scale)


def test_emul_env_shade_strided_inputs_and_seeds(emul):
    OC.check_shade_layouts_and_seeds(emul)


def test_emul_env_shade_low_roughness_is_finite(emul):
    OC.check_shade_low_roughness(emul)


@pytest.mark.parametrize('case,BSDF', (('constant', 'diffuse'), ('occluded', 'pbr')))
def test_emul_env_shade_is_an_unbiased_estimator(emul, case, BSDF):
    OC.check_estimator(emul, case, BSDF)


@pytest.mark.parametrize('sigma', OC.DENOISE_SIGMAS)
@pytest.mark.parametrize('shape', OC.DENOISE_SHAPES)
def test_emul_denoiser_output_and_gradient_match_the_yardstick(emul, shape, sigma):
    OC.check_denoiser(emul, shape, sigma)


def test_emul_denoiser_arguments_are_validated(emul):
    OC.check_denoiser_validation(emul)


def test_emul_optix_build_bvh_is_free_and_the_build_is_lazy(emul, monkeypatch):
    OC.check_shim_is_lazy(emul, monkeypatch)


def test_emul_optix_env_shade_with_a_random_seed_backward(emul):
    OC.check_shim_random_seed_backward(emul)


def test_optixutils_exports_the_names_of_the_reference():
    OC.check_shim_exports()
