"""render.optixutils -- BVH occlusion, environment shading, denoiser, the shim -- on the MI355X (GPU twins of
tests/test_optixutils_emul.py; the check functions, the yardsticks and the parity rule live in tests/optixutils_cases.py)."""
import pytest

import optixutils_cases as OC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', OC.MESHES)
def test_gpu_occlusion_matches_the_float64_test_over_all_triangles(gpu, name):
    OC.check_occlusion(gpu, name)


def test_gpu_occlusion_honours_tmin_and_tmax(gpu):
    OC.check_occlusion_range(gpu)


def test_gpu_occlusion_arguments_are_validated(gpu):
    OC.check_occlusion_validation(gpu)


@pytest.mark.parametrize('shadow_scale', (1.0, 0.5))
@pytest.mark.parametrize('n', (1, 3))
@pytest.mark.parametrize('BSDF', OC.BSDFS)
def test_gpu_env_shade_outputs_and_gradients_match_the_yardstick(gpu, BSDF, n, shadow_scale):
    OC.check_shade_parity(gpu, BSDF, n, shadow_scale)


def test_gpu_env_shade_strided_inputs_and_seeds(gpu):
    OC.check_shade_layouts_and_seeds(gpu)


def test_gpu_env_shade_low_roughness_is_finite(gpu):
    OC.check_shade_low_roughness(gpu)


@pytest.mark.parametrize('case,BSDF', (('constant', 'diffuse'), ('occluded', 'pbr')))
def test_gpu_env_shade_is_an_unbiased_estimator(gpu, case, BSDF):
    OC.check_estimator(gpu, case, BSDF)


@pytest.mark.parametrize('sigma', OC.DENOISE_SIGMAS)
@pytest.mark.parametrize('shape', OC.DENOISE_SHAPES)
def test_gpu_denoiser_output_and_gradient_match_the_yardstick(gpu, shape, sigma):
    OC.check_denoiser(gpu, shape, sigma)


def test_gpu_denoiser_arguments_are_validated(gpu):
    OC.check_denoiser_validation(gpu)


def test_gpu_optix_build_bvh_is_free_and_the_build_is_lazy(gpu, monkeypatch):
    OC.check_shim_is_lazy(gpu, monkeypatch)


def test_gpu_optix_env_shade_with_a_random_seed_backward(gpu):
    OC.check_shim_random_seed_backward(gpu)
