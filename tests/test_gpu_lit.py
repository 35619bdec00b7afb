"""The lit render path -- light tables, light and denoiser modules, the two-image denoise kernel, shade_lit, FLAGS.lit_shading in render_mesh, a
lit tick_init -- on the MI355X (GPU twins of tests/test_lit_emul.py; the check functions live in
tests/lit_cases.py)."""
import pytest

import lit_cases as LC
import optixutils_cases as OC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', LC.LIGHT_MAPS + LC.TALL_MAPS)
def test_gpu_light_tables_match_float64_and_are_exactly_monotone(gpu, name):
    LC.check_light_tables(gpu, name)


def test_gpu_light_tables_arguments_are_validated(gpu):
    LC.check_light_validation(gpu)


def test_gpu_light_module_has_the_reference_surface(gpu):
    LC.check_light_module(gpu)


def test_gpu_load_env_and_save_env_map(gpu, tmp_path):
    LC.check_light_files(gpu, tmp_path)


@pytest.mark.parametrize('sigma', OC.DENOISE_SIGMAS)
@pytest.mark.parametrize('shape', OC.DENOISE_SHAPES)
def test_gpu_denoiser_pair_equals_two_single_calls(gpu, shape, sigma):
    LC.check_denoiser_pair(gpu, shape, sigma)


@pytest.mark.parametrize('shape', OC.DENOISE_SHAPES)
def test_gpu_denoiser_module_forward_and_forward_many(gpu, shape):
    LC.check_denoiser_module(gpu, shape)


def test_gpu_denoiser_pair_arguments_are_validated(gpu):
    LC.check_denoiser_pair_validation(gpu)


@pytest.mark.parametrize('demodulate', (True, False))
@pytest.mark.parametrize('bsdf', OC.BSDFS)
def test_gpu_shade_lit_equals_the_op_by_op_composition(gpu, bsdf, demodulate):
    LC.check_shade_lit(gpu, bsdf, demodulate)


def test_gpu_shade_lit_seed_counter_and_denoiser_paths(gpu, monkeypatch):
    LC.check_shade_lit_seed_and_denoiser_paths(gpu, monkeypatch)


def test_gpu_render_mesh_without_the_flag_is_untouched(gpu):
    LC.check_render_mesh_unlit_is_untouched(gpu)


def test_gpu_render_mesh_lit_branch(gpu, monkeypatch):
    LC.check_render_mesh_lit(gpu, monkeypatch)


def test_gpu_render_mesh_other_bsdfs_under_the_flag(gpu, monkeypatch):
    LC.check_render_mesh_unlit_bsdfs(gpu, monkeypatch)


def test_gpu_tick_init_lit(gpu):
    LC.check_tick_init_lit(gpu)
