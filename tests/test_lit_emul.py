"""The lit render path -- light tables, light and denoiser modules, the two-image denoise kernel, shade_lit, FLAGS.lit_shading in render_mesh, a
lit tick_init -- on the host emulation of the kernel sources (CPU twins of tests/test_gpu_lit.py; the check functions live in
tests/lit_cases.py)."""
import pytest

import lit_cases as LC
import optixutils_cases as OC


@pytest.mark.parametrize('name', LC.LIGHT_MAPS + LC.TALL_MAPS)
def test_emul_light_tables_match_float64_and_are_exactly_monotone(emul, name):
    LC.check_light_tables(emul, name)


def test_emul_light_tables_arguments_are_validated(emul):
    LC.check_light_validation(emul)


def test_emul_light_module_has_the_reference_surface(emul):
    LC.check_light_module(emul)


def test_emul_load_env_and_save_env_map(emul, tmp_path):
    LC.check_light_files(emul, tmp_path)


@pytest.mark.parametrize('sigma', OC.DENOISE_SIGMAS)
@pytest.mark.parametrize('shape', OC.DENOISE_SHAPES)
def test_emul_denoiser_pair_equals_two_single_calls(emul, shape, sigma):
    LC.check_denoiser_pair(emul, shape, sigma)


@pytest.mark.parametrize('shape', OC.DENOISE_SHAPES)
def test_emul_denoiser_module_forward_and_forward_many(emul, shape):
    LC.check_denoiser_module(emul, shape)


def test_emul_denoiser_pair_arguments_are_validated(emul):
    LC.check_denoiser_pair_validation(emul)


@pytest.mark.parametrize('demodulate', (True, False))
@pytest.mark.parametrize('bsdf', OC.BSDFS)
def test_emul_shade_lit_equals_the_op_by_op_composition(emul, bsdf, demodulate):
    LC.check_shade_lit(emul, bsdf, demodulate)


def test_emul_shade_lit_seed_counter_and_denoiser_paths(emul, monkeypatch):
    LC.check_shade_lit_seed_and_denoiser_paths(emul, monkeypatch)


def test_emul_render_mesh_without_the_flag_is_untouched(emul):
    LC.check_render_mesh_unlit_is_untouched(emul)


def test_emul_render_mesh_lit_branch(emul, monkeypatch):
    LC.check_render_mesh_lit(emul, monkeypatch)


def test_emul_render_mesh_other_bsdfs_under_the_flag(emul, monkeypatch):
    LC.check_render_mesh_unlit_bsdfs(emul, monkeypatch)


def test_emul_tick_init_lit(emul):
    LC.check_tick_init_lit(emul)
