"""The general grid encoding on the MI355X, at working sizes (the check functions and the float64 restatement live in tests/gridenc_cases.py)."""
import pytest

import gridenc_cases as GC

pytestmark = pytest.mark.gpu


def test_gpu_gridenc_reference_configuration_equals_the_oracle_and_the_fused_kernels(gpu):
    GC.check_anchor(gpu, n=5000)


def test_gpu_gridenc_hashed_levels(gpu):
    GC.check_hashed_collisions(gpu)
    for T in (19, 21):
        GC.check_hashed(gpu, T, 1 << 20)


def test_gpu_gridenc_matrix_of_dims_features_interpolation_and_type(gpu):
    GC.check_matrix(gpu, n=20000)


def test_gpu_gridenc_accumulation_of_coherent_and_identical_points(gpu):
    GC.check_accumulation(gpu, T=19, m=1 << 16, n_same=100000)


def test_gpu_gridenc_edges(gpu):
    GC.check_edges(gpu, T=19, n_big=100003)


def test_gpu_gridenc_finite_rows_outside_the_unit_cube_stay_inside_the_table(gpu):
    GC.check_out_of_range(gpu, nonfinite=False, n=60000, T=19)


def test_gpu_gridenc_configurations_are_validated_before_any_launch(gpu):
    GC.check_validation(gpu)


def test_gpu_tcnn_encoding_shim_and_texture_routing(gpu, monkeypatch):
    GC.check_shim(gpu, monkeypatch)


def test_gpu_mlptexture_with_a_16_level_grid(gpu):
    GC.check_texture(gpu, 40000, enc_cfg=GC.cfg16(19))


def test_gpu_mlptexture_with_another_network_shape(gpu):
    GC.check_texture(gpu, 40000, channels=9, internal_dims=64, hidden=3)


def test_gpu_tick_init_step_with_a_16_level_texture_grid(gpu, monkeypatch):
    GC.check_step(gpu, monkeypatch)
