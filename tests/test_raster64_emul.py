"""Raster and antialias gradients against float64 at 4096 px, and the edges of the antialias kernels, on the host emulation of the kernel
sources (CPU twins of tests/test_gpu_raster64.py; the cases, the float64 reference and the bars live in tests/raster64_cases.py)."""
import pytest

import raster64_cases as RC


@pytest.mark.parametrize('name', list(RC.CASES))
def test_emul_raster64_rasterize_and_gbuffer_fold(emul, name):
    RC.run_raster(emul, name)


@pytest.mark.parametrize('name', list(RC.CASES))
def test_emul_raster64_antialias_separate_fused_and_mask_chain(emul, name):
    RC.run_aa(emul, name)


def test_raster64_kink_masking_on_synthetic_pairs():
    RC.check_kink_masking()


def test_antialias_edge_shapes_reach_the_scalar_copy_branch():
    RC.check_aa_shapes_reach_the_scalar_branch()


@pytest.mark.parametrize('shape', RC.AA_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_emul_antialias_scalar_copy_branch_and_odd_channel_totals(emul, shape):
    RC.check_aa_copy_branch(emul, shape)


def test_emul_antialias_silhouette_across_a_wave_boundary(emul):
    RC.check_aa_wave_boundary(emul)


def test_emul_antialias_nothing_blends_across_the_frame_boundary(emul):
    RC.check_aa_frame_boundary(emul)


def test_emul_antialias_three_routes_to_one_image_agree_bit_for_bit(emul):
    RC.check_aa_three_routes_agree_bit_for_bit(emul)


def test_emul_raster64_large_cases_within_three_times_the_float32_oracle(emul):
    RC.check_bar(emul, list(RC.LARGE), 'large')


def test_emul_raster64_control_cases_within_three_times_the_float32_oracle(emul):
    RC.check_bar(emul, list(RC.CONTROL), 'control')

