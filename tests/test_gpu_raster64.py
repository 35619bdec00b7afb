"""Raster and antialias gradients against float64 at 4096 px, and the edges of the antialias kernels, on the MI355X (the cases, the float64
reference and the bars live in tests/raster64_cases.py)."""
import pytest

import raster64_cases as RC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', list(RC.CASES))
def test_gpu_raster64_rasterize_and_gbuffer_fold(gpu, name):
    RC.run_raster(gpu, name)


@pytest.mark.parametrize('name', list(RC.CASES))
def test_gpu_raster64_antialias_separate_fused_and_mask_chain(gpu, name):
    RC.run_aa(gpu, name)


@pytest.mark.parametrize('shape', RC.AA_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_gpu_antialias_scalar_copy_branch_and_odd_channel_totals(gpu, shape):
    RC.check_aa_copy_branch(gpu, shape)


def test_gpu_antialias_silhouette_across_a_wave_boundary(gpu):
    RC.check_aa_wave_boundary(gpu)


def test_gpu_antialias_nothing_blends_across_the_frame_boundary(gpu):
    RC.check_aa_frame_boundary(gpu)


def test_gpu_raster64_large_cases_within_three_times_the_float32_oracle(gpu):
    RC.check_bar(gpu, list(RC.LARGE), 'large')


def test_gpu_raster64_control_cases_within_three_times_the_float32_oracle(gpu):
    RC.check_bar(gpu, list(RC.CONTROL), 'control')

