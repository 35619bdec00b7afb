"""The image-space loss kernels against float64, per element and at their edges, on the MI355X (the cases, the float64 references and the rules
live in tests/loss64_cases.py)."""
import pytest

import loss64_cases as LC

pytestmark = pytest.mark.gpu

_id = lambda c: c['tag'][c['tag'].index(' ') + 1:].replace(' ', '-')
SSIM_SHAPES = [(H, W, N, nb) for (H, W) in LC.GEOMETRY for N in (1, 3) for nb in (0, 1)]
OCC = LC.OCC_CASES + LC.OCC_CASES_GPU_ONLY


@pytest.mark.parametrize('H,W,N,need_b', SSIM_SHAPES, ids=[f'{H}x{W}-N{N}-' + ('d_a-d_b' if nb else 'd_a') for H, W, N, nb in SSIM_SHAPES])
def test_gpu_loss64_ssim_value_and_gradients_vs_float64(gpu, H, W, N, need_b):
    for c in LC.SSIM_CASES:
        if (c['H'], c['W'], c['N']) == (H, W, N):
            LC.run_ssim(gpu, c, need_b)


@pytest.mark.parametrize('case', OCC, ids=[_id(c) for c in OCC])
def test_gpu_loss64_ssim_occupancy_cells_with_poisoned_buffers(gpu, case):
    LC.run_occ(gpu, case)


@pytest.mark.parametrize('case', LC.PIXEL_CASES, ids=[_id(c) for c in LC.PIXEL_CASES])
def test_gpu_loss64_pixel_losses_vs_float64(gpu, case):
    LC.run_pixel(gpu, case)


@pytest.mark.parametrize('case', LC.SEQ_CASES, ids=[_id(c) for c in LC.SEQ_CASES])
def test_gpu_loss64_seq_losses_vs_float64(gpu, case):
    LC.run_seq(gpu, case)


@pytest.mark.parametrize('case', LC.IMAGE_CASES, ids=[_id(c) for c in LC.IMAGE_CASES])
def test_gpu_loss64_image_loss_vs_float64(gpu, case):
    LC.run_image(gpu, case)


@pytest.mark.parametrize('group', LC.GROUPS)
def test_gpu_loss64_decade_bands_within_three_times_the_float32_reference(gpu, group):
    LC.check_group(gpu, group)


def test_gpu_loss64_logf_powf_within_the_figures_rule_b_uses(gpu):
    LC.check_log_pow(gpu)
