"""The image-space loss kernels against float64, per element and at their edges, on the host emulation of csrc/image_ops.hip (CPU twins of
tests/test_gpu_loss64.py; the cases, the float64 references and the rules live in tests/loss64_cases.py)."""
import pytest

import loss64_cases as LC

_id = lambda c: c['tag'][c['tag'].index(' ') + 1:].replace(' ', '-')
SSIM_SHAPES = [(H, W, N, nb) for (H, W) in LC.GEOMETRY for N in (1, 3) for nb in (0, 1)]


@pytest.mark.parametrize('H,W,N,need_b', SSIM_SHAPES, ids=[f'{H}x{W}-N{N}-' + ('d_a-d_b' if nb else 'd_a') for H, W, N, nb in SSIM_SHAPES])
def test_emul_loss64_ssim_value_and_gradients_vs_float64(emul, H, W, N, need_b):
    for c in LC.SSIM_CASES:
        if (c['H'], c['W'], c['N']) == (H, W, N):
            LC.run_ssim(emul, c, need_b)


@pytest.mark.parametrize('case', LC.OCC_CASES, ids=[_id(c) for c in LC.OCC_CASES])
def test_emul_loss64_ssim_occupancy_cells_with_poisoned_buffers(emul, case):
    LC.run_occ(emul, case)


@pytest.mark.parametrize('case', LC.PIXEL_CASES, ids=[_id(c) for c in LC.PIXEL_CASES])
def test_emul_loss64_pixel_losses_vs_float64(emul, case):
    LC.run_pixel(emul, case)


@pytest.mark.parametrize('case', LC.SEQ_CASES, ids=[_id(c) for c in LC.SEQ_CASES])
def test_emul_loss64_seq_losses_vs_float64(emul, case):
    LC.run_seq(emul, case)


@pytest.mark.parametrize('case', LC.IMAGE_CASES, ids=[_id(c) for c in LC.IMAGE_CASES])
def test_emul_loss64_image_loss_vs_float64(emul, case):
    LC.run_image(emul, case)


@pytest.mark.parametrize('group', LC.GROUPS)
def test_emul_loss64_decade_bands_within_three_times_the_float32_reference(emul, group):
    LC.check_group(emul, group)


def test_emul_loss64_logf_powf_within_the_figures_rule_b_uses(emul):
    LC.check_log_pow(emul)


def test_loss64_restated_image_loss_backward_vs_float64_autograd():
    LC.check_restated_backward()


def test_loss64_inputs_have_the_edges_they_claim():
    LC.check_inputs()


def test_loss64_band_exceptions_cover_only_the_bands_they_name():
    for (group, tensor), (tops, bar, _) in LC.BAND_RATIO.items():
        assert bar > LC.RATIO
        for top in tops:
            assert LC.band_bar(group, tensor, top) == bar
        for top in (-30, -7, 0, 5):
            if top not in tops:
                assert LC.band_bar(group, tensor, top) == LC.RATIO
        assert LC.band_bar('image', tensor, tops[0]) == LC.RATIO
    assert LC.band_bar('seq', 'd_st', LC.ZERO_BAND) == LC.RATIO and LC.band_bar('image', 'd_img', -3) == LC.RATIO


def test_loss64_rule_b_chains_follow_the_grids_of_the_wrappers():
    """the grid sizes rule (b) counts with: 2048 / 1024 / 2048 workgroups at most, and the sizes that give a workgroup a second trip"""
    assert LC.chain_pixel(524288) == 1 + 9 + 8 + 9 + 1 and LC.chain_pixel(524289) == 2 + 9 + 8 + 9 + 1
    assert LC.chain_seq(262144) == 1 + 9 + 1024 + 1 and LC.chain_seq(262145) == 2 + 9 + 1024 + 1
    assert LC.chain_image(257) == 1 + 9 + 2 + 1 and LC.chain_ssim(3, 129, 70) == 32 + 9 + 2 * 2 * 3 + 1
    assert 524289 in LC.SHAPES and 262145 in LC.SEQ_SHAPES
