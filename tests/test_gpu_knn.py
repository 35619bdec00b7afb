"""K-nearest search and K-blended skinning on the MI355X, at working sizes (the check functions live in tests/knn_cases.py)."""
import pytest

import knn_cases as KC

pytestmark = pytest.mark.gpu


def test_gpu_knnk_equals_the_restatement_and_the_grid_the_exhaustive_search(gpu):
    KC.check_knnk_search(gpu)
    KC.check_knnk_search(gpu, nv=10475, nq=50000, seed=1, Ks=(4, 8), degenerate=False)


def test_gpu_knnk_counted_rows(gpu):
    KC.check_knnk_counted(gpu)
    KC.check_knnk_counted(gpu, nv=10475, nq=20000, K=8)


def test_gpu_knn_arguments_are_validated_before_any_launch(gpu):
    KC.check_knn_argument_errors(gpu)


def test_gpu_lbsk_reference_golden(gpu):
    KC.check_lbsk_golden(gpu)


def test_gpu_lbsk_gradient_through_the_blend_weights(gpu):
    for K in (2, 4, 8):
        for nb in (1, 4):
            KC.check_lbsk_grad(gpu, K, nb, P=20000)


def test_gpu_knn_points_shim_contract(gpu):
    KC.check_shim(gpu)


def test_gpu_deformer_k(gpu):
    KC.check_deformer_k(gpu)


def test_gpu_launch_ahead_of_the_sizes_equals_the_plain_order_with_k4(gpu, monkeypatch):
    KC.check_launch_ahead_k(gpu, monkeypatch, res=256, grid_n=24, frames=2, ticks=5, prefit=300, body_verts=2048, samples=20000, loss_set='full')


def test_gpu_tick_init_step_with_k4(gpu):
    KC.check_tick_init_k(gpu)
