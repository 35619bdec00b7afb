"""K-nearest search and K-blended skinning on the host emulation of the kernel sources (CPU twins of tests/test_gpu_knn.py; the check
functions live in tests/knn_cases.py)."""
import knn_cases as KC


def test_emul_knnk_equals_the_restatement_and_the_grid_the_exhaustive_search(emul):
    KC.check_knnk_search(emul, nv=400, nq=300)


def test_emul_knnk_counted_rows(emul):
    KC.check_knnk_counted(emul)


def test_emul_knn_arguments_are_validated_before_any_launch(emul):
    KC.check_knn_argument_errors(emul)


def test_emul_lbsk_reference_golden(emul):
    KC.check_lbsk_golden(emul)


def test_reference_golden_lies_within_the_quoted_distance_of_the_float64_chain():
    """the figures in check_lbsk_golden's docstring: 4x the reference's own float32 distance from the float64 chain is inside the K = 1 bars"""
    for K, r in KC.measure_reference_distance().items():
        assert 4 * r['posed_abs'] < 5e-6 and 4 * r['canonical_abs'] < 5e-6 and 4 * r['d_pts_rel'] < 1e-4 and 4 * r['d_trans_rel'] < 1e-4, (K, r)


def test_emul_lbsk_gradient_through_the_blend_weights(emul):
    for K in (2, 4, 8):
        for nb in (1, 4):
            KC.check_lbsk_grad(emul, K, nb, P=200)


def test_emul_knn_points_shim_contract(emul):
    KC.check_shim(emul)


def test_emul_deformer_k(emul):
    KC.check_deformer_k(emul)


def test_emul_launch_ahead_of_the_sizes_equals_the_plain_order_with_k4(emul, monkeypatch):
    KC.check_launch_ahead_k(emul, monkeypatch, res=32, grid_n=6, frames=2, ticks=3, prefit=150, body_verts=300, samples=64)
