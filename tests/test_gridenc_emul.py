"""The general grid encoding on the host emulation of the kernel sources (CPU twins of tests/test_gpu_gridenc.py; the check functions and
the float64 restatement live in tests/gridenc_cases.py)."""
import gridenc_cases as GC


def test_emul_gridenc_reference_configuration_equals_the_oracle_and_the_fused_kernels(emul):
    GC.check_anchor(emul, n=2000)


def test_emul_gridenc_hashed_levels_with_collisions(emul):
    GC.check_hashed_collisions(emul)


def test_emul_gridenc_matrix_of_dims_features_interpolation_and_type(emul):
    GC.check_matrix(emul, n=300)


def test_emul_gridenc_accumulation_of_coherent_and_identical_points(emul):
    GC.check_accumulation(emul, T=14, m=1024, n_same=500)


def test_emul_gridenc_edges(emul):
    GC.check_edges(emul)


def test_emul_gridenc_rows_outside_the_unit_cube_and_non_finite_rows_stay_inside_the_table(emul):
    GC.check_out_of_range(emul, nonfinite=True)


def test_emul_gridenc_configurations_are_validated_before_any_launch(emul):
    GC.check_validation(emul)


def test_emul_tcnn_encoding_shim_and_texture_routing(emul, monkeypatch):
    GC.check_shim(emul, monkeypatch)


def test_emul_mlptexture_with_a_16_level_grid(emul):
    GC.check_texture(emul, 400, enc_cfg=GC.cfg16(14))


def test_emul_mlptexture_with_another_network_shape(emul):
    GC.check_texture(emul, 400, channels=9, internal_dims=64, hidden=3)
