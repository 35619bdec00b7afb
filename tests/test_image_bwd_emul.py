"""Image-space backward tail on the host emulation: texture d_x from the MLP half, G-buffer backward summed in LDS (tests/image_bwd_cases.py)."""
import image_bwd_cases as IC


def test_emul_tex_dx_fused(emul):
    IC.check_tex_dx_fused(emul, n=700)


def test_emul_tex_dx_partial_chains_and_waves(emul):
    IC.check_tex_dx_partial(emul)


def test_emul_tex_dx_all_masked(emul):
    IC.check_tex_dx_all_masked(emul)


def test_emul_tex_dx_tiny_upstream(emul):
    IC.check_tex_dx_tiny_upstream(emul)


def test_emul_tex_dx_x_without_grad(emul):
    IC.check_tex_dx_x_without_grad(emul)


def test_emul_tex_dx_async_on_off(emul):
    IC.check_tex_dx_async_on_off(emul)


def test_emul_gbuf_lds_mesh(emul):
    IC.check_gbuf_lds_mesh(emul)


def test_emul_gbuf_lds_tiles(emul):
    IC.check_gbuf_lds_tiles(emul)


def test_emul_gbuf_lds_one_triangle_and_empty_frame(emul):
    IC.check_gbuf_lds_one_triangle(emul)


def test_emul_gbuf_lds_overflow(emul):
    IC.check_gbuf_lds_overflow(emul)
