"""Image-space backward tail on the GPU: texture d_x from the MLP half, G-buffer backward summed in LDS (tests/image_bwd_cases.py)."""
import pytest

import image_bwd_cases as IC

pytestmark = pytest.mark.gpu


def test_gpu_tex_dx_fused(gpu):
    IC.check_tex_dx_fused(gpu, n=700)


def test_gpu_tex_dx_partial_chains_and_waves(gpu):
    IC.check_tex_dx_partial(gpu)


def test_gpu_tex_dx_all_masked(gpu):
    IC.check_tex_dx_all_masked(gpu)


def test_gpu_tex_dx_tiny_upstream(gpu):
    IC.check_tex_dx_tiny_upstream(gpu)


def test_gpu_tex_dx_x_without_grad(gpu):
    IC.check_tex_dx_x_without_grad(gpu)


def test_gpu_tex_dx_async_on_off(gpu):
    IC.check_tex_dx_async_on_off(gpu)


def test_gpu_gbuf_lds_mesh(gpu):
    IC.check_gbuf_lds_mesh(gpu)


def test_gpu_gbuf_lds_tiles(gpu):
    IC.check_gbuf_lds_tiles(gpu)


def test_gpu_gbuf_lds_one_triangle_and_empty_frame(gpu):
    IC.check_gbuf_lds_one_triangle(gpu)


def test_gpu_gbuf_lds_overflow(gpu):
    IC.check_gbuf_lds_overflow(gpu)


def test_gpu_gbuf_lds_1080(gpu):
    IC.check_gbuf_lds_1080(gpu)
