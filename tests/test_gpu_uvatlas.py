"""Textured-mesh export -- atlas, bake, mip op, Texture2D, material, export -- on the MI355X (GPU twins of tests/test_uvatlas_emul.py; the
check functions, the yardstick and the parity rule live in tests/uvatlas_cases.py)."""
import pytest

import uvatlas_cases as UC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', UC.CASES)
def test_gpu_atlas_layout_matches_the_integer_restatement(gpu, case):
    UC.check_layout(gpu, case)


def test_gpu_atlas_of_an_empty_mesh(gpu):
    UC.check_layout_empty(gpu)


def test_gpu_atlas_refuses_a_texture_that_is_too_small(gpu):
    UC.check_layout_too_small(gpu)


def test_gpu_atlas_rotation_rule(gpu):
    UC.check_rotation_rule(gpu)


@pytest.mark.parametrize('case', UC.CASES)
def test_gpu_bake_matches_the_yardstick(gpu, case):
    UC.check_bake(gpu, case)


@pytest.mark.parametrize('case', UC.CASES)
def test_gpu_bilinear_lookups_never_leave_their_triangle(gpu, case):
    UC.check_seamfree(gpu, case)


def test_gpu_bake_agrees_with_the_rasterised_uv_chart(gpu):
    UC.check_against_rasteriser(gpu)


@pytest.mark.parametrize('i', range(len(UC.MIP_SHAPES)))
def test_gpu_mip_forward_and_backward(gpu, i):
    UC.check_mip(gpu, i)


def test_gpu_mip_refuses_odd_sizes(gpu):
    UC.check_mip_odd_raises(gpu)


def test_gpu_texture2d_reproduces_the_golden(gpu):
    UC.check_texture2d_golden(gpu)


def test_gpu_material_round_trip(gpu, tmp_path):
    UC.check_material_roundtrip(gpu, tmp_path)


def test_gpu_export_end_to_end(gpu, tmp_path):
    UC.check_export(gpu, tmp_path)


def test_gpu_entry_points_validate_their_arguments(gpu):
    UC.check_entry_points_validate(gpu)
