"""Textured-mesh export -- atlas, bake, mip op, Texture2D, material, export -- on the host emulation of the kernel sources (CPU twins of
tests/test_gpu_uvatlas.py; the check functions, the yardstick and the parity rule live in tests/uvatlas_cases.py)."""
import pytest

import uvatlas_cases as UC


@pytest.mark.parametrize('case', UC.CASES)
def test_emul_atlas_layout_matches_the_integer_restatement(emul, case):
    UC.check_layout(emul, case)


def test_emul_atlas_of_an_empty_mesh(emul):
    UC.check_layout_empty(emul)


def test_emul_atlas_refuses_a_texture_that_is_too_small(emul):
    UC.check_layout_too_small(emul)


def test_emul_atlas_rotation_rule(emul):
    UC.check_rotation_rule(emul)


@pytest.mark.parametrize('case', UC.CASES)
def test_emul_bake_matches_the_yardstick(emul, case):
    UC.check_bake(emul, case)


@pytest.mark.parametrize('case', UC.CASES)
def test_emul_bilinear_lookups_never_leave_their_triangle(emul, case):
    UC.check_seamfree(emul, case)


def test_emul_bake_agrees_with_the_rasterised_uv_chart(emul):
    UC.check_against_rasteriser(emul)


@pytest.mark.parametrize('i', range(len(UC.MIP_SHAPES)))
def test_emul_mip_forward_and_backward(emul, i):
    UC.check_mip(emul, i)


def test_emul_mip_refuses_odd_sizes(emul):
    UC.check_mip_odd_raises(emul)


def test_emul_texture2d_reproduces_the_golden(emul):
    UC.check_texture2d_golden(emul)


def test_emul_material_round_trip(emul, tmp_path):
    UC.check_material_roundtrip(emul, tmp_path)


def test_emul_export_end_to_end(emul, tmp_path):
    UC.check_export(emul, tmp_path)


def test_emul_entry_points_validate_their_arguments(emul):
    UC.check_entry_points_validate(emul)
