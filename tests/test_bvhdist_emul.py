"""Distance queries on the BVH -- nearest triangle, hierarchical winding number, signed distance, their opt-in wiring -- on the host emulation of the
kernel sources (CPU twins of tests/test_gpu_bvhdist.py; the check functions, the yardsticks and the parity rule live in tests/bvhdist_cases.py)."""
import pytest

import bvhdist_cases as BC

WALK_MESHES = tuple(m for m in BC.MESHES if m != 'soup0')


@pytest.mark.parametrize('name', BC.MESHES)
def test_emul_nearest_distance_triangle_and_barycentrics_match_the_float64_loop(emul, name):
    BC.check_nearest(emul, name)


def test_emul_nearest_ties_go_to_the_smallest_original_index(emul):
    BC.check_nearest_ties(emul)


@pytest.mark.parametrize('name', BC.NO_ZERO_AREA)
def test_emul_nearest_distance_is_the_brute_force_minimum(emul, name):
    BC.check_nearest_bits(emul, name, exact=True)


def test_emul_nearest_empty_scene_non_finite_queries_and_batch_shapes(emul):
    BC.check_nearest_edges(emul)


@pytest.mark.parametrize('name', WALK_MESHES)
def test_emul_leaf_map_and_tree_links(emul, name):
    BC.check_tree_and_leaf_map(emul, name)


@pytest.mark.parametrize('name', WALK_MESHES)
def test_emul_node_moments_match_float64_sums_over_the_subtrees(emul, name):
    BC.check_moments(emul, name)


@pytest.mark.parametrize('beta', BC.BETAS)
@pytest.mark.parametrize('name', WALK_MESHES)
def test_emul_winding_matches_the_float64_walk_of_the_tree(emul, name, beta):
    BC.check_winding_walk(emul, name, beta)


@pytest.mark.parametrize('name', BC.MESHES)
def test_emul_winding_at_beta_inf_is_the_exact_sum(emul, name):
    BC.check_winding_exact(emul, name)


@pytest.mark.parametrize('name', ('ico', 'ico_open'))
def test_emul_signed_distance_sign_agrees_with_the_float64_winding_number(emul, name):
    BC.check_sign(emul, name)


@pytest.mark.parametrize('name', ('ico', 'ico_open'))
def test_emul_mesh_wsdf_accel_bvh(emul, name):
    BC.check_mesh_wsdf_accel(emul, name)


def test_emul_watertight_accel_bvh(emul):
    BC.check_watertight_accel(emul)


def test_emul_garment_field_builds_one_bvh_for_all_rounds(emul):
    BC.check_garment_field_builds_once(emul)


def test_emul_defaults_build_no_bvh_and_keep_their_bits(emul):
    BC.check_defaults_are_untouched(emul)


def test_emul_flag_mesh_sdf_accel_reaches_the_body_tet_mesh(emul):
    BC.check_flag_mesh_sdf_accel(emul)


def test_emul_arguments_are_validated_before_any_native_call(emul, monkeypatch):
    BC.check_validation(emul, monkeypatch)


@pytest.mark.parametrize('name', ('ico', 'ico_open'))
def test_emul_walker_alone_keeps_the_shares_left_out_under_their_caps(emul, name):
    """the caps on the queries left out (borderline accept tests: 1 %; within tau of |w| = 0.5: 5 %), from the float64 walker alone"""
    for beta in BC.BETAS:
        BC.check_winding_walk(emul, name, beta, kernel=False)
    BC.sign_case(emul, name)
