"""Distance queries on the BVH -- nearest triangle, hierarchical winding number, signed distance, their opt-in wiring -- on the MI355X (GPU twins of
tests/test_bvhdist_emul.py; the check functions, the yardsticks and the parity rule live in tests/bvhdist_cases.py)."""
import pytest

import bvhdist_cases as BC

pytestmark = pytest.mark.gpu

WALK_MESHES = tuple(m for m in BC.MESHES if m != 'soup0')


@pytest.mark.parametrize('name', BC.MESHES)
def test_gpu_nearest_distance_triangle_and_barycentrics_match_the_float64_loop(gpu, name):
    BC.check_nearest(gpu, name)


def test_gpu_nearest_ties_go_to_the_smallest_original_index(gpu):
    BC.check_nearest_ties(gpu)


@pytest.mark.parametrize('name', BC.NO_ZERO_AREA)
def test_gpu_nearest_distance_is_the_brute_force_minimum(gpu, name):
    BC.check_nearest_bits(gpu, name, exact=False)


def test_gpu_nearest_empty_scene_non_finite_queries_and_batch_shapes(gpu):
    BC.check_nearest_edges(gpu)


@pytest.mark.parametrize('name', WALK_MESHES)
def test_gpu_leaf_map_and_tree_links(gpu, name):
    BC.check_tree_and_leaf_map(gpu, name)


@pytest.mark.parametrize('name', WALK_MESHES)
def test_gpu_node_moments_match_float64_sums_over_the_subtrees(gpu, name):
    BC.check_moments(gpu, name)


@pytest.mark.parametrize('beta', BC.BETAS)
@pytest.mark.parametrize('name', WALK_MESHES)
def test_gpu_winding_matches_the_float64_walk_of_the_tree(gpu, name, beta):
    BC.check_winding_walk(gpu, name, beta)


@pytest.mark.parametrize('name', BC.MESHES)
def test_gpu_winding_at_beta_inf_is_the_exact_sum(gpu, name):
    BC.check_winding_exact(gpu, name)


@pytest.mark.parametrize('name', ('ico', 'ico_open'))
def test_gpu_signed_distance_sign_agrees_with_the_float64_winding_number(gpu, name):
    BC.check_sign(gpu, name)


@pytest.mark.parametrize('name', ('ico', 'ico_open'))
def test_gpu_mesh_wsdf_accel_bvh(gpu, name):
    BC.check_mesh_wsdf_accel(gpu, name)


def test_gpu_watertight_accel_bvh(gpu):
    BC.check_watertight_accel(gpu)


def test_gpu_garment_field_builds_one_bvh_for_all_rounds(gpu):
    BC.check_garment_field_builds_once(gpu)


def test_gpu_defaults_build_no_bvh_and_keep_their_bits(gpu):
    BC.check_defaults_are_untouched(gpu)


def test_gpu_flag_mesh_sdf_accel_reaches_the_body_tet_mesh(gpu):
    BC.check_flag_mesh_sdf_accel(gpu)


def test_gpu_arguments_are_validated_before_any_native_call(gpu, monkeypatch):
    BC.check_validation(gpu, monkeypatch)
