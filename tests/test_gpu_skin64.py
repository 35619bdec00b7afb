"""The K = 1 skinning chain against float64, per element and at its edges, on the MI355X (the cases, the float64 reference and the rules live
in tests/skin64_cases.py)."""
import pytest

import skin64_cases as SC

pytestmark = pytest.mark.gpu

_ids = lambda cases: [c['tag'][c['tag'].index(' ') + 1:].replace(' ', '-') for c in cases]
POSE = [(g, c) for g, cs in SC.POSE_GROUPS.items() for c in cs]
LBS = [(g, c) for g, cs in SC.LBS_GROUPS.items() for c in cs]


@pytest.mark.parametrize('group,case', POSE, ids=_ids([c for _, c in POSE]))
def test_gpu_skin64_pose_transforms_and_vjp_vs_float64(gpu, group, case):
    SC.run_pose(gpu, group, case)


@pytest.mark.parametrize('group,case', LBS, ids=_ids([c for _, c in LBS]))
def test_gpu_skin64_lbs_forward_and_vjp_vs_float64(gpu, group, case):
    SC.run_lbs(gpu, group, case)


def test_gpu_skin64_lbs_no_points(gpu):
    SC.run_lbs_empty(gpu)


@pytest.mark.parametrize('P', [2, 1000])
def test_gpu_skin64_lbs_gradient_subsets_equal_the_full_run(gpu, P):
    SC.run_lbs_subsets(gpu, P)


@pytest.mark.parametrize('kind', list(SC.COUNTED))
def test_gpu_skin64_counted_forward_and_search_equal_the_plain_calls(gpu, kind):
    SC.run_counted(gpu, kind)


def test_gpu_skin64_whole_chain_pose_to_posed_points(gpu):
    SC.run_chain(gpu)


@pytest.mark.parametrize('group', SC.GROUPS)
def test_gpu_skin64_decade_bands_within_three_times_the_float32_oracle(gpu, group):
    SC.check_group(gpu, group)


def test_gpu_skin64_wrappers_refuse_bad_arguments_before_any_launch(gpu):
    SC.check_validation(gpu)
