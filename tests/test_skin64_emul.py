"""The K = 1 skinning chain against float64, per element and at its edges, on the host emulation of csrc/smplx_pose.hip and csrc/lbs.hip (CPU
twins of tests/test_gpu_skin64.py; the cases, the float64 reference and the rules live in tests/skin64_cases.py)."""
import pytest

import skin64_cases as SC

_ids = lambda cases: [c['tag'][c['tag'].index(' ') + 1:].replace(' ', '-') for c in cases]
POSE = [(g, c) for g, cs in SC.POSE_GROUPS.items() for c in cs]
LBS = [(g, c) for g, cs in SC.LBS_GROUPS.items() for c in cs]


@pytest.mark.parametrize('group,case', POSE, ids=_ids([c for _, c in POSE]))
def test_emul_skin64_pose_transforms_and_vjp_vs_float64(emul, group, case):
    SC.run_pose(emul, group, case)


@pytest.mark.parametrize('group,case', LBS, ids=_ids([c for _, c in LBS]))
def test_emul_skin64_lbs_forward_and_vjp_vs_float64(emul, group, case):
    SC.run_lbs(emul, group, case)


def test_emul_skin64_lbs_no_points(emul):
    SC.run_lbs_empty(emul)


@pytest.mark.parametrize('P', [2, 1000])
def test_emul_skin64_lbs_gradient_subsets_equal_the_full_run(emul, P):
    SC.run_lbs_subsets(emul, P)


@pytest.mark.parametrize('kind', list(SC.COUNTED))
def test_emul_skin64_counted_forward_and_search_equal_the_plain_calls(emul, kind):
    SC.run_counted(emul, kind)


def test_emul_skin64_whole_chain_pose_to_posed_points(emul):
    SC.run_chain(emul)


@pytest.mark.parametrize('group', SC.GROUPS)
def test_emul_skin64_decade_bands_within_three_times_the_float32_oracle(emul, group):
    SC.check_group(emul, group)


def test_emul_skin64_wrappers_refuse_bad_arguments_before_any_launch(emul):
    SC.check_validation(emul)


def test_skin64_inputs_have_the_edges_they_claim():
    """the inputs, without a kernel: weight rows one-hot / four / dense / off-1 sums, trees, rotation sizes, and the power of rule (b)"""
    import torch
    g = SC._gen('inputs')
    w = SC.weight_table('onehot', 50, 55, g)
    assert bool(((w != 0).sum(1) == 1).all()) and bool((w.sum(1) == 1).all())
    assert bool(((SC.weight_table('four', 50, 55, g) != 0).sum(1) == 4).all())
    assert bool((SC.weight_table('dense', 50, 55, g) != 0).all())
    assert abs(float(SC.weight_table('s1.001', 50, 55, g).sum(1).mean()) - 1.001) < 1e-6
    assert abs(float(SC.weight_table('s0.9', 50, 55, g).sum(1).mean()) - 0.9) < 1e-6
    assert SC.tree('chain64') == list(range(-1, 63)) and len(SC.tree('smplx')) == 55 and SC.tree('star64')[1:] == [0] * 63
    assert all(0 <= p < j for name in SC.TREES for j, p in enumerate(SC.tree(name)) if j)
    for kind, a in SC.SCALES.items():
        n = SC.rotations(kind, 3, 7, g).double().norm(dim=-1)
        assert bool(((n - a).abs() <= 1e-6 * max(a, 1e-30)).all()) if a else not bool(n.any()), kind
    ax = SC.rotations('axes', 5, 55, g)
    assert bool(((ax != 0).sum(-1) == 1).all()) and {round(float(v), 3) for v in ax.abs().amax(-1).reshape(-1)} == {3.141, 3.142, 3.143, 7.0}
    d = SC.lbs_inputs(SC.lbs_case(1000, nb=3, cond=True))
    M0 = torch.einsum('pj,jab->pab', d['lbs_w'].double()[d['idx'].long()], d['A0'].double())[:, :3, :3]
    cond = torch.linalg.cond(M0)
    assert 50 < float(cond.median()) < 200, float(cond.median())
    span = d['gout'].abs().amax(-1).log10()
    assert float(span.min()) < -5.5 and float(span.max()) > 1.5
    assert SC.bound_factor(1024) * 1024 < 1          # P <= 1024: the largest term (>= the mean) always exceeds the bound


def test_skin64_band_exception_covers_only_the_bands_it_names():
    assert SC.band_bar('pose-smplx', 'd_J', -19) == 5.1 and SC.band_bar('pose-smplx', 'd_J', -12) == 5.1
    for top in (-20, -18, -13, -11, -4, 0, 3, SC.ZERO_BAND):
        assert SC.band_bar('pose-smplx', 'd_J', top) == SC.RATIO
    assert SC.band_bar('pose-trees', 'd_J', -19) == SC.RATIO and SC.band_bar('pose-smplx', 'd_fp', -19) == SC.RATIO
    acc = {SC.ZERO_BAND: [10, 0, 0, 0], -19: [100, 0, 0, 0], -12: [5, 0, 0, 0], -11: [70, 0, 0, 0], 0: [3, 0, 0, 0]}
    assert SC._top_decades(acc) == [-19, 0] and len(SC.merged_bands(acc)) == 2         # a band joined to higher decades is another band: it keeps 3
