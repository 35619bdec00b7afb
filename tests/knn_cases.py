"""Checks of the K-nearest search and the K-blended skinning (csrc/lbs.hip: knnk / lbsk kernels, d3h/lbs.py, SMPLX_Deformer.k, the
pytorch3d.ops shim), shared by the emulator tests (tests/test_knn_emul.py) and the GPU tests (tests/test_gpu_knn.py): every function takes
the `emul` / `gpu` fixture value as `dev`, the way tests/parity_cases.py does.

Host restatements are written from the stated semantics: the search is fully specified in float32 (restate_knn, compared with
torch.equal); the skinning chain (deformer :363-421) is restated in torch at a chosen precision (lbsk_chain), float64 being the truth the
float32 kernels and the float32 reference are both measured against.
"""
import numpy as np
import torch

from conftest import golden
import parity_cases as PC

T = PC.T
KS_ALL = (1, 2, 3, 4, 8, 16, 32)


# ---- the search ------------------------------------------------------------------------------------------------------------------------
def restate_knn(pts, tmpl, K):
    """numpy float32: d = (dx*dx + dy*dy) + dz*dz, every operation rounded; the K smallest under (d, index), ascending.  A candidate whose
    d is not below +inf is never held; an empty slot is (0, +inf), a slot the template has no vertex for (nv..K-1) is (0, 0)"""
    pts, tmpl = np.asarray(pts, np.float32), np.asarray(tmpl, np.float32)
    P, nv = pts.shape[0], tmpl.shape[0]
    with np.errstate(invalid='ignore', over='ignore'):
        dx, dy, dz = (pts[:, None, a] - tmpl[None, :, a] for a in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        ok = d < np.inf
    dm = np.where(ok, d, np.float32(np.inf))
    ids = np.broadcast_to(np.arange(nv, dtype=np.int64), (P, nv))
    order = np.lexsort((ids, dm), axis=-1)[:, :K]
    idx = np.zeros((P, K), np.int32)
    d2 = np.zeros((P, K), np.float32)
    n = min(K, nv)
    held = np.take_along_axis(ok, order, 1)
    idx[:, :n] = np.where(held, order, 0)
    d2[:, :n] = np.where(held, np.take_along_axis(dm, order, 1), np.float32(np.inf))
    return torch.from_numpy(idx), torch.from_numpy(d2)


def knn_scene(dev, nv, nq, seed):
    """the scene of parity_cases.check_knn_grid: ellipsoid-shell template with 40 exact duplicate vertices; queries near it, far outside its
    box, exactly on vertices (the first 40 of them on duplicated ones), non-finite, on midpoints"""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(nv, 3, generator=g)
    tmpl = u / u.norm(dim=1, keepdim=True) * torch.tensor([0.3, 0.8, 0.2]) + torch.tensor([0.0, -0.3, 0.05])
    if nv >= 100:
        tmpl[nv // 2:nv // 2 + 40] = tmpl[:40]
    tmpl = tmpl.to(dev).contiguous()
    near = tmpl[torch.randint(0, nv, (nq,), generator=g).to(dev)] + 0.03 * torch.randn(nq, 3, generator=g).to(dev)
    far = (torch.rand(200, 3, generator=g).to(dev) * 2 - 1) * 5.0
    onv = tmpl[:100].clone()
    bad = torch.tensor([[float('nan'), 0, 0], [float('inf'), 0, 0], [0, float('-inf'), 0]], device=dev)
    mid = 0.5 * (tmpl[:50] + tmpl[50:100])
    pts = torch.cat([near, far, onv, bad, mid]).contiguous()
    return tmpl, pts, dict(onv=nq + 200, bad=nq + 300, special=nq)


def _same(a, b, what):
    assert torch.equal(a.idx.cpu(), b.idx.cpu()), f'{what}: indices differ in {int((a.idx.cpu() != b.idx.cpu()).any(1).sum())} queries'
    da, db = a.d2.cpu(), b.d2.cpu()
    assert torch.equal(da, db), f'{what}: distances differ'


def check_knnk_search(dev, nv=1500, nq=3000, seed=0, Ks=KS_ALL, degenerate=True):
    """exhaustive search == host restatement and grid search == exhaustive search, indices AND squared distances with torch.equal, no exempted
    query; K = 1 == d3h_knn1; duplicated vertices: both copies, the lower index first; non-finite queries: index 0 in every slot"""
    from d3h import lbs as HL
    tmpl, pts, at = knn_scene(dev, nv, nq, seed)
    grid = HL.KnnGrid(tmpl)
    sub = torch.arange(0, pts.shape[0], max(1, pts.shape[0] * nv // 4_000_000))          # restatement: bounded [q, nv] distance matrix
    sub = torch.cat([sub, torch.arange(at['special'], pts.shape[0])]).unique()
    for K in Ks:
        e = HL.knnk(pts, tmpl, K)
        assert e.idx.dtype == torch.int32 and e.d2.dtype == torch.float32 and tuple(e.idx.shape) == tuple(e.d2.shape) == (pts.shape[0], K)
        ri, rd = restate_knn(pts.cpu()[sub], tmpl.cpu(), K)
        assert torch.equal(e.idx.cpu()[sub], ri), (K, 'indices differ from the restatement')
        assert torch.equal(e.d2.cpu()[sub], rd), (K, 'distances differ from the restatement')
        _same(HL.knnk(pts, tmpl, K, grid=grid), e, f'grid vs exhaustive, K={K}')
        bad = e.idx[at['bad']:at['bad'] + 3].cpu()
        assert int(bad.abs().max()) == 0 and bool(torch.isinf(e.d2[at['bad']:at['bad'] + 3]).all())
        if K == 1:
            i1, d1 = grid.query(pts, want_dist=True)
            assert torch.equal(e.idx[:, 0].cpu(), HL.knn1(pts, tmpl).cpu()) and torch.equal(e.idx[:, 0].cpu(), i1.cpu())
            assert torch.equal(e.d2[:, 0].cpu(), d1.cpu())
        elif nv >= 100:
            dup = e.idx[at['onv']:at['onv'] + 40].cpu().long()                              # queries ON duplicated vertices 0..39
            want = torch.arange(40)
            assert torch.equal(dup[:, 0], want) and torch.equal(dup[:, 1], want + nv // 2), (K, 'duplicates: both copies, lower index first')
            assert bool((e.d2[at['onv']:at['onv'] + 40, :2] == 0).all())
    if not degenerate:
        return
    for tiny in (1, 2, 17):                                                               # K > nv: slots nv..K-1 are (0, 0)
        t2 = tmpl[:tiny].contiguous()
        for K in (tiny + 1, 4, 32):
            if K <= tiny:
                continue
            e = HL.knnk(pts, t2, K)
            ri, rd = restate_knn(pts.cpu(), t2.cpu(), K)
            assert torch.equal(e.idx.cpu(), ri) and torch.equal(e.d2.cpu(), rd), (tiny, K)
            assert int(e.idx[:, tiny:].abs().max()) == 0 and float(e.d2[:, tiny:].abs().max()) == 0.0
            _same(HL.KnnGrid(t2).query_k(pts, K), e, f'grid vs exhaustive, nv={tiny}, K={K}')
    flat = tmpl.clone(); flat[:, 2] = 0.25
    for K in (2, 8):
        e = HL.knnk(pts, flat, K)
        ri, rd = restate_knn(pts.cpu()[sub], flat.cpu(), K)
        assert torch.equal(e.idx.cpu()[sub], ri) and torch.equal(e.d2.cpu()[sub], rd)
        _same(HL.KnnGrid(flat).query_k(pts, K), e, f'flat template, K={K}')
    for r in (HL.knnk(pts[:0], tmpl, 4), grid.query_k(pts[:0], 4)):
        assert tuple(r.idx.shape) == (0, 4) and tuple(r.d2.shape) == (0, 4)


def check_knnk_counted(dev, nv=400, nq=300, K=4):
    """query_k_counted over a capacity buffer == query_k on the counted rows; the other rows stay unwritten"""
    from d3h import lbs as HL
    tmpl, pts, _ = knn_scene(dev, nv, nq, 3)
    grid = HL.KnnGrid(tmpl)
    cap = pts.shape[0]
    for c in ((7, 11, 5, 0), (cap, 5, 5, 0), (0, 0, 0, 0), (50, 0, 0, 1)):               # rows = c0 + 3 c1 + 4 c2; c[3]: the overflow flag
        counts = torch.zeros(16, dtype=torch.int32)
        counts[0], counts[1], counts[2], counts[10] = c
        rows = 0 if c[3] else min(cap, c[0] + 3 * c[1] + 4 * c[2])
        out = HL.KnnResult(torch.full((cap, K), -7, dtype=torch.int32, device=dev), torch.full((cap, K), -7.0, device=dev))
        r = grid.query_k_counted(pts, counts.to(dev), K, out=out)
        _same(r[:rows], grid.query_k(pts[:rows].contiguous(), K), f'counted rows {rows}')
        assert bool((r.idx[rows:] == -7).all()) and bool((r.d2[rows:] == -7.0).all()), 'rows beyond the count were written'


def check_knn_argument_errors(dev):
    import pytest
    from d3h import lbs as HL
    tmpl, pts, _ = knn_scene(dev, 120, 10, 0)
    for K in (0, 33, -1, 2.0, True):
        with pytest.raises(ValueError):
            HL.knnk(pts, tmpl, K)
    with pytest.raises(RuntimeError):
        HL.knnk(pts[:, :2], tmpl, 2)
    with pytest.raises(RuntimeError):
        HL.knnk(pts, tmpl[:0], 2)
    nn = HL.knnk(pts, tmpl, 2)
    z = torch.zeros
    with pytest.raises(RuntimeError):                                                     # rows of the search result != rows of pts
        HL.lbs_points_k(pts[:5].contiguous(), nn, z(120, 55, device=dev), tmpl, z(55, 4, 4, device=dev), z(1, 55, 4, 4, device=dev), z(1, 3, device=dev))
    with pytest.raises(RuntimeError):                                                     # int64 ids
        HL.lbs_points_k(pts, HL.KnnResult(nn.idx.long(), nn.d2), z(120, 55, device=dev), tmpl, z(55, 4, 4, device=dev), z(1, 55, 4, 4, device=dev),
                        z(1, 3, device=dev))


# ---- the skinning chain at a chosen precision ----------------------------------------------------------------------------------------------
def lbsk_chain(pts, idx, tmpl, W, A0, A, trans, hold_weights=False):
    """deformer :363-421 for given neighbour ids, in the dtype of `pts`: inverse-distance blend of the K weight rows, M0 = sum_j w_j A0_j
    inverted as a full 4x4, canonical point, M = sum_j w_j A_j, posed point + trans.  -> (posed [B,P,3], w [P,J], canonical [P,3]).
    hold_weights: the blend weights are constants (what a backward without the weight path computes)"""
    dt = pts.dtype
    tmpl, W, A0, A, trans = (t.to(dt) for t in (tmpl, W, A0, A, trans))
    d2 = ((pts[:, None] - tmpl[idx]) ** 2).sum(-1)
    dist = torch.sqrt(d2 + 1e-9)
    u = 1.0 / (dist + 1e-9)
    a = u / u.sum(1, keepdim=True)
    if hold_weights:
        a = a.detach()
    w = (W[idx] * a[..., None]).sum(1)
    ph = torch.cat([pts, torch.ones_like(pts[:, :1])], 1)[..., None]
    can = (torch.inverse(torch.einsum('pj,jmn->pmn', w, A0)) @ ph)[:, :3, 0]
    ch = torch.cat([can, torch.ones_like(can[:, :1])], 1)[..., None]
    out = torch.stack([(torch.einsum('pj,jmn->pmn', w, A[b]) @ ch)[:, :3, 0] + trans[b] for b in range(A.shape[0])])
    return out, w, can


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _golden_deformer(dev, k=1):
    g, d = PC._lbs_setup(dev)
    d.k = k
    d.vs_template = T(g['tmpl'], dev)[None]
    betas = T(g['betas'], dev)
    z = lambda n: torch.zeros(1, n, device=dev)
    body0 = z(63); body0[:, 2] = torch.pi / 36; body0[:, 5] = -torch.pi / 36
    d.init_A = d.layer.transforms(betas, z(3), body0, z(3), z(5))
    param = lambda: {'shape': betas, 'face_offset': T(g['face_offset'], dev), 'joint_offset': T(g['joint_offset'], dev),
                     'locator_offset': T(g['locator_offset'], dev), 'trans': T(g['trans'], dev, True), 'jaw_pose': T(g['jaw'], dev),
                     'expr': T(g['expr'], dev), 'body_pose': T(g['body_pose'], dev, True), 'root_pose': T(g['root_pose'], dev, True)}
    return g, d, param


# measure_reference_distance(): against the float64 chain on the golden's inputs and neighbour ids (the reference's A0 / A taken as given) the
# reference's own float32 results lie within  posed 2.6e-7 and canonical 1.9e-7 absolute, d_pts 1.0e-6 (k=2) / 4.4e-7 (k=4) and d_trans 9.2e-8
# relative.  4x that is far inside the K = 1 bars, which therefore stay: 5e-6 absolute on points, 1e-4 relative on gradients
def check_lbsk_golden(dev, report=print):
    """tests/golden/lbs_knn.npz (tools/gen_golden_knn.py): the reference's SMPLX_Deformer with k in {2, 4} -- neighbour ids exact; blended
    weights, canonical and posed points for 3 frames and the gradients of pts / trans / body_pose / root_pose at the K = 1 bars of
    parity_cases.check_lbs_golden (5e-6 absolute on points, 1e-4 relative on gradients).

    The bars were not widened: the float64 chain on the same ids puts the reference's own float32 results within 2.6e-7 (posed points,
    absolute) and 1.0e-6 (d_pts, relative) of the truth (measure_reference_distance), so 4x the reference's distance lies well inside the
    K = 1 bars.  Measured on the host emulation: posed 4.8e-7, d_pts 2.1e-6 (k=2) / 8.9e-7 (k=4), the other gradients below 4e-7; on the
    MI355X: posed 4.8e-7, d_pts 2.0e-6 / 7.6e-7, the other gradients below 3e-7."""
    gk = golden('lbs_knn.npz')
    for K in (2, 4):
        g, d, mk = _golden_deformer(dev, K)
        pts = T(g['pts'], dev, True)
        nn = d.nearest(pts)
        assert np.array_equal(nn.idx.cpu().numpy(), gk[f'k{K}.idx']), f'k={K}: neighbour ids differ from the reference'
        w = d.interpolate_weights(pts.detach()[None])[0]
        e_w = float((w.cpu() - torch.from_numpy(gk[f'k{K}.w_pts'])).abs().max())
        can = d.lbs_forward_inverse(pts.detach()[None])[0]
        e_c = float((can.cpu() - torch.from_numpy(gk[f'k{K}.canonical'])).abs().max())
        param = mk()
        nfr = gk[f'k{K}.out'].shape[0]
        out = d.lbs_forward_batch(pts, param, range(nfr))
        e_o = float((out.detach().cpu() - torch.from_numpy(gk[f'k{K}.out'])).abs().max())
        one = d.lbs_forward(pts.detach().reshape(1, -1, 3), param, idx=1)
        e_1 = float((one.detach().cpu() - torch.from_numpy(gk[f'k{K}.out'][1])).abs().max())
        (out * T(g['gout'], dev)).sum().backward()
        rel = lambda a, b: float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))
        e_g = {n: rel(t.grad.cpu().numpy(), gk[f'k{K}.d_{n}']) for n, t in
               (('pts', pts), ('trans', param['trans']), ('body_pose', param['body_pose']), ('root_pose', param['root_pose']))}
        report(f'lbs_knn golden k={K}: w_pts {e_w:.2e} canonical {e_c:.2e} posed {e_o:.2e} single-frame {e_1:.2e} abs; grads rel {e_g}')
        assert e_w < 2e-6 and e_c < 5e-6 and e_o < 5e-6 and e_1 < 5e-6, (K, e_w, e_c, e_o, e_1)
        for n, v in e_g.items():
            assert v < 1e-4, (K, n, v)


def measure_reference_distance(report=print):
    """how far the reference's float32 golden lies from the float64 chain on the same neighbour ids (the figures quoted in
    check_lbsk_golden's docstring); host only"""
    g, gk = golden('lbs.npz'), golden('lbs_knn.npz')
    t = lambda a: torch.from_numpy(np.asarray(a))
    res = {}
    for K in (2, 4):
        pts = t(g['pts']).double().requires_grad_(True)
        trans = t(g['trans']).double().requires_grad_(True)
        out, w, can = lbsk_chain(pts, t(gk[f'k{K}.idx']).long(), t(g['tmpl']), t(g['model.weights']), t(g['A0']), t(g['A']), trans)
        (out * t(g['gout']).double()).sum().backward()
        res[K] = dict(posed_abs=float((out.detach() - t(gk[f'k{K}.out'])).abs().max()), canonical_abs=float((can.detach() - t(gk[f'k{K}.canonical'])).abs().max()),
                      w_abs=float((w.detach() - t(gk[f'k{K}.w_pts'])).abs().max()), d_pts_rel=_rel(t(gk[f'k{K}.d_pts']), pts.grad),
                      d_trans_rel=_rel(t(gk[f'k{K}.d_trans']), trans.grad))
        report(f'reference float32 vs float64 chain, k={K}: {res[K]}')
    return res


def check_lbsk_grad(dev, K, nb, P=400, report=print):
    """d_pts / dA / d_trans of the K-blended skinning against the float64 chain fed the kernel's own neighbour ids, points exactly on template
    vertices included (d2 = 0).  Bar: 4x the distance of the float32 evaluation of the same chain from the float64 one (the reference's own
    error: it IS that float32 chain), not below the project's K = 1 bar of 1e-4 relative.  The weight path must be present: the result is
    farther than the bar from the float64 gradient with the blend weights held constant.  Two backward runs are bit-identical."""
    from d3h import lbs as HL
    g, d, mk = _golden_deformer(dev, K)
    tmpl = d.vs_template[0]
    gen = torch.Generator().manual_seed(100 + K)
    nv = tmpl.shape[0]
    pts = tmpl[torch.randint(0, nv, (P,), generator=gen).to(dev)] + 0.02 * torch.randn(P, 3, generator=gen).to(dev)
    pts[:25] = tmpl[torch.randperm(nv, generator=gen)[:25].to(dev)]                        # exactly on a vertex
    pts = pts.contiguous()
    A = T(g['A'], dev)
    A = A[torch.arange(nb) % A.shape[0]].contiguous()
    trans = (0.1 * torch.randn(nb, 3, generator=gen)).to(dev)
    gout = torch.randn(nb, P, 3, generator=gen).to(dev)
    nn = HL.knnk(pts, tmpl, K)
    assert bool((nn.d2[:25, 0] == 0).all())

    def run_kernel():
        p, a, t = pts.clone().requires_grad_(True), A.clone().requires_grad_(True), trans.clone().requires_grad_(True)
        out = HL.lbs_points_k(p, nn, d.lbs_weights, tmpl, d.init_A[0], a, t)
        (out * gout).sum().backward()
        return out.detach(), p.grad, a.grad, t.grad

    def run_chain(dt, hold=False):
        p, a, t = (x.detach().cpu().to(dt).requires_grad_(True) for x in (pts, A, trans))
        out, _, _ = lbsk_chain(p, nn.idx.cpu().long(), tmpl.cpu(), d.lbs_weights.cpu(), d.init_A[0].detach().cpu(), a, t, hold_weights=hold)
        (out * gout.cpu().to(dt)).sum().backward()
        return out.detach(), p.grad, a.grad, t.grad

    k_out, k_p, k_a, k_t = run_kernel()
    t_out, t_p, t_a, t_t = run_chain(torch.float64)
    f_out, f_p, f_a, f_t = run_chain(torch.float32)
    _, h_p, _, _ = run_chain(torch.float64, hold=True)
    assert bool(torch.isfinite(k_p).all()) and bool(torch.isfinite(t_p).all())
    rows3 = lambda a: a[:, :, :3, :]                                                       # the posed point reads rows 0..2 of A only
    for name, k, f, t in (('posed', k_out, f_out, t_out), ('d_pts', k_p, f_p, t_p), ('dA', rows3(k_a), rows3(f_a), rows3(t_a)), ('d_trans', k_t, f_t, t_t)):
        ref32, got = _rel(f, t), _rel(k, t)
        bar = max(1e-4, 4 * ref32) if name != 'posed' else max(5e-6 / float(t.abs().max()), 4 * ref32)
        report(f'lbsk K={K} nb={nb} {name}: kernel {got:.2e}, float32 chain {ref32:.2e}, bar {bar:.2e} (relative to max |float64|)')
        assert got <= bar, (K, nb, name, got, bar)
        if name == 'd_pts':
            missing = _rel(h_p, t)
            report(f'lbsk K={K} nb={nb}: float64 d_pts with the weights held constant lies {missing:.2e} from the full one; kernel to held: {_rel(k, h_p):.2e}')
            assert missing > 10 * bar and _rel(k, h_p) > bar, 'the weight path does not matter here: the test shows nothing'
    again = run_kernel()
    assert torch.equal(again[1], k_p), 'two backward runs differ in d_pts'


# ---- the pytorch3d.ops shim --------------------------------------------------------------------------------------------------------------
def check_shim(dev, report=print):
    import pytest
    from pytorch3d.ops import knn_points, knn_gather
    gen = torch.Generator().manual_seed(5)
    N, P1, P2, K = 2, 50, 40, 5
    p1 = torch.randn(N, P1, 3, generator=gen).to(dev).requires_grad_(True)
    p2 = torch.randn(N, P2, 3, generator=gen).to(dev).requires_grad_(True)
    l1 = torch.tensor([P1, 30], device=dev)
    l2 = torch.tensor([P2, 3], device=dev)
    r = knn_points(p1, p2, lengths1=l1, lengths2=l2, K=K, return_nn=True)
    assert tuple(r.dists.shape) == (N, P1, K) and r.dists.dtype == torch.float32
    assert tuple(r.idx.shape) == (N, P1, K) and r.idx.dtype == torch.int64 and not r.idx.requires_grad and r.dists.requires_grad
    assert tuple(r.knn.shape) == (N, P1, K, 3)
    assert float(r.dists.detach()[1, :, 3:].abs().max()) == 0 and int(r.idx[1, :, 3:].abs().max()) == 0          # lengths2 < K
    assert float(r.dists.detach()[1, 30:].abs().max()) == 0 and int(r.idx[1, 30:].abs().max()) == 0              # lengths1 < P1
    assert torch.equal(r.knn, knn_gather(p2, r.idx, l2)) and float(r.knn.detach()[1, :, 3:].abs().max()) == 0
    for n, (a, b) in enumerate(((P1, P2), (30, 3))):                                                     # every cloud == its own restatement
        ri, rd = restate_knn(p1[n, :a].detach().cpu(), p2[n, :b].detach().cpu(), K)
        assert torch.equal(r.idx[n, :a].cpu(), ri.long()) and torch.equal(r.dists[n, :a].detach().cpu(), rd)
    assert bool((r.dists[0, :, 1:] >= r.dists[0, :, :-1]).all())
    r.dists.sum().backward()

    def closed(dt):                                                                                      # knn_cpu.cpp:101-126, grad_dists = 1
        a, b, idx = p1.detach().cpu().to(dt), p2.detach().cpu().to(dt), r.idx.cpu()
        g1, g2 = torch.zeros_like(a), torch.zeros_like(b)
        for n in range(N):
            for i in range(int(l1[n])):
                for k in range(min(int(l2[n]), K)):
                    j = int(idx[n, i, k])
                    diff = 2.0 * (a[n, i] - b[n, j])
                    g1[n, i] += diff
                    g2[n, j] -= diff
        return g1, g2
    (t1, t2), (f1, f2) = closed(torch.float64), closed(torch.float32)
    for name, got, f, t in (('grad_p1', p1.grad, f1, t1), ('grad_p2', p2.grad, f2, t2)):
        ref32, e = _rel(f, t), _rel(got, t)
        bar = max(4 * ref32, 4 * 2.0 ** -23)               # 4x the float32 closed form's own distance, not below a few float32 roundings
        report(f'knn_points {name}: {e:.2e} from the float64 closed form, float32 closed form {ref32:.2e}, bar {bar:.2e}')
        assert e <= bar, (name, e, bar)
    # K = 1, no lengths, no gradient: the single-neighbour kernel, as before
    with torch.no_grad():
        r1 = knn_points(p1, p2, K=1, return_nn=True)
    ri, rd = restate_knn(p1[0].detach().cpu(), p2[0].detach().cpu(), 1)
    assert torch.equal(r1.idx[0].cpu(), ri.long()) and torch.equal(r1.dists[0].cpu(), rd) and tuple(r1.knn.shape) == (N, P1, 1, 3)
    # both values of return_sorted, and K = 1 WITH a gradient
    r2 = knn_points(p1, p2, K=3, return_sorted=False)
    assert torch.equal(r2.idx, knn_points(p1, p2, K=3).idx) and r2.knn is None
    assert knn_points(p1, p2, K=1).dists.requires_grad
    for kw, err in ((dict(norm=1), NotImplementedError), (dict(K=33), NotImplementedError), (dict(norm=3), ValueError)):
        with pytest.raises(err):
            knn_points(p1, p2, **{'K': 2, **kw})
    with pytest.raises(NotImplementedError):
        knn_points(p1[..., :2], p2[..., :2], K=2)


# ---- SMPLX_Deformer.k ----------------------------------------------------------------------------------------------------------------------
def check_deformer_k(dev, K=4):
    from deform.smplx_exavatar_deformer import SMPLX_Deformer
    from d3h import lbs as HL
    g, d, mk = _golden_deformer(dev, 1)
    md = {k[6:]: g[k] for k in g.files if k.startswith('model.')}
    md['posedirs'] = np.zeros((54 * 9, md['v_template'].shape[0] * 3), np.float32)
    d2 = SMPLX_Deformer(model_dict=md, device=dev, shape_param_dim=10, expr_param_dim=5, k=K)          # constructor argument ...
    assert d2.k == K and d.k == 1
    d2.vs_template, d2.init_A = d.vs_template, d.init_A
    pts = T(g['pts'], dev)
    out1 = d.lbs_forward_batch(pts, mk(), range(3))
    d.k = K                                                                                            # ... and the reference idiom
    nn = d.nearest(pts)
    assert isinstance(nn, HL.KnnResult) and tuple(nn.idx.shape) == (pts.shape[0], K)
    idx, dist = nn
    assert idx is nn.idx and dist is nn.d2 and tuple(nn[:7].idx.shape) == (7, K)
    out_a, out_b = d.lbs_forward_batch(pts, mk(), range(3)), d2.lbs_forward_batch(pts, mk(), range(3))
    assert torch.equal(out_a, out_b) and not torch.equal(out_a, out1)
    for f in range(3):
        # (not bit for bit: the joint transforms of one frame and of a batch of three come from differently shaped torch products; the
        # project's bar on posed points, parity_cases.check_lbs_golden)
        assert float((d.lbs_forward(pts.reshape(1, -1, 3), mk(), idx=f).detach() - out_a[f].detach()).abs().max()) < 5e-6, f
    # interpolate_weights: rows non-negative, summing to 1 within the rounding of a 55-term float32 sum (plus the K-term blend)
    p = pts.clone().requires_grad_(True)
    w = d.interpolate_weights(p[None])
    assert tuple(w.shape) == (1, pts.shape[0], 55) and bool((w >= 0).all())
    assert float((w.sum(-1) - 1).abs().max()) <= 64 * 2.0 ** -23
    w[0, :, 3].sum().backward()
    assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    can = d.lbs_forward_inverse(pts[None])
    assert tuple(can.shape) == (1, pts.shape[0], 3) and bool(torch.isfinite(can).all())
    # the launch-ahead pair at a capacity, rows counted on the device, adopted through pre=: bit for bit the plain order
    P = pts.shape[0]
    cap = P + 37
    buf = torch.cat([pts, torch.full((37, 3), float('nan'), device=dev)]).contiguous()
    counts = torch.zeros(16, dtype=torch.int32)
    counts[0], counts[1], counts[2] = P - 3 * 20 - 4 * 10, 20, 10
    counts = counts.to(dev)
    param = mk()
    tr = d.frame_transforms(param, range(3))
    nn_cap = d.nearest_counted(buf, counts)
    flat = d.lbs_forward_counted(buf, counts, nn_cap, tr)
    pre = HL.counted_result(flat, 3, P)
    p2 = pts.clone().requires_grad_(True)
    ahead = d.lbs_forward_batch(p2, param, range(3), nn_idx=nn_cap[:P], transforms=tr, pre=pre)
    assert ahead.data_ptr() == pre.data_ptr()
    p3 = pts.clone().requires_grad_(True)
    plain = d.lbs_forward_batch(p3, mk(), range(3))
    assert torch.equal(ahead, plain) and torch.equal(nn_cap[:P].idx, nn.idx) and torch.equal(nn_cap[:P].d2, nn.d2)
    gout = T(g['gout'], dev)
    (ahead * gout).sum().backward(); (plain * gout).sum().backward()
    assert torch.equal(p2.grad, p3.grad)
    for bad in (0, 33, 2.5):
        d.k = bad
        try:
            d.nearest(pts)
        except ValueError:
            continue
        raise AssertionError(f'k = {bad!r} was accepted')


def check_launch_ahead_k(dev, monkeypatch, K=4, **kw):
    """tests/e2e_cases.check_launch_ahead, unchanged, on a scene whose deformer has k = K: the tick whose nearest-K search and K-blended LBS
    were queued before the host knew the sizes equals the plain order; the K kernels were really the ones launched ahead"""
    import e2e_cases as E
    from d3h import scene, lbs as HL
    made, calls = [], {'counted': 0, 'plain': 0}

    class SceneK(scene.Scene):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.geometry.smplx_deform.k = K
            made.append(self)
    counted, plain = HL.lbs_points_k_counted, HL.lbs_points_k
    monkeypatch.setattr(scene, 'Scene', SceneK)
    monkeypatch.setattr(HL, 'lbs_points_k_counted', lambda *a, **k: (calls.__setitem__('counted', calls['counted'] + 1), counted(*a, **k))[1])
    monkeypatch.setattr(HL, 'lbs_points_k', lambda *a, **k: (calls.__setitem__('plain', calls['plain'] + 1), plain(*a, **k))[1])
    E.check_launch_ahead(dev, **kw)
    assert len(made) == 1 and made[0].geometry.smplx_deform.k == K
    assert calls['counted'] >= kw.get('ticks', 4) - 1 and calls['plain'] >= 2 * kw.get('ticks', 4), calls


def check_tick_init_k(dev, K=4, res=128, grid_n=12, body_verts=2048):
    """one tick_init step of the synthetic scene with k = K: every loss and gradient finite, and not the k = 1 step"""
    from d3h.scene import Scene
    ell = lambda x: (((x - torch.tensor([0.0, -0.4, 0.0], device=x.device)) / torch.tensor([0.55, 0.8, 0.45], device=x.device)).norm(dim=-1) - 1.0) * 0.4
    torch.manual_seed(0)
    sc = Scene(res=res, grid_n=grid_n, n_frames=2, device=dev, prefit_steps=150, loss_set='full', body_verts=body_verts, sdf_fn=ell)
    bg = torch.rand(2, res, res, 3, device=dev)
    g = sc.geometry

    def tick(k):
        g.smplx_deform.k = k
        torch.manual_seed(7)
        sc._zero_grad()
        r = g.tick_init(sc.glctx, sc.target(bg), None, sc.material, sc.loss_fn, 5, None)
        (r['d3h_total'] if 'd3h_total' in r else (r['msk_loss'] + r['reg_loss'] + r['normal_loss'])).backward()
        losses = {n: float(v.detach()) for n, v in r.items() if torch.is_tensor(v) and v.numel() == 1}
        grads = [p.grad.clone() for p in [g.deform, sc.FLAGS.trans_optim] + list(g.sdf_net.parameters()) if p.grad is not None]
        return losses, grads, g.last_mesh_dict['deform_imesh'].v_pos.detach().clone()
    l1, g1, v1 = tick(1)
    lk, gk, vk = tick(K)
    assert all(np.isfinite(v) for v in lk.values()), lk
    assert len(gk) >= 10 and all(bool(torch.isfinite(t).all()) for t in gk)
    assert v1.shape == vk.shape and not torch.equal(v1, vk), 'the posed mesh of the k step equals the k = 1 one: the feature was not reached'
    assert not torch.equal(g1[0], gk[0]) and float(gk[0].abs().max()) > 0
