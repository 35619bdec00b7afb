"""FLAGS.tet_smpl: the body tet mesh, `sdf_tet_gt`, `all_edges_smpl` and the `smpl_msdf` parameter that HmSDFTetsGeometry builds at start-up
(geometry/hmsdf.py:239-249,391-397 of the reference), the optimisers and the checkpoint -- on a synthetic SMPL-X model dict whose template is a
closed mesh.  Used by tests/test_tetfill_emul.py and tests/test_gpu_tetfill.py."""
import os

import numpy as np
import pytest
import torch

from d3h import synth

import tetfill_cases as TC

ELL = lambda x: (((x - torch.tensor([0.0, -0.4, 0.0], device=x.device)) / torch.tensor([0.55, 0.8, 0.45], device=x.device)).norm(dim=-1) - 1.0) * 0.4


def body_model(faces=True):
    """synth.make_body_model with a closed template: an ellipsoid of 258 vertices (the skinning fields keep their shapes)"""
    d = synth.make_body_model(n_verts=258, seed=0)
    v, f = synth.icosphere(3)
    d['v_template'] = (v * np.array([0.33, 0.6, 0.28], np.float32) + np.array([0.0, -0.35, 0.0], np.float32)).astype(np.float32)
    if faces:
        d['f'] = f
    return d


def scene(dev, tet_smpl=None, faces=True, out_dir=None, seed=0):
    """a tiny init-stage scene whose SDF network is the CPU-fitted golden state (no pre-fit: nothing in its construction depends on the order of
    float atomics); tet_smpl None: the flag is absent"""
    from d3h.scene import Scene
    from conftest import GOLD

    def hook(F):
        F.prefit_with_library_path, F.eikonal_samples = True, 96
        F.smplx_model_dict = body_model(faces)
        F.out_dir = out_dir
        if tet_smpl is not None:
            F.tet_smpl, F.tet_smpl_res = tet_smpl, 8
    torch.manual_seed(seed)
    return Scene(res=32, grid_n=6, n_frames=1, device=dev, seed=seed, prefit_steps=0, loss_set='mask', body_verts=258, sdf_fn=ELL, flags_hook=hook,
                 sdf_state=os.path.join(GOLD, 'parity_state_sdf.npz'))


def tick(sc, it=0, seed=11):
    """one tick_init under a fixed seed, with its backward -> (losses, gradients by parameter name)"""
    torch.manual_seed(seed)
    bg = torch.zeros(1, sc.res, sc.res, 3, device=sc.device)
    sc._zero_grad()
    r = sc.geometry.tick_init(sc.glctx, sc.target(bg), None, sc.material, sc.loss_fn, it, None)
    (r['d3h_total'] if 'd3h_total' in r else (r['msk_loss'] + r['reg_loss'])).backward()
    if sc.device.type == 'cuda':
        torch.cuda.synchronize()
    losses = {k: v.detach().clone() for k, v in r.items() if torch.is_tensor(v) and v.numel() == 1}
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in sc.geometry.named_parameters()}
    return losses, grads


def check_startup_attributes(dev, tmp_path):
    from d3h import meshops, tetfill
    sc = scene(dev, True, out_dir=str(tmp_path))
    g = sc.geometry
    template = g.smplx_deform.vs_template[0].detach().float().contiguous()
    faces = torch.as_tensor(body_model()['f'], device=g.device)
    v, t, h = tetfill.fill_mesh(template, faces, res=8, scale=1.1)
    n = v.shape[0]
    assert n > 0 and t.shape[0] > 0
    assert torch.equal(g.tet_smpl_v, v) and g.tet_smpl_v.dtype == torch.float32
    assert torch.equal(g.tet_smpl_f, t) and g.tet_smpl_f.dtype == torch.int64
    assert g.sdf_tet_gt.shape == (n, 1) and torch.equal(g.sdf_tet_gt, meshops.mesh_sdf(v, template, faces).reshape(-1, 1))
    e = torch.sort(t[:, [0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3]].reshape(-1, 2), dim=1)[0]
    assert torch.equal(g.all_edges_smpl, torch.unique(e, dim=0)) and g.all_edges_smpl.dtype == torch.int64
    assert g.max_displacement_smpl == g.max_displacement
    sd = g.state_dict()
    assert 'smpl_msdf' in sd and sd['smpl_msdf'].shape == (n,) and float(sd['smpl_msdf'].min()) >= -1 and float(sd['smpl_msdf'].max()) <= 1
    assert isinstance(g.smpl_msdf, torch.nn.Parameter) and g.smpl_msdf.requires_grad and len(torch.unique(g.smpl_msdf)) > n // 2
    assert not any(k.startswith(('tet_smpl', 'sdf_tet', 'all_edges')) for k in sd)
    z = np.load(os.path.join(str(tmp_path), 'smpl_template_tet_{}.npz'.format(g.grid_res)))
    assert sorted(z.files) == ['f', 'v'] and np.array_equal(z['v'], v.cpu().numpy()) and np.array_equal(z['f'], t.cpu().numpy())
    side = float((template.max(0).values - template.min(0).values).max()) * 1.1
    TC.check_geometry(v.cpu().numpy(), t.cpu().numpy(), float(template.abs().max()) + side, h, 2)
    with pytest.raises(RuntimeError, match='body model with faces'):
        scene(dev, True, faces=False)


def check_step_leaves_smpl_msdf(dev, fused):
    """a tick and a step under the init-stage and under the split-stage groups (where 'msdf' in name puts the parameter into a group), and under a
    gradient arena that enumerates it: never a gradient, never a change"""
    from d3h import scene as S
    keep = S.FUSED_OPTIMIZER
    S.FUSED_OPTIMIZER = fused
    try:
        sc = scene(dev, True)
        g = sc.geometry
        assert (sc.opt is not None) == fused
        want = g.smpl_msdf.detach().clone()
        groups = lambda: [p for grp in sc.opt_geo.param_groups for p in grp['params']]
        for stage, arena in (('init', False), ('split', False), ('split', True)):
            sc._build_optimizers(stage, 300)
            assert any(p is g.smpl_msdf for p in groups()) == (stage == 'split')
            _, grads = tick(sc)
            assert grads['smpl_msdf'] is None and grads['deform'] is not None
            if arena:
                sc._arena = None
                a = sc._grad_arena()
                assert any(p is g.smpl_msdf for p in a.params)
                a.collect()
                assert g.smpl_msdf.grad is not None and not bool(g.smpl_msdf.grad.any())
            sc._optimizer_step()
            assert torch.equal(g.smpl_msdf.detach(), want)
    finally:
        S.FUSED_OPTIMIZER = keep


def _close(x, y):
    """the comparison of tests/test_gpu_data_edges.py's checkpoint round trip (float atomics: the sums are not bit-reproducible)"""
    return all(abs(float(x[k]) - float(y[k])) <= 1e-5 * max(1e-6, abs(float(y[k]))) for k in y)


def check_checkpoint(dev, tmp_path):
    """save_ckp -> load_ckp into a second geometry restores smpl_msdf exactly and reproduces the next tick; a file whose smpl_msdf has another
    length keeps the model's own"""
    from d3h import checkpoint as C
    a = scene(dev, True, seed=0)
    a.step()
    a.FLAGS.init_epoch = 2
    C.save_ckp(a.FLAGS, str(tmp_path / 'init'), 1, a.geometry, a.material)
    before, gbefore = tick(a, it=1)
    b = scene(dev, True, seed=5)
    assert not torch.equal(b.geometry.smpl_msdf, a.geometry.smpl_msdf)
    b.FLAGS.init_epoch = 2
    C.load_ckp(b.FLAGS, str(tmp_path), b.geometry, b.material, 'init')
    assert torch.equal(b.geometry.smpl_msdf, a.geometry.smpl_msdf)
    sa, sb = a.geometry.state_dict(), b.geometry.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    after, gafter = tick(b, it=1)
    assert _close(after, before), (after, before)
    for n in gbefore:
        assert (gbefore[n] is None) == (gafter[n] is None)
        if gbefore[n] is not None:
            assert float((gafter[n] - gbefore[n]).abs().max()) <= 1e-4 * max(1e-9, float(gbefore[n].abs().max())), n
    # another length: the shape filter keeps the model's own parameter
    path = str(tmp_path / 'init' / 'ckp' / 'model_1.pt')
    sd = torch.load(path, map_location=b.device)
    sd['smpl_msdf'] = torch.zeros(sd['smpl_msdf'].shape[0] + 3, device=b.device)
    sd['deform'] = sd['deform'] + 0.25
    torch.save(sd, path)
    own = b.geometry.smpl_msdf.detach().clone()
    C.load_ckp(b.FLAGS, str(tmp_path), b.geometry, b.material, 'init')
    assert torch.equal(b.geometry.smpl_msdf, own) and torch.equal(b.geometry.deform, sd['deform'])


def check_flag_absent(dev):
    """the flag absent and the flag False: no new attribute, the parent commit's state_dict keys, the same first tick bit for bit (the new code
    path is never entered: it is made to raise); and with the flag on, every other parameter steps as without it"""
    from geometry.hmsdf import HmSDFTetsGeometry
    real = HmSDFTetsGeometry._init_tet_smpl

    def never(self):
        raise AssertionError('_init_tet_smpl entered without FLAGS.tet_smpl')
    HmSDFTetsGeometry._init_tet_smpl = never
    try:
        a, b = scene(dev, None), scene(dev, False)
    finally:
        HmSDFTetsGeometry._init_tet_smpl = real
    keys = ['sdf', 'msdf', 'deform', 'cond', 'render_cond', 'fix_code'] + [f'sdf_net.net.{i}.{w}' for i in range(0, 16, 2) for w in ('weight', 'bias')]
    for sc in (a, b):
        g = sc.geometry
        assert sorted(g.state_dict().keys()) == sorted(keys)
        assert not any(hasattr(g, k) for k in ('smpl_msdf', 'tet_smpl_v', 'tet_smpl_f', 'sdf_tet_gt', 'all_edges_smpl', 'max_displacement_smpl'))
    sa, sb = a.geometry.state_dict(), b.geometry.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    la, la2, lb = tick(a)[0], tick(a)[0], tick(b)[0]
    assert la.keys() == lb.keys()
    if all(torch.equal(la[k], la2[k]) for k in la):         # the tick repeats itself bit for bit on this device: so must the other construction
        assert all(torch.equal(la[k], lb[k]) for k in la), (la, lb)
    else:                                                   # (sums formed by float atomics: not bit-reproducible even on one scene)
        assert _close(la, lb), (la, lb)
    # the flag on, the other parameters brought to the same state: one step moves them as without the flag
    c = scene(dev, True)
    c.geometry.load_state_dict(sa, strict=False)
    c.material['kd_ks'].load_state_dict(a.material['kd_ks'].state_dict())
    with torch.no_grad():
        c.FLAGS.trans_optim.copy_(a.FLAGS.trans_optim)
    names = lambda sc: [[n for n, q in sc.geometry.named_parameters() if any(q is p for p in grp['params'])] for grp in sc.opt_geo.param_groups]
    assert names(a) == names(c) and [grp['lr'] for grp in a.opt_geo.param_groups] == [grp['lr'] for grp in c.opt_geo.param_groups]
    if torch.device(dev).type != 'cpu':                     # (an Adam step divides by |g|: the order of the atomics decides where g is rounding noise)
        return
    for sc in (a, c):
        tick(sc)
        sc._optimizer_step()
    sc_, sa_ = c.geometry.state_dict(), a.geometry.state_dict()
    assert set(sc_) - set(sa_) == {'smpl_msdf'}
    assert all(torch.equal(sc_[k], sa_[k]) for k in sa_)
