"""Differentiable pixel derivatives (rasterize grad_db, interpolate out_da) on the host emulation of csrc/raster.hip, against a float64 torch
restatement of the contract in the docstring of d3human-code_amd/d3h/raster.py.  The restatement (`ref_*` below) is the oracle of this file
and of test_gpu_raster_db_grad.py; its own gradients are checked with torch.autograd.gradcheck.  It is evaluated at the kernel's own
winning triangle ids: the visibility decision carries no gradient and is not what these tests are about."""
import pytest
import torch

import test_texture_modes as TM

f64 = torch.float64

# ---- the restatement ------------------------------------------------------------------------------------------------------------------


def _bidx(nsrc, ids):
    B = ids.shape[0]
    return (torch.arange(B, device=ids.device)[:, None, None] * (1 if nsrc > 1 else 0)).expand(ids.shape)


def ref_rasterize(pos, tri, ids, H, W):
    """(u, v, db) at winning ids [B,H,W] (id + 1, 0 = empty) as functions of pos [B or 1, V, 4]: u, v [B,H,W], db [B,H,W,4] =
    (du/dX, du/dY, dv/dX, dv/dY) in pixel units -- the formulas of oracle/raster.py:rasterize, without its detach"""
    dev = pos.device
    ys, xs = torch.meshgrid(torch.arange(H, dtype=f64, device=dev), torch.arange(W, dtype=f64, device=dev), indexing='ij')
    fx, fy = (xs + 0.5) * (2.0 / W) - 1.0, (ys + 0.5) * (2.0 / H) - 1.0
    cov = ids > 0
    f = (ids - 1).clamp(min=0)
    P = pos[_bidx(pos.shape[0], ids)[..., None], tri[f]]            # [B,H,W,3,4]
    q = 1.0 / P[..., 3]
    X, Y = P[..., 0] * q, P[..., 1] * q
    dx, dy = X - fx[..., None], Y - fy[..., None]
    a = torch.stack([dx[..., 1] * dy[..., 2] - dy[..., 1] * dx[..., 2],
                     dx[..., 2] * dy[..., 0] - dy[..., 2] * dx[..., 0],
                     dx[..., 0] * dy[..., 1] - dy[..., 0] * dx[..., 1]], -1)
    n = a * q
    S = torch.where(cov, n.sum(-1), torch.ones_like(q[..., 0]))     # (empty pixels: a placeholder that keeps 0/0 out of the gradient)
    u, v = n[..., 0] / S, n[..., 1] / S
    dnx = torch.stack([Y[..., 1] - Y[..., 2], Y[..., 2] - Y[..., 0], Y[..., 0] - Y[..., 1]], -1) * q
    dny = torch.stack([X[..., 2] - X[..., 1], X[..., 0] - X[..., 2], X[..., 1] - X[..., 0]], -1) * q
    dSx, dSy = dnx.sum(-1), dny.sum(-1)
    sx, sy = 2.0 / W, 2.0 / H
    db = torch.stack([(dnx[..., 0] - u * dSx) / S * sx, (dny[..., 0] - u * dSy) / S * sy,
                      (dnx[..., 1] - v * dSx) / S * sx, (dny[..., 1] - v * dSy) / S * sy], -1)
    z = torch.zeros_like(u)
    return torch.where(cov, u, z), torch.where(cov, v, z), torch.where(cov[..., None], db, torch.zeros_like(db))


def ref_interpolate(attr, u, v, ids, tri, db, diff_attrs='all'):
    """(out [B,H,W,A], out_da [B,H,W,2 len(diff_attrs)]): per listed channel c, in list order, (db.x e0 + db.z e1, db.y e0 + db.w e1)"""
    B, H, W = ids.shape
    cov = ids > 0
    f = (ids - 1).clamp(min=0)
    a = attr[_bidx(attr.shape[0], ids)[..., None], tri[f]]          # [B,H,W,3,A]
    out = u[..., None] * a[..., 0, :] + v[..., None] * a[..., 1, :] + (1 - u - v)[..., None] * a[..., 2, :]
    out = torch.where(cov[..., None], out, torch.zeros_like(out))
    if db is None:
        return out, None
    idx = list(range(attr.shape[-1])) if diff_attrs == 'all' else list(diff_attrs)
    e0, e1 = (a[..., 0, :] - a[..., 2, :])[..., idx], (a[..., 1, :] - a[..., 2, :])[..., idx]
    dX = db[..., 0:1] * e0 + db[..., 2:3] * e1
    dY = db[..., 1:2] * e0 + db[..., 3:4] * e1
    da = torch.stack([dX, dY], -1).reshape(B, H, W, -1)
    return out, torch.where(cov[..., None], da, torch.zeros_like(da))


# ---- cases ----------------------------------------------------------------------------------------------------------------------------


def random_mesh(gen, nf, B=1, spread=0.9, size=0.35, w_lo=1.0, w_hi=3.0):
    """nf small random triangles in NDC, lifted to clip space with random w; both windings occur"""
    cen = (torch.rand(B, nf, 1, 2, generator=gen, dtype=f64) * 2 - 1) * spread
    xy = (cen + (torch.rand(B, nf, 3, 2, generator=gen, dtype=f64) * 2 - 1) * size).reshape(B, nf * 3, 2)
    z = torch.rand(B, nf * 3, 1, generator=gen, dtype=f64) * 1.6 - 0.8
    w = torch.rand(B, nf * 3, 1, generator=gen, dtype=f64) * (w_hi - w_lo) + w_lo
    pos = torch.cat([xy * w, z * w, w], -1)
    tri = torch.arange(nf * 3, dtype=torch.int32).reshape(nf, 3)
    return pos.float(), tri


def crossing_mesh():
    """two triangles: one crosses the camera plane (a vertex behind it: the homogeneous-edge path), one in front"""
    pos = torch.tensor([[[-0.6, -0.5, 0.2, 1.0], [0.7, -0.4, 0.1, 1.2], [0.3, 0.5, 0.5, -0.7],
                         [-0.8, 0.2, 0.3, 1.5], [-0.1, 0.9, 0.4, 1.1], [-0.9, 0.9, 0.2, 1.3]]], dtype=torch.float32)
    return pos, torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32)


def tiny_mesh():
    """a quad of two triangles whose corners sit on pixel corners of an 8 x 6 image (pixel-exact coverage), opposite windings"""
    X = lambda px: px * (2.0 / 8) - 1.0
    Y = lambda py: py * (2.0 / 6) - 1.0
    pts = [(X(1), Y(1), 0.1, 1.0), (X(7), Y(1), 0.2, 2.0), (X(1), Y(5), 0.3, 1.5), (X(7), Y(5), 0.1, 1.2)]
    pos = torch.tensor([[[x * w, y * w, z * w, w] for x, y, z, w in pts]], dtype=torch.float32)
    return pos, torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)


def rast_grads(dev, pos, tri, H, W, nb, G1, G2, use_rast=True):
    """kernel d_pos of  sum G1 rast[..., :2] + sum G2 db  (use_rast False: the db term alone), with the rast / db it rendered"""
    from d3h import raster
    p = pos.to(dev).requires_grad_(True)
    rast, db = raster.rasterize(p, tri.to(dev), (H, W), nb=nb, grad_db=True)
    loss = (db * G2.float().to(dev)).sum()
    if use_rast:
        loss = loss + (rast[..., :2] * G1.float().to(dev)).sum()
    g, = torch.autograd.grad(loss, p)
    return g, rast.detach(), db.detach()


def ref_rast_grads(pos, tri, ids, H, W, G1, G2, use_rast=True):
    pd = pos.double().to(ids.device).requires_grad_(True)
    u, v, db = ref_rasterize(pd, tri.long().to(ids.device), ids, H, W)
    loss = (db * G2.to(ids.device)).sum()
    if use_rast:
        loss = loss + (torch.stack([u, v], -1) * G1.to(ids.device)).sum()
    g, = torch.autograd.grad(loss, pd)
    return g, db.detach()


def check_raster(dev, pos, tri, H, W, nb=None, gen=None, rtol=2e-4, bad_frac=0.0, min_cov=1):
    nb = pos.shape[0] if nb is None else nb
    G1 = torch.randn(nb, H, W, 2, generator=gen, dtype=f64)
    G2 = torch.randn(nb, H, W, 4, generator=gen, dtype=f64)
    for use_rast in (True, False):
        g, rast, db = rast_grads(dev, pos, tri, H, W, nb, G1, G2, use_rast)
        ids = rast[..., 3].long()
        assert int((ids > 0).sum()) >= min_cov
        gr, dbr = ref_rast_grads(pos, tri, ids, H, W, G1, G2, use_rast)
        TM.close(db, dbr, rtol, 'db', bad_frac)
        TM.close(g, gr, rtol, f'd_pos ({"rast + db" if use_rast else "db alone"})', bad_frac)
        assert float(g.abs().max()) > 0
    return rast, db


# ---- the restatement's own gradients --------------------------------------------------------------------------------------------------


def test_restatement_gradcheck():
    pos, tri = tiny_mesh()
    pos2, tri2 = crossing_mesh()
    for p, t, (H, W) in ((pos, tri, (6, 8)), (pos2, tri2, (5, 7))):
        from oracle import raster as OR
        ids = torch.from_numpy(OR.rasterize_ids(p.numpy(), t.numpy(), H, W))
        assert int((ids > 0).sum()) > 3
        pd = p.double().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda x: ref_rasterize(x, t.long(), ids, H, W), (pd,), eps=1e-7, atol=1e-5)
    gen = torch.Generator().manual_seed(0)
    attr = torch.randn(1, 4, 5, generator=gen, dtype=f64).requires_grad_(True)
    u, v, db = (t.detach().requires_grad_(True) for t in ref_rasterize(pos.double(), tri.long(), ids_tiny(), 6, 8))
    for da in ('all', [2, 0], [4, 4, 1]):
        f = lambda a, uu, vv, d: ref_interpolate(a, uu, vv, ids_tiny(), tri.long(), d, da)
        assert torch.autograd.gradcheck(f, (attr, u, v, db), eps=1e-7, atol=1e-5)


def ids_tiny():
    from oracle import raster as OR
    pos, tri = tiny_mesh()
    return torch.from_numpy(OR.rasterize_ids(pos.numpy(), tri.numpy(), 6, 8))


# ---- kernel vs restatement (host emulation) --------------------------------------------------------------------------------------------


def test_raster_tiny_pixel_exact(emul):
    """the pixel-exact quad: ids equal the oracle's, every pixel of the 6 x 4 interior covered, db and d_pos as the restatement"""
    gen = torch.Generator().manual_seed(1)
    pos, tri = tiny_mesh()
    rast, _ = check_raster(emul, pos, tri, 6, 8, gen=gen, min_cov=24)
    assert torch.equal(rast[0, ..., 3].long(), ids_tiny()[0])
    # the quad's two windings: reversed triangles give the same coverage and the same gradients
    check_raster(emul, pos, tri[:, [0, 2, 1]].contiguous(), 6, 8, gen=gen, min_cov=24)


def test_raster_near_plane_crossing(emul):
    gen = torch.Generator().manual_seed(2)
    pos, tri = crossing_mesh()
    rast, _ = check_raster(emul, pos, tri, 24, 28, gen=gen, min_cov=20)
    assert int((rast[..., 3] == 1).sum()) > 10, 'the crossing triangle wins no pixel'


def test_raster_random_batched_and_broadcast(emul):
    gen = torch.Generator().manual_seed(3)
    pos, tri = random_mesh(gen, 300, B=2)
    check_raster(emul, pos, tri, 40, 48, gen=gen, min_cov=800)
    check_raster(emul, pos[:1].contiguous(), tri, 40, 48, nb=2, gen=gen, min_cov=800)          # one mesh broadcast over two frames


def test_raster_db_only_through_db(emul):
    """a loss of db alone reaches pos (on the current tree the db output is not differentiable: autograd.grad raises)"""
    from d3h import raster
    pos, tri = tiny_mesh()
    p = pos.requires_grad_(True)
    _, db = raster.rasterize(p, tri, (6, 8), grad_db=True)
    assert db.requires_grad
    g, = torch.autograd.grad(db.square().sum(), p)
    assert float(g.abs().max()) > 0


def _interp_case(gen, B, A, H, W, bcast):
    from d3h import raster
    pos, tri = random_mesh(gen, 60, B=B, size=0.5)
    rast, db = raster.rasterize(pos, tri, (H, W))
    nv = pos.shape[1]
    attr = torch.randn(1 if bcast else B, nv, A, generator=gen, dtype=f64)
    return rast, db, tri, attr


def check_interp(dev, rast, db, tri, attr, diff_attrs, G_out, G_da, rtol=1e-5):
    """kernel d_attr, d_rast, d_rast_db of  sum G_out out + sum G_da out_da  against the restatement; G_out / G_da None: that term absent"""
    from d3h import raster
    a = attr.detach().float().to(dev).requires_grad_(True)
    r = rast.detach().to(dev).requires_grad_(True)
    d = db.detach().to(dev).requires_grad_(True)
    out, da = raster.interpolate(a, r, tri.to(dev), rast_db=d, diff_attrs=diff_attrs)
    ids = rast[..., 3].detach().long()
    ad, ud, vd, dd = (t.detach().double().requires_grad_(True) for t in (attr.float(), rast[..., 0], rast[..., 1], db))
    ro, rda = ref_interpolate(ad, ud, vd, ids, tri.long(), dd, diff_attrs)
    TM.close(out, ro, rtol, 'out')
    TM.close(da, rda, rtol, 'out_da')
    loss, rloss = 0.0, 0.0
    if G_out is not None:
        loss, rloss = loss + (out * G_out.float()).sum(), rloss + (ro * G_out).sum()
    if G_da is not None:
        loss, rloss = loss + (da * G_da.float()).sum(), rloss + (rda * G_da).sum()
    g = torch.autograd.grad(loss, (a, r, d), allow_unused=True)
    gr = torch.autograd.grad(rloss, (ad, ud, vd, dd), allow_unused=True)
    z = lambda t, like: torch.zeros_like(like) if t is None else t
    TM.close(z(g[0], a), z(gr[0], ad), rtol, 'd_attr')
    TM.close(z(g[1], r)[..., 0], z(gr[1], ud), rtol, 'd_rast u')
    TM.close(z(g[1], r)[..., 1], z(gr[2], vd), rtol, 'd_rast v')
    assert g[1] is None or float(g[1][..., 2:].abs().max()) == 0
    TM.close(z(g[2], d), z(gr[3], dd), rtol, 'd_rast_db')
    return g


@pytest.mark.parametrize('diff_attrs', ['all', [2, 0], [4, 1, 1]])
@pytest.mark.parametrize('bcast', [False, True])
def test_interpolate_da_grads(emul, diff_attrs, bcast):
    gen = torch.Generator().manual_seed(4 + bcast)
    B, A, H, W = 2, 5, 24, 32
    rast, db, tri, attr = _interp_case(gen, B, A, H, W, bcast)
    nd = 2 * (A if diff_attrs == 'all' else len(diff_attrs))
    G_out = torch.randn(B, H, W, A, generator=gen, dtype=f64)
    G_da = torch.randn(B, H, W, nd, generator=gen, dtype=f64)
    g = check_interp(emul, rast, db, tri, attr, diff_attrs, G_out, G_da)             # both
    assert float(g[2].abs().max()) > 0 and float(g[0].abs().max()) > 0
    g = check_interp(emul, rast, db, tri, attr, diff_attrs, None, G_da)               # out_da alone
    assert float(g[1].abs().max()) == 0, 'out_da does not depend on (u, v)'
    check_interp(emul, rast, db, tri, attr, diff_attrs, G_out, None)                  # out alone: the existing backward


def test_interpolate_per_face_index_buffer(emul):
    """an index buffer of its own (a uv chart's t_tex_idx: other vertices, other count) with a list of channels"""
    gen = torch.Generator().manual_seed(6)
    B, H, W = 2, 20, 28
    rast, db, tri, _ = _interp_case(gen, B, 3, H, W, False)
    tri2 = torch.randint(0, 17, tri.shape, generator=gen, dtype=torch.int32)
    attr = torch.randn(1, 17, 3, generator=gen, dtype=f64)
    G_out = torch.randn(B, H, W, 3, generator=gen, dtype=f64)
    G_da = torch.randn(B, H, W, 4, generator=gen, dtype=f64)
    check_interp(emul, rast, db, tri2, attr, [1, 2], G_out, G_da)
    check_interp(emul, rast, db, tri2, attr, 'all', None, torch.randn(B, H, W, 6, generator=gen, dtype=f64))


def test_interpolate_list_forward_matches_all(emul):
    """a list picks the 'all' output's channel pairs, in list order, bit for bit; the out image is unchanged"""
    from d3h import raster
    gen = torch.Generator().manual_seed(7)
    rast, db, tri, attr = _interp_case(gen, 2, 5, 16, 16, False)
    a = attr.float()
    o_all, d_all = raster.interpolate(a, rast, tri, rast_db=db, diff_attrs='all')
    o_l, d_l = raster.interpolate(a, rast, tri, rast_db=db, diff_attrs=[2, 0])
    assert d_l.shape[-1] == 4 and d_all.shape[-1] == 10
    assert torch.equal(o_all, o_l)
    assert torch.equal(d_l, d_all[..., [4, 5, 0, 1]])
    o_n, d_n = raster.interpolate(a, rast, tri)
    assert d_n is None and torch.equal(o_n, o_all)
    with pytest.raises(ValueError, match='out of range'):
        raster.interpolate(a, rast, tri, rast_db=db, diff_attrs=[5])


# ---- end to end: rasterize -> interpolate -> mip-mapped texture ----------------------------------------------------------------------------


def receding_quad(dev, wf=400.0):
    """a floor receding to the horizon (as test_gpu_texture_modes.py:test_gpu_texture2d_flow): footprints from ~1 texel to the whole texture"""
    pos = torch.tensor([[-0.9, -0.9, 0.5, 1.0], [0.9, -0.9, 0.5, 1.0], [-0.9 * wf, 0.99 * wf, 0.9 * wf, wf], [0.9 * wf, 0.99 * wf, 0.9 * wf, wf]],
                       device=dev)[None]
    tri = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32, device=dev)
    uv_attr = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], device=dev)
    return pos, tri, uv_attr


def check_chain(dev, pos, tri, uv_attr, tex, res, gen, rtol, bad_frac=0.0, grtol=None, tex_grtol=None):
    """d pos, d uv_attr, d tex of  sum G texture(interpolate(rasterize))  against the restatement chain at the kernel's ids (grtol: the bar of
    d pos and d uv_attr, sums over every pixel; rtol and bad_frac hold for the output and d tex)"""
    import nvdiffrast.torch as dr
    p = pos.clone().requires_grad_(True)
    ua = uv_attr.clone().requires_grad_(True)
    tk = tex.float().to(dev).requires_grad_(True)
    rast, db = dr.rasterize(None, p, tri, res)
    uv, uv_da = dr.interpolate(ua, rast, tri, rast_db=db, diff_attrs='all')
    out = dr.texture(tk, uv, uv_da, filter_mode='linear-mipmap-linear', boundary_mode='wrap')
    G = torch.randn(out.shape, generator=gen, dtype=f64)
    g = torch.autograd.grad((out * G.float().to(dev)).sum(), (p, ua, tk))
    ids = rast[..., 3].detach().long()
    pd, ud, td = pos.double().requires_grad_(True), uv_attr.double().requires_grad_(True), tex.double().to(dev).requires_grad_(True)
    u, v, dbr = ref_rasterize(pd, tri.long(), ids, *res)
    uvr, uvr_da = ref_interpolate(ud[None], u, v, ids, tri.long(), dbr, 'all')
    ref = TM.ref_texture(td, uvr, uvr_da, filter_mode='linear-mipmap-linear', boundary_mode='wrap')
    TM.close(out, ref, rtol, 'texture output', bad_frac)
    gr = torch.autograd.grad((ref * G.to(dev)).sum(), (pd, ud, td))
    for name, a, b in zip(('d_pos', 'd_uv_attr'), g, gr):
        TM.close(a, b, rtol if grtol is None else grtol, name)
    TM.close(g[2], gr[2], rtol if tex_grtol is None else tex_grtol, 'd_tex', bad_frac)
    return g


def test_texture_chain(emul):
    gen = torch.Generator().manual_seed(8)
    pos, tri, uv_attr = receding_quad(emul)
    tex = torch.rand(1, 32, 32, 3, generator=gen, dtype=f64)
    g = check_chain(emul, pos, tri, uv_attr, tex, (40, 40), gen, rtol=2e-3)
    assert float(g[0].abs().max()) > 0 and float(g[1].abs().max()) > 0


# ---- unchanged behaviour -------------------------------------------------------------------------------------------------------------


def test_grad_db_false_is_the_existing_path(emul):
    """grad_db False (d3h.raster's default, the shim's opt-out, the product's DepthPeeler): db comes back detached and d_pos is bit for bit
    the barycentric-only gradient -- also with grad_db True when nothing differentiates db"""
    import nvdiffrast.torch as dr
    from d3h import raster
    gen = torch.Generator().manual_seed(9)
    pos, tri = random_mesh(gen, 120, B=2)
    G1 = torch.randn(2, 32, 32, 4, generator=gen).float()
    grads = []
    for how in ('raster', 'shim', 'peeler', 'grad_db_unused'):
        p = pos.clone().requires_grad_(True)
        if how == 'raster':
            rast, db = raster.rasterize(p, tri, (32, 32))
        elif how == 'shim':
            rast, db = dr.rasterize(None, p, tri, (32, 32), grad_db=False)
        elif how == 'peeler':
            with dr.DepthPeeler(None, p, tri, (32, 32), grad_db=False) as peeler:
                rast, db = peeler.rasterize_next_layer()
        else:
            rast, db = raster.rasterize(p, tri, (32, 32), grad_db=True)
        assert db.shape == rast.shape and db.requires_grad == (how == 'grad_db_unused')
        loss = (rast * G1).sum() + (db.detach() * 2).sum()
        grads.append(torch.autograd.grad(loss, p)[0])
    assert all(torch.equal(grads[0], g) for g in grads[1:])
    # the shim's default is nvdiffrast's: grad_db True
    _, db = dr.rasterize(None, pos.clone().requires_grad_(True), tri, (32, 32))
    assert db.requires_grad


class _Counting:
    """a library handle that counts the calls of some entry points"""

    def __init__(self, lib, names):
        self._l, self.calls = lib, {n: 0 for n in names}

    def __getattr__(self, name):
        fn = getattr(self._l, name)
        if name not in self.calls:
            return fn

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


def test_tick_init_never_calls_the_new_entry_points(emul):
    """one emulated tick_init of the small scene (test_e2e_emul.py's size), forward and backward: the product's graph does not reach the
    pixel-derivative gradients"""
    import e2e_cases as E
    from d3h import _lib as L
    names = ('d3h_rasterize_bwd_db', 'd3h_interpolate_fwd_da', 'd3h_interpolate_bwd_da', 'd3h_rasterize_bwd', 'd3h_gbuffer_raster_bwd',
             'd3h_rasterize_fwd')
    cnt = _Counting(L.lib(), names)
    L._lib = cnt
    st = E.make_state(n=6, res=32, frames=2, n_samples=96)
    P = E.build_product(emul, st, 12, ('shaded', 'geometric_normal', 'msdf_image'))
    r, total = E.product_tick(P, st, emul)
    total.backward()
    assert cnt.calls['d3h_rasterize_fwd'] > 0 and cnt.calls['d3h_rasterize_bwd'] + cnt.calls['d3h_gbuffer_raster_bwd'] > 0, cnt.calls
    assert cnt.calls['d3h_rasterize_bwd_db'] == cnt.calls['d3h_interpolate_fwd_da'] == cnt.calls['d3h_interpolate_bwd_da'] == 0, cnt.calls
