"""Cases for the image-space backward tail: the texture position gradient written by the MLP half of the split backward
(csrc/texmlp.hip: texmlp_bwd_mlp_h2_kernel<true>) and the G-buffer / rasteriser backward that sums per workgroup in LDS
(csrc/raster.hip: gbuffer_bwd_tile_kernel).  Case functions take `dev`; tests/test_image_bwd_emul.py runs them on the host emulation,
tests/test_gpu_image_bwd.py on the GPU.  References: oracle/texmlp.py, oracle/raster.py; bars: those of check_texmlp / check_gbuffer /
check_texmlp_shared_table in tests/parity_cases.py."""
import contextlib
import os

import numpy as np
import torch

from parity_cases import T, _raster_scene

TEX_BAR = 2e-4          # check_texmlp: gradients against the oracle, of the reference maximum
TEX_SCALE_BAR = 2e-5    # check_texmlp: tiny upstream gradient; check_texmlp_shared_table: side stream on / off
GBUF_BAR = 1e-4         # check_gbuffer: d(attr), d(face), d(rast) against the oracle, of the reference maximum
FOLD_BAR = 2e-6         # check_gbuffer: folded d(pos) / d(attr) / d(face) against the separate path
WIDTHS = (3, 3, 3, 1)
TILES = ((16, 16), (32, 8), (64, 4), (8, 32), (32, 32))      # every tile shape the launcher knows (D3H_GBUF_TILE)


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def _tex_fused(on=True, async_grad=None):
    from d3h import texmlp
    was = texmlp.DX_FUSED, texmlp.ASYNC_TABLE_GRAD
    try:
        texmlp.DX_FUSED = on
        if async_grad is not None:
            texmlp.ASYNC_TABLE_GRAD = async_grad
        with _env(D3H_TEX_DX_FUSED='1' if on else '0', D3H_TEX_H2=None):
            yield
    finally:
        texmlp.DX_FUSED, texmlp.ASYNC_TABLE_GRAD = was


# ---- texture d_x ---------------------------------------------------------------------------------------------------------------------
BBOX = (0.6, 0.6, 0.2, -0.8, -1.2, -0.2)
OMIN, OMAX = (0, 0, 0, 0, 0.001, 0), (1, 1, 1, 0, 1, 1)
_TEX = {}


def _tex_inputs(n):
    """the point set of check_texmlp (same seed, same edits), and the oracle's gradients for it -- computed once per n"""
    if n in _TEX:
        return _TEX[n]
    from d3h import texmlp
    from oracle import texmlp as OT
    gen = torch.Generator().manual_seed(31)
    npar = texmlp.grid_param_count()
    table = (torch.rand(npar, generator=gen) * 2 - 1) * 0.5
    w1 = torch.randn(32, 10, generator=gen) * 0.5
    w2 = torch.randn(32, 32, generator=gen) * 0.3
    w3 = torch.randn(6, 32, generator=gen) * 0.3
    x = torch.rand(n, 3, generator=gen) * torch.tensor([1.8, 2.2, 0.6]) + torch.tensor([-1.0, -1.4, -0.3])   # partly outside the box
    x[0] = torch.tensor([-0.8, -1.2, -0.2])                                     # exactly on the x_n == 1 corner (level-0 wrap)
    mask = (torch.rand(n, generator=gen) > 0.2).float()
    if n >= 400:
        mask[128:352] = 0        # three background waves in a row, then a wave whose first 32-pixel MFMA chain is all background
    mask[0] = 1
    G = torch.randn(n, 6, generator=gen)
    if n >= 200:
        G[40:136] = 0.0          # covered pixels without an upstream gradient: a whole 32-pixel chain and a whole wave
    ref_args = [t.clone().requires_grad_(True) for t in (x, table, w1, w2, w3)]
    ref = OT.texture_mlp(*ref_args, BBOX, OMIN, OMAX) * mask[:, None]
    (ref * G).sum().backward()
    _TEX[n] = dict(x=x, table=table, w=(w1, w2, w3), mask=mask, G=G, ref=[a.grad.clone() for a in ref_args])
    return _TEX[n]


def _tex_run(dev, c, scale=1.0, x_grad=True, mask=None):
    from d3h import texmlp
    x = c['x'].clone().to(dev).requires_grad_(x_grad)
    rest = [t.clone().to(dev).requires_grad_(True) for t in (c['table'],) + c['w']]
    m = c['mask'] if mask is None else mask
    out = texmlp.texture_mlp(x, rest[0], rest[1], rest[2], rest[3], BBOX, OMIN, OMAX, mask=m.to(dev))
    (out * (c['G'] * scale).to(dev)).sum().backward()
    if dev != 'cpu':
        torch.cuda.synchronize()
    return [x.grad.cpu() if x_grad else None] + [t.grad.cpu() for t in rest]


def _rel(a, r):
    return float((a - r).abs().max() / (r.abs().max() + 1e-30))


def check_tex_dx_fused(dev, n=700):
    """d_x from the MLP half against the oracle; clamped coordinates and masked pixels give exact zeros"""
    c = _tex_inputs(n)
    with _tex_fused(True):
        got = _tex_run(dev, c)
    for a, r, name in zip(got, c['ref'], ('x', 'table', 'w1', 'w2', 'w3')):
        assert _rel(a, r) < TEX_BAR, (n, name, _rel(a, r))
    b0, b1 = torch.tensor(BBOX[:3]), torch.tensor(BBOX[3:])
    v = (c['x'] - b0) / (b1 - b0)
    outside = (v < -1e-6) | (v > 1 + 1e-6)
    assert int(outside.sum()) > 0 or n < 50
    assert float(got[0][outside].abs().max() if outside.any() else 0.0) == 0.0, 'clamped coordinate with a gradient'
    assert float(got[0][c['mask'] == 0].abs().max() if (c['mask'] == 0).any() else 0.0) == 0.0, 'masked pixel with a gradient'
    assert float(got[0][0].abs().max()) > 0.0            # the x_n == 1 corner is inside the box: it takes a gradient
    return got


def check_tex_dx_partial(dev):
    """partial chains and waves"""
    for n in (5, 33, 64 + 1):
        check_tex_dx_fused(dev, n)


def check_tex_dx_all_masked(dev, n=130):
    c = _tex_inputs(n)
    with _tex_fused(True):
        got = _tex_run(dev, c, mask=torch.zeros(n))
    for a, name in zip(got, ('x', 'table', 'w1', 'w2', 'w3')):
        assert float(a.abs().max()) == 0.0, name


def check_tex_dx_tiny_upstream(dev, n=700):
    c = _tex_inputs(n)
    with _tex_fused(True):
        unit = _tex_run(dev, c)
        tiny = _tex_run(dev, c, scale=3e-7)
    assert _rel(tiny[0] / 3e-7, unit[0]) < TEX_SCALE_BAR, _rel(tiny[0] / 3e-7, unit[0])


def check_tex_dx_x_without_grad(dev, n=700):
    """x not requiring grad: the kernel gets d_x NULL; table and weight gradients as with it"""
    c = _tex_inputs(n)
    with _tex_fused(True):
        with_x = _tex_run(dev, c)
        without = _tex_run(dev, c, x_grad=False)
    for a, r, name in zip(without[1:], with_x[1:], ('table', 'w1', 'w2', 'w3')):
        assert _rel(a, r) < TEX_SCALE_BAR, (name, _rel(a, r))
        assert _rel(a, c['ref'][1 + ('table', 'w1', 'w2', 'w3').index(name)]) < TEX_BAR


def check_tex_dx_async_on_off(dev, n=700):
    """table scatter on its side stream or not, fused d_x or the three-call sequence: same d_x and table gradient"""
    c = _tex_inputs(n)
    res = {}
    for fused in (True, False):
        for a in (True, False):
            with _tex_fused(fused, async_grad=a):
                res[(fused, a)] = _tex_run(dev, c)
    base = res[(True, False)]
    for k, got in res.items():
        assert _rel(got[0], base[0]) < TEX_SCALE_BAR, (k, 'x', _rel(got[0], base[0]))
        assert _rel(got[1], base[1]) < TEX_SCALE_BAR, (k, 'table', _rel(got[1], base[1]))


# ---- G-buffer / rasteriser backward ---------------------------------------------------------------------------------------------------
def _gbuf_scene(dev, posn, f, H, W):
    """one device rasterisation of the scene (kept with its graph for rasterize-backward), shared by the combinations"""
    from d3h import raster
    pos = T(posn, dev, True)
    tri = T(f.astype(np.int32), dev)
    rs, _ = raster.rasterize(pos, tri, (H, W))
    return dict(posn=posn, f=f, H=H, W=W, pos=pos, tri=tri, rs=rs, tri_o=torch.from_numpy(f.astype(np.int64)))


def _gbuf_combo(dev, sc, batched, need, with_face, gen):
    """both entry points on one scene: d3h_gbuffer_bwd (d(attr), d(face), d(rast) against the oracle) and d3h_gbuffer_raster_bwd (same
    d(attr) / d(face); d(pos) against rasterize-backward of the separate path's d(rast))"""
    from d3h import raster
    from oracle import raster as OR
    rs_dev = sc['rs'].detach()
    rs_cpu = rs_dev.cpu()
    nb, H, W = rs_cpu.shape[:3]
    V, Fn = sc['posn'].shape[1], sc['f'].shape[0]
    attrn = torch.randn(nb if batched else 1, V, 10, generator=gen)
    facen = torch.randn(nb if batched else 1, Fn, 3, generator=gen) if with_face else None
    Gs = [torch.randn(nb, H, W, w, generator=gen) for w in WIDTHS]
    Gf = torch.randn(nb, H, W, 3, generator=gen)
    # oracle
    attr_o = attrn.clone().requires_grad_(True)
    rs_o = rs_cpu.clone().requires_grad_(True)
    out_o, _ = OR.interpolate(attr_o, rs_o, sc['tri_o'], None)
    loss_o, c0 = 0.0, 0
    for k, w in enumerate(WIDTHS):
        if need[k]:
            loss_o = loss_o + (out_o[..., c0:c0 + w] * Gs[k]).sum()
        c0 += w
    fa_o = None
    if with_face:
        fa_o = facen.clone().requires_grad_(True)
        fidx_o = torch.arange(Fn)[:, None].expand(-1, 3).contiguous()
        face_o, _ = OR.interpolate(fa_o, rs_o, fidx_o, None)
        loss_o = loss_o + (face_o * Gf).sum()
    loss_o.backward()

    def run(fold):
        attr = attrn.clone().to(dev).requires_grad_(True)
        fa = facen.clone().to(dev).requires_grad_(True) if with_face else None
        pos = sc['pos'].detach().clone().requires_grad_(True)
        rs = rs_dev.clone().requires_grad_(True)
        groups, face_img, _ = raster.gbuffer(attr, WIDTHS, rs, sc['tri'], need=need, face_attr=fa, want_mask=False, raster_pos=pos if fold else None)
        loss = sum((groups[k] * Gs[k].to(dev)).sum() for k in range(4) if need[k])
        if with_face:
            loss = loss + (face_img * Gf.to(dev)).sum()
        loss.backward()
        return attr.grad, (fa.grad if with_face else None), (pos.grad if fold else rs.grad)

    d_attr, d_face, d_rast = run(False)
    den = float(rs_o.grad[..., :2].abs().max())
    assert float(attr_o.grad.abs().max()) > 0 or float((rs_cpu[..., 3] > 0).sum()) == 0
    assert (d_attr.cpu() - attr_o.grad).abs().max() <= GBUF_BAR * attr_o.grad.abs().max(), ('d_attr', batched, need, with_face)
    if with_face:
        assert (d_face.cpu() - fa_o.grad).abs().max() <= GBUF_BAR * fa_o.grad.abs().max(), ('d_face', batched, need, with_face)
    assert (d_rast.cpu()[..., :2] - rs_o.grad[..., :2]).abs().max() <= GBUF_BAR * den, ('d_rast', batched, need, with_face)
    assert float(d_rast[..., 2:].abs().max()) == 0.0
    # folded: d(pos) against rasterize-backward of the separate path's d(rast)
    sc['pos'].grad = None
    sc['rs'].backward(d_rast, retain_graph=True)
    pos_ref = sc['pos'].grad.detach().clone()
    f_attr, f_face, f_pos = run(True)
    assert (f_pos - pos_ref).abs().max() <= FOLD_BAR * pos_ref.abs().max(), ('d_pos', batched, need, with_face,
                                                                              float((f_pos - pos_ref).abs().max() / (pos_ref.abs().max() + 1e-30)))
    assert float(f_pos[..., 2].abs().max()) == 0.0
    assert (f_attr.cpu() - attr_o.grad).abs().max() <= GBUF_BAR * attr_o.grad.abs().max()
    assert (f_attr - d_attr).abs().max() <= FOLD_BAR * d_attr.abs().max()
    if with_face:
        assert (f_face.cpu() - fa_o.grad).abs().max() <= GBUF_BAR * fa_o.grad.abs().max()
        assert (f_face - d_face).abs().max() <= FOLD_BAR * d_face.abs().max()


COMBOS = ((True, (True, True, True, True), True), (False, (False, True, False, True), True), (True, (True, False, True, False), False),
          (False, (True, True, True, True), False))


def check_gbuf_lds_mesh(dev, H=40, W=56, nb=2, combos=COMBOS, tile=None):
    """the mesh of check_gbuffer on frames ragged against every tile shape, in both dimensions"""
    tw, th = (int(v) for v in tile.split('x')) if tile else TILES[0]
    assert H % th and W % tw
    posn, f = _raster_scene(48, nb)
    gen = torch.Generator().manual_seed(160)
    with _env(D3H_GBUF_LDS='1', D3H_GBUF_LDS_SLOTS=None, D3H_GBUF_TILE=tile):
        sc = _gbuf_scene(dev, posn, f, H, W)
        assert float((sc['rs'][..., 3] > 0).float().mean()) > 0.05
        for batched, need, with_face in combos:
            _gbuf_combo(dev, sc, batched, need, with_face, gen)


def check_gbuf_lds_tiles(dev):
    """every other tile shape the launcher knows, one combination each"""
    for tw, th in TILES[1:]:
        check_gbuf_lds_mesh(dev, H=42, W=59, combos=COMBOS[:1], tile=f'{tw}x{th}')     # (42 x 59: a multiple of no tile side)


def check_gbuf_lds_one_triangle(dev, H=40, W=56):
    """one triangle over the whole frame -- every tile flushes the same three rows -- and one empty frame"""
    posn = np.array([[[-1.5, -1.5, 0.1, 1.0], [4.0, -1.2, 0.2, 1.0], [-1.2, 4.0, -0.1, 1.0]],
                     [[2.5, 2.5, 0.0, 1.0], [3.5, 2.5, 0.0, 1.0], [2.5, 3.5, 0.0, 1.0]]], np.float32)
    f = np.array([[0, 1, 2]], np.int64)
    gen = torch.Generator().manual_seed(161)
    with _env(D3H_GBUF_LDS='1', D3H_GBUF_LDS_SLOTS=None, D3H_GBUF_TILE=None):
        sc = _gbuf_scene(dev, posn, f, H, W)
        cov = sc['rs'][..., 3] > 0
        assert bool(cov[0].all()) and not bool(cov[1].any())
        for batched in (True, False):
            _gbuf_combo(dev, sc, batched, (True, True, True, True), True, gen)


def check_gbuf_lds_overflow(dev, H=40, W=56, slots=8):
    """a table of 8 slots and a lattice of sub-pixel triangles with distinct vertices inside one tile: the tile sees more than 8 distinct
    vertices (asserted from the oracle's raster), so contributions take the direct-atomic path; the bars hold all the same"""
    from oracle import raster as OR
    tris, verts = [], []
    for fr in range(2):
        vs = []
        for r in range(4):
            for c in range(16):
                cx, cy = c + 0.5 + fr, r + 0.5          # pixel centres; the second frame one pixel to the right
                for dx, dy in ((-0.3, -0.3), (0.3, -0.3), (0.0, 0.35)):
                    vs.append([2.0 * (cx + dx) / W - 1.0, 2.0 * (cy + dy) / H - 1.0, 0.0, 1.0])
        verts.append(vs)
    posn = np.array(verts, np.float32)
    f = np.arange(3 * 64, dtype=np.int64).reshape(-1, 3)
    rast_o, _ = OR.rasterize(torch.from_numpy(posn), torch.from_numpy(f), H, W)
    ids = rast_o[0, ..., 3].long()
    ys, xs = torch.nonzero(ids > 0, as_tuple=True)
    assert len(ys) >= 32
    for tw, th in TILES:
        per_tile = {}
        for y, x in zip(ys.tolist(), xs.tolist()):
            per_tile.setdefault((y // th, x // tw), set()).update(f[ids[y, x] - 1].tolist())
        assert max(len(v) for v in per_tile.values()) > slots, (tw, th)
    gen = torch.Generator().manual_seed(162)
    with _env(D3H_GBUF_LDS='1', D3H_GBUF_LDS_SLOTS=slots, D3H_GBUF_TILE=None):
        sc = _gbuf_scene(dev, posn, f, H, W)
        assert torch.equal(sc['rs'].detach().cpu()[..., 3], rast_o[..., 3])
        _gbuf_combo(dev, sc, True, (True, True, True, True), True, gen)
        _gbuf_combo(dev, sc, False, (True, True, False, True), True, gen)
    with _env(D3H_GBUF_LDS='1', D3H_GBUF_LDS_SLOTS=0, D3H_GBUF_TILE=None):           # no table at all: everything direct
        _gbuf_combo(dev, sc, True, (True, True, True, True), True, gen)


def check_gbuf_lds_1080(dev):
    """one 1080 x 1080 frame (a multiple of no tile) of the check_gbuffer mesh"""
    posn, f = _raster_scene(1080, 1)
    gen = torch.Generator().manual_seed(163)
    with _env(D3H_GBUF_LDS='1', D3H_GBUF_LDS_SLOTS=None, D3H_GBUF_TILE=None):
        sc = _gbuf_scene(dev, posn, f, 1080, 1080)
        _gbuf_combo(dev, sc, True, (True, True, True, True), True, gen)
