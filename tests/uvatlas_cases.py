"""Check functions of the textured-mesh export -- the triangle-pair atlas and the bake (csrc/uvatlas.hip, d3h/uvatlas.py), the mip op, render/texture.py,
render/material.py, d3h/export.py -- shared by tests/test_uvatlas_emul.py (host emulation of the kernel sources) and tests/test_gpu_uvatlas.py
(MI355X).  Same shapes on both.  Every mesh is generated here from a seed; tests/golden/texture2d.npz holds the upstream project's own results
(tools/gen_golden.py texture2d).

The yardstick is a restatement of the layout and bake formulas in numpy: everything that is an integer or a decision (cell size, slots, ownership,
the half, `inside`, the owning face) is computed in exact integer arithmetic and must be EQUAL; positions are evaluated in float64.

Parity rule for the float tensors (the project's rule, tests/renderutils_cases.py): max|got - f64| / max|f64| <= max(5 * ref32_err, 2^-20) per
tensor, f64 the yardstick in float64 and ref32_err the distance of the same yardstick evaluated in float32.  Every figure is printed before it is
asserted (run with -s).  Where the golden fixture is the float32 evaluation (upstream's own float32 result on the same inputs), it takes the place
of ref32.  Fixture entries with no float64 restatement here (Texture2D.sample) are held to 2^-20 of the tensor's largest value directly: got and
golden are two float32 evaluations of one formula -- a mip chain of at most 3 means and an 8-tap blend, each within a few 2^-24 of exact."""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

from conftest import golden
from d3h import uvatlas as UA

FLOOR = 2.0 ** -20
CASES = ((1, 8, 8), (2, 5, 5), (37, 64, 64), (20, 40, 96), (301, 128, 128))
EXPECT = {(1, 8, 8): (8, 1, 1), (2, 5, 5): (5, 1, 1), (37, 64, 64): (12, 5, 5), (20, 40, 96): (19, 5, 2), (301, 128, 128): (9, 14, 14), (0, 8, 8): (8, 1, 1)}
MIP_SHAPES = ((1, 2, 2, 1), (2, 6, 4, 3), (1, 8, 8, 4), (1, 4, 4, 6))


def rel(got, ref):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def assert_close(what, got, ref, ref32):
    ref32_err = rel(ref32, ref)
    tol = max(5.0 * ref32_err, FLOOR)
    r = rel(got, ref)
    print(f'{what:56s} {r:.3e}  (ref32_err {ref32_err:.2e}, bound {tol:.3e}, {r / tol:.2f} of it)')
    assert r <= tol, (what, r, tol)


def assert_floor(what, got, ref):
    r = rel(got, ref)
    print(f'{what:56s} {r:.3e}  (bound {FLOOR:.3e})')
    assert r <= FLOOR, (what, r)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


@functools.lru_cache(maxsize=None)
def mesh(F):
    """an indexed mesh of F random triangles over F + 2 vertices in [-1, 1]^3 (distinct corners per face)"""
    rng = _rng(f'uvatlas mesh {F}')
    v = rng.uniform(-1.0, 1.0, (F + 2, 3)).astype(np.float32)
    t = np.stack([rng.permutation(F + 2)[:3] for _ in range(F)]).astype(np.int64) if F else np.zeros((0, 3), np.int64)
    return v, t


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------
def yard_cell(F, H, W):
    cells = (F + 1) // 2
    s = max((k for k in range(1, min(H, W) + 1) if (W // k) * (H // k) >= cells), default=0)
    return (s, W // s, H // s) if s else (0, 0, 0)


def yard_rot(v, t, dtype=np.float64):
    """-> (rot [F], unambiguous [F]): the corner opposite the longest edge, lowest index on ties; unambiguous where the longest squared edge beats the
    others by 1e-5 relative (a float32 evaluation decides the same)"""
    p = v.astype(dtype)[t]
    l = np.stack([((p[:, (k + 1) % 3] - p[:, (k + 2) % 3]) ** 2).sum(-1) for k in range(3)], -1)
    rot = l.argmax(-1)                                  # the first maximum
    top = np.sort(l, -1)
    return rot.astype(np.uint8), top[:, 2] > top[:, 1] * (1 + 1e-5)


def yard_slots(F, s, nx, rot):
    """integer texel-corner coordinates [3F, 2] of the uv vertices (row 3 f + corner)"""
    f = np.arange(F)
    c, h = f // 2, f % 2
    cx, cy = c % nx, c // nx
    q = np.array([[1, 1], [s - 3, 1], [1, s - 3]])
    out = np.zeros((F, 3, 2), np.int64)
    for k in range(3):
        slot = np.where(h[:, None] == 0, q[k][None], s - q[k][None])
        out[f, (rot.astype(np.int64) + k) % 3] = np.stack([cx, cy], -1) * s + slot
    return out.reshape(-1, 2)


def yard_bake(v, t, rot, s, nx, ny, H, W, dtype=np.float64):
    """-> pos [H,W,3] (dtype), owned, inside [H,W] bool, tri [H,W] int: steps 1-8 of the bake.  The decisions in integers of HALF texels; the
    barycentrics and the position in `dtype` as the formulas state them (b0 = 1 - b1 - b2)"""
    F = len(t)
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    cx, cy = i // s, j // s
    x2, y2 = 2 * (i - cx * s) + 1, 2 * (j - cy * s) + 1
    h = (x2 + y2 > 2 * s).astype(np.int64)
    f = 2 * (cy * nx + cx) + h
    owned = (cx < nx) & (cy < ny) & (f < F)
    x2, y2 = np.where(h == 1, 2 * s - x2, x2), np.where(h == 1, 2 * s - y2, y2)
    inside = owned & (x2 >= 2) & (y2 >= 2) & (2 * (s - 4) - (x2 - 2) - (y2 - 2) >= 0)
    tri = np.where(owned, f, -1).astype(np.int32)
    pos = np.zeros((H, W, 3), dtype)
    if F:
        one, half = dtype(1.0), dtype(0.5)
        x, y = x2.astype(dtype) * half, y2.astype(dtype) * half
        b1, b2 = (x - one) / dtype(s - 4), (y - one) / dtype(s - 4)
        b0 = one - b1 - b2
        fo = np.where(owned, f, 0)
        r = rot.astype(np.int64)[fo]
        P = v.astype(dtype)[t[fo[..., None], (r[..., None] + np.arange(3)) % 3]]               # [H,W,3 corners,3]
        pos = (b0[..., None] * P[..., 0, :] + b1[..., None] * P[..., 1, :] + b2[..., None] * P[..., 2, :]).astype(dtype)
        pos[~owned] = 0
    return pos, owned, inside, tri


def bilinear(tex, uv):
    """level-0 bilinear lookup with clamped taps in the dtype of `tex` [H,W,C] at uv [N,2] -> (value [N,C], taps [N,4,2] (x, y), weights [N,4])"""
    H, W = tex.shape[:2]
    dt = tex.dtype.type
    x, y = uv[:, 0].astype(dt) * dt(W) - dt(0.5), uv[:, 1].astype(dt) * dt(H) - dt(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    xs = np.clip(np.stack([x0, x0 + 1, x0, x0 + 1], -1), 0, W - 1).astype(np.int64)
    ys = np.clip(np.stack([y0, y0, y0 + 1, y0 + 1], -1), 0, H - 1).astype(np.int64)
    w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], -1).astype(dt)
    return (tex[ys, xs] * w[..., None]).sum(1), np.stack([xs, ys], -1), w


def _t(a, dev, dtype=None):
    return torch.as_tensor(a, dtype=dtype).to(dev)


# ---- 1. layout -------------------------------------------------------------------------------------------------------------------------
def check_layout(dev, case):
    F, H, W = case
    v, t = mesh(F)
    tv, tt = _t(v, dev), _t(t, dev)
    A = UA.make_atlas(tv, tt, (H, W))
    assert (A.s, A.nx, A.ny) == EXPECT[case] == yard_cell(F, H, W) and tuple(A.resolution) == (H, W)
    assert A.uvs.shape == (3 * F, 2) and A.uvs.dtype == torch.float32 and A.t_tex_idx.dtype == torch.int64 and A.rot.dtype == torch.uint8
    assert torch.equal(A.t_tex_idx.cpu(), torch.arange(3 * F).reshape(F, 3))
    assert torch.equal(A.vmapping.cpu(), torch.from_numpy(t).reshape(-1))
    assert torch.equal(tv[A.vmapping][A.t_tex_idx], tv[tt])
    uvs, rot = A.uvs.cpu(), A.rot.cpu().numpy()
    assert bool(((uvs >= 0) & (uvs <= 1)).all())
    ints = torch.from_numpy(yard_slots(F, A.s, A.nx, rot))
    assert torch.equal(uvs, ints.float() / torch.tensor([W, H], dtype=torch.float32)), 'uvs are not the correctly rounded quotients of the slot integers'
    yr, sure = yard_rot(v, t)
    assert sure.mean() > 0.9 if F > 10 else True
    assert np.array_equal(rot[sure], yr[sure])
    # int32 indices, a strided vertex array and a strided face array: the same atlas
    wide = torch.zeros(F + 2, 6, device=dev)
    wide[:, ::2] = tv
    tw = torch.zeros(F, 6, dtype=torch.int32, device=dev)
    tw[:, ::2] = tt.int()
    for vv, ff in ((tv, tt.int()), (wide[:, ::2], tt), (tv, tw[:, ::2])):
        assert not (vv is wide and vv.is_contiguous())
        B = UA.make_atlas(vv, ff, (H, W))
        assert torch.equal(B.uvs, A.uvs) and torch.equal(B.rot, A.rot) and torch.equal(B.t_tex_idx, A.t_tex_idx) and torch.equal(B.vmapping.long(), A.vmapping)


def check_layout_empty(dev):
    A = UA.make_atlas(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev), 8)
    assert (A.s, A.nx, A.ny) == EXPECT[(0, 8, 8)] and A.uvs.shape == (0, 2) and A.t_tex_idx.shape == (0, 3) and A.vmapping.shape == (0,) and A.rot.shape == (0,)
    pos, owned, inside, tri = UA.bake_positions(A, torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev))
    assert pos.shape == (1, 8, 8, 3) and not pos.any() and not owned.any() and not inside.any() and bool((tri == -1).all())


def check_layout_too_small(dev):
    v, t = mesh(3)
    with pytest.raises(ValueError, match=r'\b10\b'):
        UA.make_atlas(_t(v, dev), _t(t, dev), (5, 5))
    UA.make_atlas(_t(v, dev), _t(t, dev), (10, 10))                # the resolution the message names does work


def check_rotation_rule(dev):
    """an obtuse triangle with the obtuse angle at corner 0, 1, 2 (longest edge 1.58 x the next); the exact equilateral; two equal vertices"""
    obt = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-0.5, 0.5, 0.0]], np.float32)
    l = sorted(float(((obt[a] - obt[b]) ** 2).sum()) ** 0.5 for a, b in ((0, 1), (1, 2), (2, 0)))
    assert l[2] >= 1.001 * l[1]
    tris = [np.roll(obt, r, axis=0) + r for r in range(3)]                      # the obtuse corner at index r
    tris.append(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32))
    tris.append(np.array([[0.3, 0.2, 0.1], [0.3, 0.2, 0.1], [1, 1, 1]], np.float32))
    v = np.concatenate(tris).astype(np.float32)
    t = np.arange(15).reshape(5, 3)
    A = UA.make_atlas(_t(v, dev), _t(t, dev), 16)
    assert A.rot.cpu().tolist() == [0, 1, 2, 0, 0]
    assert bool(torch.isfinite(A.uvs).all())
    pos, owned, inside, tri = UA.bake_positions(A, _t(v, dev), _t(t, dev))
    assert bool(torch.isfinite(pos).all())
    yp, yo, yi, yt = yard_bake(v, t, A.rot.cpu().numpy(), A.s, A.nx, A.ny, 16, 16)
    assert np.array_equal(tri[0].cpu().numpy(), yt)
    assert_close('bake of the rotation-rule mesh', pos[0], yp, yard_bake(v, t, A.rot.cpu().numpy(), A.s, A.nx, A.ny, 16, 16, np.float32)[0])


# ---- 2. bake ---------------------------------------------------------------------------------------------------------------------------
def _bake_against_yardstick(what, dev, A, v, t, H, W):
    pos, owned, inside, tri = UA.bake_positions(A, _t(v, dev), _t(t, dev))
    assert pos.shape == (1, H, W, 3) and owned.shape == (1, H, W, 1) and inside.shape == (1, H, W, 1) and tri.shape == (1, H, W) and tri.dtype == torch.int32
    rot = A.rot.cpu().numpy()
    yp, yo, yi, yt = yard_bake(v, t, rot, A.s, A.nx, A.ny, H, W)
    yp32 = yard_bake(v, t, rot, A.s, A.nx, A.ny, H, W, np.float32)[0]
    assert np.array_equal(owned[0, ..., 0].cpu().numpy(), yo.astype(np.float32))
    assert np.array_equal(inside[0, ..., 0].cpu().numpy(), yi.astype(np.float32))
    assert np.array_equal(tri[0].cpu().numpy(), yt)
    assert_close(what, pos[0], yp, yp32)
    return pos, owned, inside, tri


def check_bake(dev, case):
    F, H, W = case
    v, t = mesh(F)
    A = UA.make_atlas(_t(v, dev), _t(t, dev), (H, W))
    _, owned, inside, _ = _bake_against_yardstick(f'bake pos {case}', dev, A, v, t, H, W)
    assert int(owned.sum()) > 0 and int(inside.sum()) >= F                         # every triangle has texels of its own
    # another pose of the same faces: the rotation is the atlas's, not recomputed
    v2 = _rng(f'uvatlas pose {F}').uniform(-1.0, 1.0, v.shape).astype(np.float32)
    if F >= 20:
        assert (yard_rot(v2, t)[0] != A.rot.cpu().numpy()).any()
    _bake_against_yardstick(f'bake pos {case}, second pose', dev, A, v2, t.astype(np.int32), H, W)


# ---- 3. seam-free ----------------------------------------------------------------------------------------------------------------------
def surface_points(F, n=4000):
    """n points (face, barycentrics): 70 % interior, 30 % with one or two barycentrics exactly zero (edges and corners)"""
    rng = _rng(f'uvatlas points {F}')
    f = rng.integers(0, F, n)
    b = rng.dirichlet((1.0, 1.0, 1.0), n)
    k = int(0.3 * n)
    b[np.arange(k), rng.integers(0, 3, k)] = 0.0
    b[np.arange(k // 3), rng.integers(0, 3, k // 3)] = 0.0                          # a third of those: possibly a second zero (a corner)
    dead = b.sum(-1) == 0
    b[dead] = (1.0, 0.0, 0.0)
    return f, b / b.sum(-1, keepdims=True)


def check_seamfree(dev, case):
    import nvdiffrast.torch as dr
    F, H, W = case
    v, t = mesh(F)
    A = UA.make_atlas(_t(v, dev), _t(t, dev), (H, W))
    pos, owned, inside, tri = UA.bake_positions(A, _t(v, dev), _t(t, dev))
    rot = A.rot.cpu().numpy()
    f, b = surface_points(F)
    corners = yard_slots(F, A.s, A.nx, rot).reshape(F, 3, 2).astype(np.float64) / np.array([W, H], np.float64)
    uv = (b[:, :, None] * corners[f]).sum(1)
    true = (b[:, :, None] * v.astype(np.float64)[t[f]]).sum(1)
    uv32 = uv.astype(np.float32)
    got = dr.texture(pos, _t(uv32, dev)[None, None].contiguous(), filter_mode='linear', boundary_mode='clamp')[0, 0]
    ref32, taps, w = bilinear(yard_bake(v, t, rot, A.s, A.nx, A.ny, H, W, np.float32)[0], uv32)
    assert_close(f'bilinear lookup of the bake {case}', got, true, ref32)
    # the float64 lookup of the float64 bake is the true position: the layout, not luck
    exact = bilinear(yard_bake(v, t, rot, A.s, A.nx, A.ny, H, W)[0], uv)
    assert rel(exact[0], true) < 1e-12
    tri_np = tri[0].cpu().numpy()
    for tp, ww in ((taps, w), (exact[1], exact[2])):
        owner = tri_np[tp[..., 1], tp[..., 0]]
        foreign = (ww != 0) & (owner != f[:, None])
        print(f'  taps on foreign texels: {int(foreign.sum())} of {int((ww != 0).sum())}')
        assert not foreign.any()


# ---- 4. against the rasteriser ---------------------------------------------------------------------------------------------------------
class _PositionAsColour:
    """stands in for the MLP material of render_uv: kd = ks = the interpolated position"""

    def sample(self, p, *a, **k):
        return torch.cat((p, p), dim=-1)


def check_against_rasteriser(dev):
    import nvdiffrast.torch as dr
    from d3h import synth
    from render import mesh as rmesh, render as rrender
    v, t = synth.icosphere(1)
    H = W = 64
    tv, tt = _t(v, dev), _t(t, dev)
    A = UA.make_atlas(tv, tt, (H, W))
    pos, owned, inside, tri = UA.bake_positions(A, tv, tt)
    m = rmesh.Mesh(tv, tt, v_tex=A.uvs, t_tex_idx=A.t_tex_idx)
    cover, kd, _ = rrender.render_uv(dr.RasterizeGLContext(), m, [H, W], _PositionAsColour())
    c = cover[0, ..., 0] > 0
    assert int(c.sum()) > 0.2 * H * W * (A.s - 4) ** 2 / A.s ** 2
    assert bool((inside[0, ..., 0][c] == 1).all())
    rot = A.rot.cpu().numpy()
    y64 = torch.from_numpy(yard_bake(v, t, rot, A.s, A.nx, A.ny, H, W)[0])
    y32 = torch.from_numpy(yard_bake(v, t, rot, A.s, A.nx, A.ny, H, W, np.float32)[0])
    c = c.cpu()
    assert_close('bake pos where the rasteriser covers', pos[0].cpu()[c], y64[c], y32[c])
    assert_close('rasterised + interpolated position', kd[0].cpu()[c], y64[c], y32[c])


# ---- 5. the mip op ---------------------------------------------------------------------------------------------------------------------
def _mip_yardstick(x, dout, dtype):
    x = x.to(dtype).permute(0, 3, 1, 2)
    y = torch.nn.functional.avg_pool2d(x, 2).permute(0, 2, 3, 1)
    g = torch.nn.functional.interpolate(0.25 * dout.to(dtype).permute(0, 3, 1, 2), scale_factor=2, mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    return y, g


def check_mip(dev, i):
    from render import texture as RT
    G = golden('texture2d.npz')
    x, dout = torch.from_numpy(G[f'mip{i}.x']), torch.from_numpy(G[f'mip{i}.dout'])
    assert tuple(x.shape) == MIP_SHAPES[i]
    xd = x.to(dev).requires_grad_(True)
    y = RT.texture2d_mip.apply(xd)
    y.backward(dout.to(dev))
    y64, g64 = _mip_yardstick(x, dout, torch.float64)
    y32, g32 = _mip_yardstick(x, dout, torch.float32)
    assert_close(f'mip forward {MIP_SHAPES[i]} vs float64', y, y64, y32)
    assert_close(f'mip backward {MIP_SHAPES[i]} vs float64', xd.grad, g64, g32)
    assert_close(f'mip forward {MIP_SHAPES[i]}, golden as the float32 run', y, y64, torch.from_numpy(G[f'mip{i}.out']))
    if f'mip{i}.grad' in G.files:                     # upstream's backward exists for one image only
        assert_close(f'mip backward {MIP_SHAPES[i]}, golden as the float32 run', xd.grad, g64, torch.from_numpy(G[f'mip{i}.grad']))
    else:
        assert MIP_SHAPES[i][0] > 1
    # strided input, the plain function
    wide = torch.zeros(*x.shape[:3], 2 * x.shape[3], device=dev)
    wide[..., ::2] = x.to(dev)
    assert torch.equal(UA.mip2x2(wide[..., ::2]), y.detach())


def check_mip_odd_raises(dev):
    from render import texture as RT
    for shp in ((1, 3, 4, 1), (1, 4, 3, 2)):
        with pytest.raises(ValueError):
            RT.texture2d_mip.apply(torch.zeros(*shp, device=dev))


# ---- 6. Texture2D and material ---------------------------------------------------------------------------------------------------------
def check_texture2d_golden(dev):
    from render import texture as RT
    G = golden('texture2d.npz')
    T = lambda k: torch.from_numpy(G[k]).to(dev)
    uv, uv_da, wgt = T('sample.uv'), T('sample.uv_da'), T('sample.wgt')
    img = T('auto.tex').requires_grad_(True)
    tex = RT.Texture2D(img)
    assert tuple(tex.getRes()) == (8, 8) and tex.getChannels() == 3 and len(tex.getMips()) == 1 and tex.parameters()[0] is img
    o = tex.sample(uv, uv_da)
    (o * wgt).sum().backward()
    assert_floor('Texture2D.sample, one image with on-the-fly mips', o, T('auto.out'))
    assert_floor('  its texture gradient', img.grad, T('auto.grad'))
    o3 = RT.Texture2D(img.detach()[0]).sample(uv, uv_da)                          # the HWC constructor form
    assert torch.equal(o3, o.detach())
    levels = [T(f'list.level{k}').requires_grad_(True) for k in range(4)]
    chain = RT.Texture2D(levels)
    assert len(chain.getMips()) == 4 and tuple(chain.getRes()) == (8, 4)
    o = chain.sample(uv, uv_da)
    (o * wgt).sum().backward()
    assert_floor('Texture2D.sample, custom mip chain', o, T('list.out'))
    for k, lv in enumerate(levels):
        assert lv.grad is not None and float(lv.grad.abs().sum()) > 0, f'no gradient reaches level {k}'
        assert_floor(f'  gradient of level {k}', lv.grad, T(f'list.grad{k}'))
    assert_floor('Texture2D.sample, constant', RT.Texture2D(T('const.value')).sample(uv, uv_da), T('const.out'))
    assert_floor('  from a numpy constant', RT.Texture2D(G['const.value']).sample(uv.to(RT._device()), uv_da.to(RT._device())), T('const.out'))
    one = RT.Texture2D([img.detach()])
    assert torch.is_tensor(one.data) and one.data.shape == (1, 8, 8, 3)
    t = RT.create_trainable(T('trainable.init'), res=[8, 8], auto_mipmaps=False)
    assert [tuple(lv.shape) for lv in t.data] == [(1, 8, 8, 3), (1, 4, 4, 3), (1, 2, 2, 3), (1, 1, 1, 3)]
    for k, lv in enumerate(t.data):
        assert lv.requires_grad and lv.is_leaf
        assert_floor(f'create_trainable(auto_mipmaps=False) level {k}', lv, T(f'trainable.level{k}'))
    auto = RT.create_trainable(RT.Texture2D(T('clamp.data'), min_max=[T('clamp.lo'), T('clamp.hi')]))
    assert torch.is_tensor(auto.data) and auto.data.requires_grad and auto.min_max is not None
    with torch.no_grad():
        auto.clamp_()
    assert torch.equal(auto.data.detach(), T('clamp.out'))
    n = RT.Texture2D(T('clamp.data').clone())
    n.normalize_()
    assert torch.allclose(n.data.norm(dim=-1), torch.ones(1, 4, 4, device=dev), atol=1e-6)


def check_material_roundtrip(dev, tmp_path):
    from render import material as RM, texture as RT, util
    G = golden('texture2d.npz')
    g = torch.Generator().manual_seed(7)
    kd, ks, nrm = (torch.rand(1, 6, 4, 3, generator=g).to(dev) for _ in range(3))
    mat = {'bsdf': 'pbr', 'kd': RT.Texture2D(kd), 'ks': RT.Texture2D(ks), 'normal': RT.Texture2D(nrm * 2 - 1)}
    fn = os.path.join(str(tmp_path), 'mesh.mtl')
    RM.save_mtl(fn, mat)
    assert open(fn).read() == str(G['mtl.text'])
    assert sorted(os.listdir(str(tmp_path))) == ['mesh.mtl', 'texture_kd.png', 'texture_ks.png', 'texture_n.png']
    back = RM.load_mtl(fn, clear_ks=False)
    assert len(back) == 1 and back[0]['name'] == 'defaultMat' and back[0]['bsdf'] == 'pbr'
    q = lambda x: torch.round(255 * x) / 255
    want_kd = util.srgb_to_rgb(q(util.rgb_to_srgb(kd)))
    assert float((back[0]['kd'].data.to(dev) - want_kd).abs().max()) <= 1e-6
    assert float((back[0]['ks'].data.to(dev) - q(ks)).abs().max()) <= 1e-6
    want_n = q((util.safe_normalize(nrm * 2 - 1) + 1) * 0.5) * 2 - 1
    assert float((back[0]['normal'].data.to(dev) - want_n).abs().max()) <= 1e-6
    assert not RM.load_mtl(fn)[0]['ks'].data[..., 0].any()                        # clear_ks
    none = os.path.join(str(tmp_path), 'none.mtl')
    RM.save_mtl(none, None)
    assert open(none).read() == str(G['mtl.text_none'])
    # a custom chain is stored as name_0, name_1, ...
    chain = RT.create_trainable(kd, auto_mipmaps=False)
    RT.save_texture2D(os.path.join(str(tmp_path), 'c.png'), chain)
    again = RT.load_texture2D(os.path.join(str(tmp_path), 'c.png'))
    assert isinstance(again.data, list) and [tuple(l.shape) for l in again.data] == [tuple(l.shape[1:]) for l in chain.data]
    tr = RM.create_trainable(mat)
    assert tr['bsdf'] == 'pbr' and all(tr[k].data.requires_grad for k in ('kd', 'ks', 'normal')) and len(RM.get_parameters(tr)) == 3
    merged, tc, tf = RM.merge_materials([mat, mat], [[0.5, 0.5]] * 3, [[0, 1, 2], [0, 1, 2]], [0, 1])
    assert tuple(merged['kd'].getRes()) == (8, 8) and len(tc) == 6 and tf[1] == [3, 4, 5] and tc[3][0] == (1 + 0.5) / 2


# ---- 7. export end to end --------------------------------------------------------------------------------------------------------------
def check_export(dev, tmp_path):
    from d3h import export, synth
    from render import mesh as rmesh, mlptexture, obj, texture as RT
    v, t = synth.icosphere(1)
    t = t[:-1]                      # 31 faces: the last cell of the 4 x 4 grid keeps an unowned half
    tv = (_t(v, dev) * torch.tensor([0.35, 0.5, 0.15], device=dev) + torch.tensor([-0.1, -0.3, 0.0], device=dev)).contiguous()     # inside the texture's box
    tt = _t(t, dev)
    H = W = 64
    torch.manual_seed(11)
    lo, hi = torch.tensor([0, 0, 0, 0, 0.001, 0.0], device=dev), torch.tensor([1, 1, 1, 0, 1.0, 1.0], device=dev)
    mlp = mlptexture.MLPTexture3D((tv.min(0).values, tv.max(0).values), channels=6, min_max=[lo, hi])
    assert mlp.fused
    with torch.no_grad():
        mlp.encoder.params.uniform_(-0.5, 0.5)
    mat = {'bsdf': 'pbr', 'kd_ks': mlp, 'name': 'fit'}
    out = export.textured_mesh(rmesh.Mesh(tv[None].expand(2, -1, -1), tt, material=mat), mat, [H, W], [0, 0, 0], [1, 1, 1], [0, 0.001, 0], [0, 1, 1], [-1, -1, 0], [1, 1, 1])
    assert 'kd_ks' not in out.material and 'kd_ks' in mat and out.material['bsdf'] == 'pbr' and out.material['name'] == 'fit'
    A = UA.make_atlas(tv, tt, (H, W))
    pos, owned, _, _ = UA.bake_positions(A, tv, tt)
    assert torch.equal(out.v_tex, A.uvs) and torch.equal(out.t_tex_idx, A.t_tex_idx) and out.t_pos_idx is tt
    kd, ks, nrm = (out.material[k] for k in ('kd', 'ks', 'normal'))
    for tex in (kd, ks, nrm):
        assert isinstance(tex, RT.Texture2D) and tex.data.shape == (1, H, W, 3) and tex.data.requires_grad and tex.data.is_leaf and tex.min_max is not None
    assert bool((nrm.data == torch.tensor([0.0, 0.0, 1.0], device=dev)).all())
    # the yardstick: the composed float64 / float32 evaluation of the same network at the baked positions
    o = owned[0, ..., 0] > 0
    got = torch.cat((kd.data, ks.data), -1).detach()[0]
    with torch.no_grad():
        w = [mlp.net.net[i].weight.detach().cpu() for i in (0, 2, 4)]
        from oracle import texmlp as OT

        def ref(dtype):
            x = pos[0][o].cpu().to(dtype)
            b0, b1 = torch.tensor(mlp.BBOX[:3], dtype=dtype), torch.tensor(mlp.BBOX[3:], dtype=dtype)
            e = OT.grid_encode(torch.clamp((x - b0) / (b1 - b0), 0, 1), mlp.encoder.params.detach().cpu().to(dtype))
            h = torch.relu(torch.relu(e @ w[0].to(dtype).T) @ w[1].to(dtype).T) @ w[2].to(dtype).T
            return torch.sigmoid(h) * (hi.cpu().to(dtype) - lo.cpu().to(dtype)) + lo.cpu().to(dtype)
        r64, r32 = ref(torch.float64), ref(torch.float32)
    assert_close('exported kd / ks on owned texels vs the network', got[o].cpu(), r64, r32)
    assert torch.equal(got[o], mlp.sample(pos, mask=owned).detach()[0][o])
    mean = got[o].double().mean(0)
    assert int((~o).sum()) > 0
    assert float((got[~o].double() - mean).abs().max()) <= 1e-6
    folder = str(tmp_path)
    obj.write_obj(folder, out)
    assert sorted(os.listdir(folder)) == ['mesh.mtl', 'mesh.obj', 'texture_kd.png', 'texture_ks.png', 'texture_n.png']
    lines = open(os.path.join(folder, 'mesh.obj')).read().splitlines()
    vt = np.array([[float(x) for x in l.split()[1:]] for l in lines if l.startswith('vt ')])
    uv = A.uvs.cpu().numpy().astype(np.float64)
    assert vt.shape == (3 * len(t), 2) and np.abs(vt - np.stack([uv[:, 0], 1.0 - uv[:, 1]], -1)).max() <= 1e-12
    faces = [l.split()[1:] for l in lines if l.startswith('f ')]
    assert len(faces) == len(t)
    for i, fl in enumerate(faces):
        assert [int(c.split('/')[0]) - 1 for c in fl] == t[i].tolist() and [int(c.split('/')[1]) - 1 for c in fl] == [3 * i, 3 * i + 1, 3 * i + 2]
    from render import material as RM, util
    back = RM.load_mtl(os.path.join(folder, 'mesh.mtl'), clear_ks=False)[0]
    q = lambda x: torch.round(255 * x) / 255
    assert float((back['kd'].data.to(dev) - util.srgb_to_rgb(q(util.rgb_to_srgb(kd.data.detach())))).abs().max()) <= 1e-6


def check_entry_points_validate(dev):
    """argument errors come back as codes, not as launches"""
    from d3h import _lib as L
    lib = L.lib()
    z = torch.zeros(64, device=dev)
    zi = torch.zeros(64, dtype=torch.int64, device=dev)
    zb = torch.zeros(64, dtype=torch.uint8, device=dev)
    p = lambda t, off=0: L._PTR(t.data_ptr() + off)
    assert lib.d3h_uvatlas_layout(p(z), L.i64(4), p(zi), L.i32(1), L.i64(1), L.i32(4), L.i32(1), L.i32(8), L.i32(8), p(z), p(zi), p(zb), L.stream()) == -1     # s < 5
    assert lib.d3h_uvatlas_layout(None, L.i64(4), p(zi), L.i32(1), L.i64(1), L.i32(8), L.i32(1), L.i32(8), L.i32(8), p(z), p(zi), p(zb), L.stream()) == -1     # NULL
    assert lib.d3h_uvatlas_layout(p(z, 2), L.i64(4), p(zi), L.i32(1), L.i64(1), L.i32(8), L.i32(1), L.i32(8), L.i32(8), p(z), p(zi), p(zb), L.stream()) == -1  # misaligned
    assert lib.d3h_uvatlas_layout(p(z), L.i64(4), p(zi), L.i32(1), L.i64(3), L.i32(8), L.i32(1), L.i32(8), L.i32(8), p(z), p(zi), p(zb), L.stream()) == -1     # too many faces
    assert lib.d3h_uvatlas_bake(p(z), L.i64(4), p(zi), L.i32(1), L.i64(1), p(zb), L.i32(4), L.i32(1), L.i32(1), L.i32(8), L.i32(8), p(z), p(z), p(z), p(zi), L.stream()) == -1
    assert lib.d3h_uvatlas_bake(p(z), L.i64(4), p(zi), L.i32(1), L.i64(1), p(zb), L.i32(8), L.i32(1), L.i32(1), L.i32(8), L.i32(8), None, p(z), p(z), p(zi), L.stream()) == -1
    assert lib.d3h_mip2x2_fwd(None, L.i64(1), L.i32(1), L.i32(1), L.i32(1), p(z), L.stream()) == -1
    assert lib.d3h_mip2x2_fwd(p(z), L.i64(1), L.i32(0), L.i32(1), L.i32(1), p(z), L.stream()) == -1
    assert lib.d3h_mip2x2_bwd(p(z), L.i64(1), L.i32(1), L.i32(1), L.i32(1), p(z, 1), L.stream()) == -1
    L._keepalive.clear()
