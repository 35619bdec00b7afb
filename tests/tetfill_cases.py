"""Cases and checks for d3h.tetfill (csrc/tetfill.hip): the lattice clipped by the linear interpolant of a signed distance.  The yardstick is
`restate`, a sequential numpy restatement of d3h/tetfill.py's docstring (one parent at a time, Python ints and lists, no kernel logic
shared); the geometric checks read nothing but the returned tensors.  Used by tests/test_tetfill_emul.py and tests/test_gpu_tetfill.py."""
import functools

import numpy as np
import pytest
import torch

from d3h import synth

PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
PARITY = (None, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0)             # d3h/tetfill.py, by inside mask
CHILDREN = (0, 1, 3, 3, 1)
F32 = np.float32


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def cut_position(p0, p1, s0, s1):
    """mt_emit_verts' expression, every operation rounded to float32"""
    a, b = F32(s0), F32(-F32(s1))
    den = F32(a + b)
    sg = F32(1.0) if den > 0 else (F32(-1.0) if den < 0 else F32(0.0))
    den = F32(sg * F32(F32(abs(den)) + F32(1e-12)))
    if den == 0:
        den = F32(1e-12)
    w0, w1 = F32(b / den), F32(a / den)
    return np.array([F32(F32(F32(p0[c]) * w0) + F32(F32(p1[c]) * w1)) for c in range(3)], F32)


def split_prism(p):
    """[P0 P1 P2 | P3 P4 P5] -> (three tets, triangles exchanged?)"""
    p = list(p)
    k = p.index(min(p))
    swapped = k >= 3
    if swapped:
        p, k = p[3:] + p[:3], k - 3
    v = [p[(k + j) % 3] for j in range(3)] + [p[3 + (k + j) % 3] for j in range(3)]
    if min(v[1], v[5]) < min(v[2], v[4]):
        return [(v[0], v[1], v[2], v[5]), (v[0], v[1], v[5], v[4]), (v[0], v[4], v[5], v[3])], swapped
    return [(v[0], v[1], v[2], v[4]), (v[0], v[4], v[2], v[5]), (v[0], v[4], v[5], v[3])], swapped


def restate(pos, sdf, tets):
    """-> (v float32 [n,3], t int64 [m,4], n_inside, tets by inside corners [5]) as d3h/tetfill.py's docstring says, sequentially"""
    pos, sdf, tets = np.asarray(pos, F32), np.asarray(sdf, F32).reshape(-1), np.asarray(tets, np.int64).reshape(-1, 4)
    with np.errstate(invalid='ignore'):
        inside = ~(sdf > 0)
    new_id = np.cumsum(inside) - 1
    n_in = int(inside.sum())
    edges = np.unique(np.sort(tets[:, [a for p in PAIRS for a in p]].reshape(-1, 2), axis=1), axis=0) if len(tets) else np.zeros((0, 2), np.int64)
    cut_id, cuts = {}, []
    for a, b in edges.tolist():
        if inside[a] != inside[b]:
            cut_id[(a, b)] = n_in + len(cuts)
            cuts.append(cut_position(pos[a], pos[b], sdf[a], sdf[b]))
    v = np.concatenate([pos[inside], np.array(cuts, F32).reshape(-1, 3)])
    out, hist = [], [0] * 5
    for tet in tets.tolist():
        I = [k for k in range(4) if inside[tet[k]]]
        O = [k for k in range(4) if not inside[tet[k]]]
        hist[len(I)] += 1
        if not I:
            continue
        mask = sum(1 << k for k in I)
        V = lambda k: int(new_id[tet[k]])
        C = lambda i, o: cut_id[(min(tet[i], tet[o]), max(tet[i], tet[o]))]
        if len(I) == 4:
            kids, swapped = [tuple(V(k) for k in range(4))], False
        elif len(I) == 1:
            kids, swapped = [(V(I[0]), C(I[0], O[0]), C(I[0], O[1]), C(I[0], O[2]))], False
        elif len(I) == 2:
            kids, swapped = split_prism([V(I[0]), C(I[0], O[0]), C(I[0], O[1]), V(I[1]), C(I[1], O[0]), C(I[1], O[1])])
        else:
            kids, swapped = split_prism([V(I[0]), V(I[1]), V(I[2]), C(I[0], O[0]), C(I[1], O[0]), C(I[2], O[0])])
        a, b, c, d = (pos[i] for i in tet)
        negative = F32(np.dot(np.cross(F32(b - a), F32(c - a)).astype(F32), F32(d - a))) < 0
        flip = bool(PARITY[mask]) ^ swapped ^ bool(negative)
        out += [(k[0], k[2], k[1], k[3]) if flip else k for k in kids]
    return v, np.array(out, np.int64).reshape(-1, 4), n_in, hist


# ---- fields of the issue's table ----------------------------------------------------------------------------------------------------------
def _sphere(p, c, r):
    return np.linalg.norm(p - np.asarray(c, np.float64), axis=1) - r


def _field(name, p):
    p = p.astype(np.float64)
    if name == 'sphere4':
        return _sphere(p, (0, 0, 0), 0.62)
    if name == 'sphere8':
        return _sphere(p, (0.03, 0.01, -0.02), 0.7)
    if name == 'two_spheres10':
        return np.minimum(_sphere(p, (-0.45, 0, 0), 0.33), _sphere(p, (0.45, 0, 0), 0.33))
    if name == 'torus12':
        return np.sqrt((np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - 0.55) ** 2 + p[:, 2] ** 2) - 0.27
    if name == 'noise6':
        s = np.random.default_rng(0).standard_normal(p.shape[0])
        s[np.abs(p).max(1) > 0.99] = 1.0
        return s
    raise KeyError(name)


#        name: (cells per side, tets by inside corners or None, children or None, Euler characteristic of the boundary or None)
TABLE = {'sphere4': (4, (264, 84, 24, 12, 0), 192, 2),
         'sphere8': (8, (2212, 296, 186, 140, 238), 1512, 2),
         'two_spheres10': (10, (5424, 276, 144, 84, 72), 1032, 4),
         'torus12': (12, (8584, 604, 436, 324, 420), 3304, 0),
         'noise6': (6, (344, 474, 310, 134, 34), None, None)}               # numpy default_rng(0).standard_normal
CASES = tuple(TABLE)


@functools.lru_cache(maxsize=None)
def case(name, zeros=False):
    """-> (pos, sdf float32, tets int64, restatement): computed once, shared, never written to.  zeros: the field rounded to a multiple of
    0.25 first, so that some lattice vertices have sdf == 0 exactly"""
    n = TABLE[name][0]
    pos, tets = synth.kuhn_grid(n, raw=True)
    sdf = _field(name, pos)
    if zeros:
        sdf = np.round(sdf * 4) / 4
        assert (sdf == 0).any()
    sdf = sdf.astype(F32)
    ref = restate(pos, sdf, tets)
    for a in (pos, sdf, tets, ref[0], ref[1]):
        a.setflags(write=False)
    return pos, sdf, tets, ref


def flipped(tets):
    """half of the parents with an odd corner permutation: negatively oriented, the same point sets"""
    t = tets.copy()
    for k, perm in enumerate(((1, 0, 2, 3), (0, 1, 3, 2), (0, 2, 1, 3), (3, 1, 2, 0), (2, 1, 0, 3), (0, 3, 2, 1))):
        t[2 * k::12] = t[2 * k::12][:, perm]
    return t


# ---- geometric checks, from the returned tensors alone ------------------------------------------------------------------------------------
def oriented_faces(t):
    """the four faces of every tet, wound outward for a positively oriented tet"""
    return np.concatenate([t[:, [0, 2, 1]], t[:, [0, 1, 3]], t[:, [0, 3, 2]], t[:, [1, 2, 3]]])


def boundary(t):
    """item 3, first half: every triangle in one or two tets, the two uses of a shared one wound oppositely -> the once-used ones, oriented"""
    f = oriented_faces(t)
    key = np.sort(f, axis=1)
    uniq, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    assert cnt.max(initial=1) <= 2, 'a triangle in more than two tets'
    # parity of the permutation that sorts a face: the two uses of an interior face must differ in it
    par = ((f[:, 0] > f[:, 1]).astype(int) + (f[:, 0] > f[:, 2]) + (f[:, 1] > f[:, 2])) & 1
    tot = np.zeros(len(uniq), int)
    np.add.at(tot, inv, par)
    assert (tot[cnt == 2] == 1).all(), 'two tets on one triangle with the same winding'
    return f[cnt[inv] == 1]


def check_closed_manifold(bf, chi=None):
    """item 3, second half: every edge of the boundary in exactly two triangles; Euler characteristic where the table gives one"""
    if len(bf) == 0:
        return
    e = np.sort(np.concatenate([bf[:, [0, 1]], bf[:, [1, 2]], bf[:, [2, 0]]]), axis=1)
    ue, cnt = np.unique(e, axis=0, return_counts=True)
    assert (cnt == 2).all(), f'boundary edges used {sorted(set(cnt.tolist()))} times'
    if chi is not None:
        assert len(np.unique(bf)) - len(ue) + len(bf) == chi


def volumes(v, t):
    p = v.astype(np.float64)[t]
    return np.einsum('ij,ij->i', np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), p[:, 3] - p[:, 0]) / 6.0


def vol_tol(L, h):
    """A child's volume may be negative by rounding only.  A cut vertex is the float32 value of p0 w0 + p1 w1: two products and a sum, each
    within half an ulp of a number <= L, and weights whose own rounding (two divisions) moves the point along its edge, which is harmless, and
    off it by under an ulp of L -- under 4 ulp = 4 * 2^-23 * L of displacement d off the exact edge in all.  Moving one vertex of a tet by d
    changes its volume by at most d * (area of the opposite face) / 3; a child's faces lie inside a lattice tet, whose faces are smaller than
    h^2 (Kuhn: h^2 / 2 and h^2 / sqrt(2)); at most three vertices of a child are cut vertices: 3 * d * h^2 / 3 = d h^2."""
    return 4 * 2.0 ** -23 * L * h * h


def check_volumes(v, t, bf, L, h):
    """item 4 -> the summed volume"""
    vol = volumes(v, t)
    assert vol.min(initial=0.0) >= -vol_tol(L, h), f'child volume {vol.min()} < -{vol_tol(L, h)}'
    p = v.astype(np.float64)[bf]
    flux = np.einsum('ij,ij->i', np.cross(p[:, 0], p[:, 1]), p[:, 2]) / 6.0
    # Both sums are the same polynomial of the stored positions when the mesh is conforming and consistently wound (interior faces cancel term by
    # term), so they differ by float64 rounding only.  Each of the K = m + |bf| determinants is six products of three factors <= 2 L, every
    # operation within u = 2^-53 relative: under 16 u * 6 (2 L)^3 / 6 = 128 u L^3 each; summing K terms adds at most K u times the sum of
    # their magnitudes.
    K, u = len(t) + len(bf), 2.0 ** -53
    bound = K * u * (128 * L ** 3 + np.abs(vol).sum() + np.abs(flux).sum())
    assert abs(vol.sum() - flux.sum()) <= bound, f'sum of children {vol.sum()} vs enclosed {flux.sum()}: off by more than {bound}'
    return float(vol.sum())


def check_geometry(v, t, L, h, chi=None):
    bf = boundary(t)
    check_closed_manifold(bf, chi)
    return check_volumes(v, t, bf, L, h)


# ---- the checks the two test files run ------------------------------------------------------------------------------------------------------
def _clip(dev, pos, sdf, tets):
    from d3h import tetfill
    v, t, n = tetfill.clip(*(torch.from_numpy(np.array(a)).to(dev) for a in (pos, sdf, tets)))
    assert v.dtype == torch.float32 and t.dtype == torch.int64 and isinstance(n, int) and v.device.type == torch.device(dev).type
    return v.cpu().numpy(), t.cpu().numpy(), n


def _exact(got, ref):
    (v, t, n), (rv, rt, rn, _) = got, ref
    assert n == rn and v.shape == rv.shape and t.shape == rt.shape
    assert np.array_equal(t, rt)
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32))


def check_restatement_counts(name):
    """the restatement itself against the issue's table (no kernel): tets by inside corners, children, and the tolerance of item 4"""
    n, hist, kids, chi = TABLE[name]
    pos, sdf, tets, ref = case(name)
    assert tuple(ref[3]) == hist and len(ref[1]) == np.dot(hist, CHILDREN) and kids in (None, len(ref[1]))
    if name == 'noise6':
        assert len(tets) == 1296 == 5 * 256 + 16
        masks = set(((sdf[tets] <= 0) * (1, 2, 4, 8)).sum(1).tolist())
        assert masks == set(range(16))
    check_geometry(ref[0], ref[1], 1.0, 2.0 / n, chi)


def check_case(dev, name):
    """items 1-4 of the issue for one row of its table"""
    from d3h import mtets
    n, _, _, chi = TABLE[name]
    pos, sdf, tets, ref = case(name)
    v, t, n_in = got = _clip(dev, pos, sdf, tets)
    _exact(got, ref)
    tp, ts, tt = (torch.from_numpy(np.array(a)).to(dev) for a in (pos, sdf, tets))
    wt = mtets.marching_tets(tp, ts, torch.ones_like(ts), tt)['verts_wt'].cpu().numpy()
    assert np.array_equal(v[n_in:].view(np.uint32), wt.view(np.uint32))
    assert np.array_equal(v[:n_in].view(np.uint32), pos[~(sdf > 0)].view(np.uint32))
    check_geometry(v, t, 1.0, 2.0 / n, chi)


def check_flipped(dev, name):
    """item 5: half of the parents negatively oriented -> the same children as point sets, still positively oriented"""
    n, _, _, chi = TABLE[name]
    pos, sdf, tets, ref = case(name)
    ft = flipped(tets)
    assert (volumes(pos, ft) < 0).sum() == len(ft) // 2
    v, t, n_in = got = _clip(dev, pos, sdf, ft)
    _exact(got, restate(pos, sdf, ft))
    assert np.array_equal(v.view(np.uint32), ref[0].view(np.uint32))
    canon = lambda a: np.unique(np.sort(a, axis=1), axis=0)
    assert np.array_equal(canon(t), canon(ref[1]))
    check_geometry(v, t, 1.0, 2.0 / n, chi)


def check_zeros(dev, name):
    """sdf exactly 0 at lattice vertices: they are inside; items 1-3 hold (children of zero volume are allowed)"""
    pos, sdf, tets, ref = case(name, True)
    v, t, n_in = got = _clip(dev, pos, sdf, tets)
    _exact(got, ref)
    assert n_in == int((sdf <= 0).sum())
    check_closed_manifold(boundary(t))


def check_all_outside_all_inside(dev):
    pos, _, tets, _ = case('sphere4')
    v, t, n = _clip(dev, pos, np.ones(len(pos), F32), tets)
    assert v.shape == (0, 3) and t.shape == (0, 4) and n == 0
    v, t, n = _clip(dev, pos, -np.ones(len(pos), F32), tets)
    assert n == len(pos) and np.array_equal(v, pos) and np.array_equal(t, tets)


def soup(T, seed=0):
    """T disjoint tets (4 T vertices), every second one negatively oriented, random signs"""
    rng = np.random.default_rng(seed + T)
    base = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    pos = (base[None] * 0.5 + rng.uniform(-0.05, 0.05, (T, 4, 3)).astype(F32) + np.arange(T, dtype=F32)[:, None, None] % 7).reshape(-1, 3)
    tets = np.arange(4 * T, dtype=np.int64).reshape(T, 4)
    tets[1::2] = tets[1::2][:, [0, 2, 1, 3]]
    return pos.astype(F32), rng.standard_normal(4 * T).astype(F32), tets


def check_soup(dev, T):
    """T = 0, 1 and the sizes round one workgroup: exact integers and positions, positive children"""
    pos, sdf, tets = soup(T)
    v, t, n_in = got = _clip(dev, pos, sdf, tets)
    _exact(got, restate(pos, sdf, tets))
    if T:
        assert volumes(v, t).min(initial=0.0) >= -vol_tol(float(np.abs(pos).max()), 0.6)
    else:
        assert t.shape == (0, 4)


def check_interface(dev):
    """a NaN is a ValueError; int32 and int64 tets, strided positions and an [N,1] field give the same result; bad arguments raise before a launch"""
    from d3h import tetfill
    from d3h import _lib as L
    pos, sdf, tets, ref = case('sphere4')
    tp, ts, tt = (torch.from_numpy(np.array(a)).to(dev) for a in (pos, sdf, tets))
    bad = ts.clone()
    bad[7] = float('nan')
    with pytest.raises(ValueError, match='NaN'):
        tetfill.clip(tp, bad, tt)
    wide = torch.zeros(len(pos), 5, device=dev)
    wide[:, 1:4] = tp
    assert not wide[:, 1:4].is_contiguous()
    for args in ((tp, ts, tt.int()), (wide[:, 1:4], ts, tt), (tp, ts.reshape(-1, 1), tt)):
        v, t, n = tetfill.clip(*args)
        _exact((v.cpu().numpy(), t.cpu().numpy(), n), ref)
    calls = []
    real = L.call
    L.call = lambda *a: (calls.append(a[0]), real(*a))[1]
    try:
        out = tt.clone()
        out[3, 2] = len(pos)
        neg = tt.clone()
        neg[0, 0] = -1
        for args in ((tp, ts, out), (tp, ts, neg), (tp.double(), ts, tt), (tp[:, :2], ts, tt), (tp, ts[:-1], tt), (tp, ts, tt[:, :3]),
                     (tp, ts, tt.float()), (tp, ts.double(), tt)):
            with pytest.raises(RuntimeError, match='clip: '):
                tetfill.clip(*args)
    finally:
        L.call = real
    assert calls == []


def _mesh(name):
    if name == 'icosphere':
        v, f = synth.icosphere(2)
        return (v * 0.6).astype(F32), f, 8
    import handoff_cases as H
    v, f, _ = H.capsule_pieces(16)
    return v.astype(F32), f, 16


def check_fill_mesh(dev, name):
    """fill_mesh on a closed and on a piece-wise open mesh: items 3 and 4, inside vertices have mesh_wsdf <= 0, and the volume is the volume
    watertight.extract's surface encloses at the same res (the same field, the same lattice, the same cut vertices: equal within item 4's bounds,
    see below; the gap to the analytic volume is marching tets' discretisation and is not judged here)"""
    from d3h import tetfill, watertight, meshops
    mv, mf, res = _mesh(name)
    tv, tf = torch.as_tensor(mv, device=dev), torch.as_tensor(mf, device=dev)
    v, t, h = tetfill.fill_mesh(tv, tf, res=res, scale=1.1)
    side = float((mv.max(0) - mv.min(0)).max()) * 1.1
    assert abs(h - side / res) <= 1e-12 * h
    centre = (mv.max(0) + mv.min(0)) * 0.5
    L = float(np.abs(centre).max()) + side / 2
    unit, tets = watertight._lattice(res, tv.device)
    lo, hi = tv.min(0).values, tv.max(0).values
    pos = ((lo + hi) * 0.5 + unit * (side * 0.5)).contiguous()
    field, _ = meshops.mesh_wsdf(pos, tv, tf, want_w=False)
    n_in = int((~(field > 0)).sum())
    vn, tn = v.cpu().numpy(), t.cpu().numpy()
    assert n_in > 0 and np.array_equal(vn[:n_in], pos[~(field > 0)].cpu().numpy())
    inside_field, _ = meshops.mesh_wsdf(v[:n_in].contiguous(), tv, tf, want_w=False)
    assert float(inside_field.max()) <= 0.0
    vol = check_geometry(vn, tn, L, h, 2)
    wv, wf, _, wh = watertight.extract(tv, tf, res=res, scale=1.1)
    assert wh == h
    p = wv.cpu().numpy().astype(np.float64)[wf.cpu().numpy()]
    flux = np.einsum('ij,ij->i', np.cross(p[:, 0], p[:, 1]), p[:, 2]) / 6.0
    # The two surfaces have the same vertices (the cut vertices) and the same cut polygons; they differ where marching tets' triangle table and
    # the prism rule cut a quad along different diagonals.  The solid between the two triangulations of a quad is the tet of its four cut
    # vertices: coplanar in the interpolant, stored within item 4's 4 ulp of that plane, faces under h^2 -- at most vol_tol each, by item 4's
    # argument.  D = the number of such quads, counted from the two face lists; the rest is item 4's float64 bound over both sums.
    mine = set(map(tuple, np.sort(boundary(tn) - n_in, axis=1).tolist()))
    theirs = set(map(tuple, np.sort(wf.cpu().numpy(), axis=1).tolist()))
    assert len(mine) == len(theirs) == len(flux) and len(mine - theirs) == len(theirs - mine) and len(mine - theirs) % 2 == 0
    D = len(mine - theirs) // 2
    K, u = len(tn) + 2 * len(flux), 2.0 ** -53
    gap, bound = abs(flux.sum() - vol), D * vol_tol(L, h) + K * u * (128 * L ** 3 + 2 * np.abs(flux).sum() + np.abs(volumes(vn, tn)).sum())
    print(f'fill_mesh[{name}]: volume {vol}, watertight surface {flux.sum()}, gap {gap}, bound {bound} ({D} quads cut the other way)')
    assert gap <= bound


def check_get_tet_mesh(dev, tmp_path):
    """script/get_tet_smpl.py: the reference's return and files"""
    from script import get_tet_smpl as G
    from script import connet_face_head as CF
    mv, mf, res = _mesh('icosphere')
    obj = str(tmp_path / 'template.obj')
    CF.write_pc(obj, mv, f=mf)
    npz = str(tmp_path / 'template_tet_8.npz')
    v, t = G.get_tet_mesh(obj, npz, res, 1.1)
    assert isinstance(v, np.ndarray) and v.dtype == np.float32 and v.ndim == 2 and v.shape[1] == 3
    assert isinstance(t, np.ndarray) and t.dtype.kind == 'i' and t.ndim == 2 and t.shape[1] == 4 and len(t) > 0 and t.max() == len(v) - 1
    z = np.load(npz)
    assert sorted(z.files) == ['f', 'v'] and np.array_equal(z['v'], v) and np.array_equal(z['f'], t) and z['v'].dtype == np.float32
    rv, rt = [], []
    for line in open(npz.replace('npz', 'obj')):
        tok = line.split()
        (rv if tok[0] == 'v' else rt).append(tok[1:])
        assert tok[0] in ('v', 'f') and (tok[0] == 'v' or rv) and (tok[0] == 'f' or not rt)
    assert np.array_equal(np.array(rv, np.float32), v) and np.array_equal(np.array(rt, np.int64) - 1, t)
    mv64, mf32 = CF.om_loadmesh(obj)
    from d3h import tetfill
    dv, dt, _ = tetfill.fill_mesh(torch.as_tensor(mv64, device=dev).float(), torch.as_tensor(mf32, device=dev), res=res, scale=1.1)
    assert np.array_equal(dv.cpu().numpy(), v) and np.array_equal(dt.cpu().numpy(), t)
    G.save_tet_mesh_as_obj(v, None, str(tmp_path / 'only_v.obj'))
    assert len(open(tmp_path / 'only_v.obj').read().splitlines()) == len(v)
