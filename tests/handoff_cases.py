"""Check functions of the second half of the stage hand-off -- winding-signed distance and collision push (csrc/mesh_ops.hip), edge-split refinement
and relaxation (csrc/meshrefine.hip, d3h/meshrefine.py), watertight extraction (d3h/watertight.py) -- shared by tests/test_handoff_emul.py (host
emulation of the kernel sources) and tests/test_gpu_handoff.py (MI355X).  Same shapes on both.  Every mesh is generated here from a seed.

Yardsticks:
  mesh_wsdf   numpy over all (query, triangle) pairs: closest point by Ericson's region test, solid angle by van Oosterom-Strackee, once in float64
              and once in float32.  PARITY RULE (the project's): a result is within max(5 x the float32 yardstick's own error against float64, 2^-20)
              of the float64 yardstick; the own error is taken per query group (random points / points ON the mesh, where the solid angle of the
              triangles the point lies on is undetermined in any precision), so that the second group does not widen the bar of the first.
  refine      a sequential Python restatement of the docstring of d3h.meshrefine in numpy float32 scalars, same operation order: EXACT equality of
              vertices, faces and parent.  Every case asserts that no comparison its yardstick makes (squared edge length against threshold^2, one
              diagonal against the other) is closer than 1e-5 relative, unless it is an exact tie.
  relax       float64 Jacobi rounds over Python adjacency sets.
The emulator runs the threads of a launch one after another, so it cannot show a race: the book and fan cases count on the GPU."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from d3h import _lib as L
from d3h import meshops as MO
from d3h import meshrefine as MR
from d3h import meshtopo as MT
from d3h import watertight as WT

FLOOR = 2.0 ** -20


# ---- mesh generators ------------------------------------------------------------------------------------------------------------------------
def cube():
    v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float64)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]          # outward
    f = np.array([t for a, b, c, d in q for t in ((a, b, c), (a, c, d))], np.int64)
    return v, f


def tetrahedron():
    v = np.array([[0.6, 0.6, 0.6], [0.6, -0.6, -0.6], [-0.6, 0.6, -0.6], [-0.6, -0.6, 0.6]], np.float64)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64)
    return v, f


def cylinder(radius=0.5, height=1.0, nu=32, nz=8, z0=None):
    """open cylinder round the z axis, nu x nz quads, no caps, wound outward"""
    z0 = -height / 2 if z0 is None else z0
    ang = 2 * np.pi * np.arange(nu) / nu
    v = np.array([[radius * np.cos(a), radius * np.sin(a), z0 + height * k / nz] for k in range(nz + 1) for a in ang], np.float64)
    f = []
    for k in range(nz):
        for i in range(nu):
            a, b = k * nu + i, k * nu + (i + 1) % nu
            f += [(a, b, b + nu), (a, b + nu, a + nu)]
    return v, np.array(f, np.int64)


def capsule_pieces(res=32):
    """a capsule round the z axis (radius 0.25, cylinder part |z| <= 0.35) as a lat-long mesh cut into three pieces by removing two bands of rings about
    two cells of a res-lattice wide; -> (v, f, h) with h the lattice pitch watertight() will use at scale 1.1"""
    r, half, nu = 0.25, 0.35, 32
    side = 1.1 * (2 * half + 2 * r)
    h = side / res
    zs = [-half - r * math.cos(t) for t in np.linspace(0, np.pi / 2, 9)[1:-1]] + list(np.linspace(-half, half, 29)) + \
        [half + r * math.sin(t) for t in np.linspace(0, np.pi / 2, 9)[1:-1]]
    rad = lambda z: r if abs(z) <= half else math.sqrt(max(r * r - (abs(z) - half) ** 2, 0.0))
    v = [[0.0, 0.0, -half - r]]
    for z in zs:
        v += [[rad(z) * math.cos(2 * np.pi * i / nu), rad(z) * math.sin(2 * np.pi * i / nu), z] for i in range(nu)]
    v.append([0.0, 0.0, half + r])
    top = len(v) - 1
    f = [(0, 1 + (i + 1) % nu, 1 + i) for i in range(nu)]
    gaps = []
    for k in range(len(zs) - 1):
        zm = 0.5 * (zs[k] + zs[k + 1])
        if any(abs(zm - c) < h for c in (-0.12, 0.17)):                       # a removed band: 2 h wide
            gaps.append(k)
            continue
        for i in range(nu):
            a, b = 1 + k * nu + i, 1 + k * nu + (i + 1) % nu
            f += [(a, b, b + nu), (a, b + nu, a + nu)]
    base = 1 + (len(zs) - 1) * nu
    f += [(base + i, base + (i + 1) % nu, top) for i in range(nu)]
    assert gaps
    return np.array(v, np.float64), np.array(f, np.int64), h


def sheet(n, m, seed=None, jitter=0.3, pitch=1.0):
    """n x m cells in the xy plane, two triangles each (z jittered too when seeded), vertex (i, j) at index i (m + 1) + j"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(m + 1), indexing='ij')
    v = np.stack([i.reshape(-1), j.reshape(-1), np.zeros(i.size)], 1).astype(np.float64)
    if seed is not None:
        v += np.random.default_rng(seed).uniform(-jitter, jitter, v.shape)
    a = (i[:-1, :-1] * (m + 1) + j[:-1, :-1]).reshape(-1)
    f = np.stack([np.stack([a, a + m + 1, a + m + 2], 1), np.stack([a, a + m + 2, a + 1], 1)], 1).reshape(-1, 3).astype(np.int64)
    return v * pitch, f


def strip(k, seed):
    """k triangles in a zig-zag strip, jittered"""
    v = np.array([[0.5 * i, float(i & 1), 0.0] for i in range(k + 2)]) + np.random.default_rng(seed).uniform(-0.2, 0.2, (k + 2, 3))
    f = np.array([(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(k)], np.int64)
    return v, f


def book(k, seed):
    """k faces that all share the edge (0, 1): every thread of the launch inserts the same key"""
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = rng.uniform(0.6, 1.6, k)
    v = np.concatenate([[[0, 0, -0.5], [0, 0, 0.5]], np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-0.3, 0.3, k)], 1)])
    return v, np.stack([np.zeros(k, np.int64), np.ones(k, np.int64), np.arange(k) + 2], 1)


def fan(k, seed):
    """k triangles round one hub (index 0): the hub's spokes are shared pairwise, all inserted at once"""
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 1.7 * np.pi, k + 1)
    rad = rng.uniform(0.7, 1.4, k + 1)
    v = np.concatenate([[[0, 0, 0]], np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-0.1, 0.1, k + 1)], 1)])
    r = np.arange(k, dtype=np.int64)
    return v, np.stack([np.zeros(k, np.int64), r + 1, r + 2], 1)


# ---- mesh_wsdf ------------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _tri_dist2(p, A, B, C):
    """squared distance of points p to triangles (A, B, C), broadcast over the leading axes, in the arrays' type: Ericson's region test"""
    one = p.dtype.type(1)
    ab, ac, ap = B - A, C - A, p - A
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - B
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - C
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all='ignore'):
        t_ab = d1 / (d1 - d3)
        t_ac = d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = one / (va + vb + vc)
    sq = lambda q: _dot(q, q)
    cand = [((d1 <= 0) & (d2 <= 0), sq(ap)), ((d3 >= 0) & (d4 <= d3), sq(bp)),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), sq(ap - ab * t_ab[..., None])), ((d6 >= 0) & (d5 <= d6), sq(cp)),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), sq(ap - ac * t_ac[..., None])),
            ((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), sq(bp - (C - B) * t_bc[..., None]))]
    inner = sq(ap - ab * (vb * den)[..., None] - ac * (vc * den)[..., None])
    return np.select([c for c, _ in cand], [x for _, x in cand], inner)


def wsdf_yardstick(points, v, f, dtype):
    """-> (w in turns, distance), both float64 arrays computed in `dtype` over all (query, triangle) pairs"""
    p_all, v = np.asarray(points, dtype), np.asarray(v, dtype)
    A, B, C = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    ws, ds = [], []
    two = dtype(2)
    sq = lambda q: _dot(q, q)
    for s in range(0, len(p_all), 256):
        p = p_all[s:s + 256, None, :]
        ds.append(np.sqrt(_tri_dist2(p, A, B, C).min(1)))
        ra, rb, rc = A - p, B - p, C - p
        la, lb, lc = np.sqrt(sq(ra)), np.sqrt(sq(rb)), np.sqrt(sq(rc))
        det = _dot(ra, np.cross(rb, rc))
        dn = la * lb * lc + _dot(ra, rb) * lc + _dot(ra, rc) * lb + _dot(rb, rc) * la
        ws.append((two * np.arctan2(det, dn)).sum(1, dtype=dtype) / dtype(4 * np.pi))
    return np.concatenate(ws).astype(np.float64), np.concatenate(ds).astype(np.float64)


def dist_upper_bound(points, v, f, k=16):
    """float64 distance of every point to the nearest of the k triangles whose centroids are nearest to it: never below the distance to the mesh, so
    `bound <= x` proves `distance <= x` at a fraction of the pairs"""
    p_all, v = np.asarray(points, np.float64), np.asarray(v, np.float64)
    cen = v[f].mean(1)
    k = min(k, len(f))
    out = []
    for s in range(0, len(p_all), 1024):
        p = p_all[s:s + 1024]
        near = np.argpartition(((p[:, None] - cen[None]) ** 2).sum(2), k - 1, axis=1)[:, :k]
        t = f[near]
        out.append(np.sqrt(_tri_dist2(p[:, None], v[t[..., 0]], v[t[..., 1]], v[t[..., 2]]).min(1)))
    return np.concatenate(out)


def wsdf_queries(v, f):
    rnd = np.random.default_rng(0).uniform(-1, 1, (4000, 3))
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
    on = np.concatenate([v, 0.5 * (v[e[:, 0]] + v[e[:, 1]])])
    q = np.concatenate([rnd, on]).astype(np.float32)
    return q, np.arange(len(q)) < len(rnd)


WSDF_MESHES = {'cube': cube, 'tetrahedron': tetrahedron, 'cylinder': cylinder}


@functools.lru_cache(None)
def wsdf_reference(name):
    v, f = WSDF_MESHES[name]()
    v = v.astype(np.float32)
    q, is_rnd = wsdf_queries(v.astype(np.float64), f)
    w64, d64 = wsdf_yardstick(q, v, f, np.float64)
    w32, d32 = wsdf_yardstick(q, v, f, np.float32)
    return v, f, q, is_rnd, w64, d64, w32, d32


def _bar(own):
    return max(5.0 * float(own), FLOOR)


def check_wsdf(dev, name):
    v, f, q, is_rnd, w64, d64, w32, d32 = wsdf_reference(name)
    T = lambda a, dt=None: torch.as_tensor(a, dtype=dt, device=dev)
    sdf, w = MO.mesh_wsdf(T(q), T(v), T(f))
    sdf, w = sdf.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64)
    for grp, sel in (('random', is_rnd), ('on the mesh', ~is_rnd)):
        ew, bw = np.abs(w - w64)[sel].max(), _bar(np.abs(w32 - w64)[sel].max())
        ed, bd = np.abs(np.abs(sdf) - d64)[sel].max(), _bar(np.abs(d32 - d64)[sel].max())
        print(f'mesh_wsdf {name} / {grp}: |dw| {ew:.3e} (bar {bw:.3e})  |ddist| {ed:.3e} (bar {bd:.3e})')
        assert ew <= bw, (name, grp, ew, bw)
        assert ed <= bd, (name, grp, ed, bd)
    if name != 'cylinder':                                                     # a closed mesh: mesh_sdf, bit for bit
        ref = MO.mesh_sdf(T(q), T(v), T(f)).cpu().numpy()
        assert np.array_equal(ref.view(np.uint32), sdf.astype(np.float32).view(np.uint32))


def check_wsdf_sign(dev, name):
    """the sign of sdf equals that of the float64 yardstick at EVERY query (random points, the mesh's own vertices and edge midpoints) whose float64
    | |w| - 0.5 | >= 1e-4; at most 0.5 % of the queries may be excluded.

    The on-mesh queries are why mesh_wsdf evaluates a triangle in float64 when the query lies in its plane to within rounding: in float32 alone 130 of the
    open cylinder's 1088 on-mesh queries took the other sign (the solid angle of a triangle seen from a point of its own edge is atan2 of two rounding
    residues, and the float32 and float64 winding numbers differed by up to a whole turn there)."""
    v, f, q, is_rnd, w64, d64, w32, d32 = wsdf_reference(name)
    T = lambda a: torch.as_tensor(a, device=dev)
    sdf = MO.mesh_wsdf(T(q), T(v), T(f), want_w=False)[0].cpu().numpy()
    clear = np.abs(np.abs(w64) - 0.5) >= 1e-4
    want = np.where(np.abs(w64) > 0.5, -1.0, 1.0)
    got = np.where(np.signbit(sdf), -1.0, 1.0)
    bad = clear & (got != want)
    print(f'mesh_wsdf {name}: {int((~clear).sum())} of {len(q)} queries within 1e-4 of |w| = 0.5; sign differs at {int(bad.sum())} '
          f'({int((bad & is_rnd).sum())} random, {int((bad & ~is_rnd).sum())} on the mesh, float64 distance there at most {d64[bad].max() if bad.any() else 0:.1e})')
    assert (~clear).mean() <= 0.005
    assert not bad.any(), np.nonzero(bad)[0][:10]


def check_wsdf_tile_and_block_edges(dev):
    """1023 / 1024 / 1025 faces (the LDS tile of 1024) x 255 / 256 / 257 queries (the block of 256)"""
    v, f = sheet(16, 33, seed=5, jitter=0.2, pitch=0.05)
    v = (v - v.mean(0)).astype(np.float32)
    q = np.random.default_rng(1).uniform(-1, 1, (257, 3)).astype(np.float32)
    T = lambda a: torch.as_tensor(a, device=dev)
    for nf in (1023, 1024, 1025):
        w64, d64 = wsdf_yardstick(q, v, f[:nf], np.float64)
        w32, d32 = wsdf_yardstick(q, v, f[:nf], np.float32)
        for nq in (255, 256, 257):
            sdf, w = MO.mesh_wsdf(T(q[:nq]), T(v), T(f[:nf]))
            sdf, w = sdf.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64)
            assert np.abs(w - w64[:nq]).max() <= _bar(np.abs(w32 - w64).max()), (nf, nq)
            assert np.abs(np.abs(sdf) - d64[:nq]).max() <= _bar(np.abs(d32 - d64).max()), (nf, nq)
    # the 1025th face matters: it is the only one near this point
    c = v[f[1024]].mean(0)
    sdf, _ = MO.mesh_wsdf(T((c + np.float32([0, 0, 1e-3]))[None]), T(v), T(f[1024:1025]))
    full, _ = MO.mesh_wsdf(T((c + np.float32([0, 0, 1e-3]))[None]), T(v), T(f[:1025]))
    assert abs(float(full.abs()) - float(sdf.abs())) <= FLOOR


def check_wsdf_edges_of_the_interface(dev):
    v, f = cube()
    T = lambda a: torch.as_tensor(a, device=dev)
    vt, ft = T(v.astype(np.float32)), T(f)
    q = T(np.random.default_rng(2).uniform(-1, 1, (300, 3)).astype(np.float32))
    sdf, w = MO.mesh_wsdf(q, vt, ft)
    s_only, none = MO.mesh_wsdf(q, vt, ft, want_w=False)                       # NULL output pointers
    assert none is None and torch.equal(s_only, sdf)
    none, w_only = MO.mesh_wsdf(q, vt, ft, want_sdf=False)
    assert none is None and torch.equal(w_only, w)
    assert MO.mesh_wsdf(q, vt, ft, want_sdf=False, want_w=False) == (None, None)
    s0, w0 = MO.mesh_wsdf(q[:0], vt, ft)                                       # zero queries
    assert s0.shape == (0,) and w0.shape == (0,)
    lib, f32 = L.lib(), ft.int().contiguous()
    args = lambda **k: [k.get('pts', L.ptr(q)), L.i32(k.get('np', 300)), k.get('v', L.ptr(vt)), k.get('f', L.ptr(f32)), L.i32(k.get('nf', 12)), L.ptr(sdf), L.ptr(w),
                        L.stream()]
    for bad in (dict(nf=0), dict(nf=-1), dict(np=-1), dict(pts=None), dict(v=None), dict(f=None)):
        assert lib.d3h_mesh_wsdf(*args(**bad)) == -1, bad
    L._keepalive.clear()
    with pytest.raises(RuntimeError):
        MO.mesh_wsdf(q, vt, ft[:0])
    with pytest.raises(RuntimeError):
        MO.mesh_wsdf(q, vt, ft + 3)                                            # an index past the vertices


# ---- collision push ---------------------------------------------------------------------------------------------------------------------------
def push_inputs():
    """300 vertices with radial normals at radii 0.498 + 0.005 (m + u), m in -3..4, u in [0.1, 0.9]: with the analytic sphere sdf_in = 0.5 - |x| and the
    margin 0.002 no vertex ever comes within 5e-4 of the decision boundary (asserted)"""
    rng = np.random.default_rng(7)
    d = rng.normal(size=(300, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    m, u = rng.integers(-3, 5, 300), rng.uniform(0.1, 0.9, 300)
    r = 0.498 + 0.005 * (m + u)
    k = np.arange(0, 12)[None]
    assert np.abs((r[:, None] - 0.005 * k) - 0.498).min() >= 5e-4
    return (d * r[:, None]).astype(np.float32), (d * rng.uniform(0.5, 2.0, (300, 1))).astype(np.float32), np.maximum(m + 1, 0)


def inside_inputs():
    """200 points at radii 0.3 .. 0.7, none within 5e-4 of the radius 0.502 at which find_inside_point decides; every second one is a body vertex"""
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(200, 3))
    r = rng.uniform(0.3, 0.7, 200)
    r = np.where(np.abs(r - 0.502) < 1e-3, r + 2e-3, r)
    return pts * (r / np.linalg.norm(pts, axis=1))[:, None], np.arange(0, 200, 2)


def label_inputs():
    """two small meshes for merge_meshes_with_face_labels, and the vertex list of face_in_bbox on the first"""
    v, f = sheet(6, 5, seed=3, jitter=0.2)
    return (v, f), (v[:10] + 1.0, f[:3] % 10), np.arange(20)


@functools.lru_cache(None)
def msdfcut_gold():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'msdfcut.npz')))


def check_push(dev):
    v, n, want_pushes = push_inputs()
    field = lambda x: 0.5 - x.norm(dim=1)
    out, pushes = MO.collision_push(torch.as_tensor(v, device=dev), torch.as_tensor(n, device=dev), field, eps=0.005, margin=0.002, rounds=100)
    assert np.array_equal(pushes.cpu().numpy(), want_pushes)
    x = v.astype(np.float64)
    nn = n.astype(np.float64)
    x32 = v.copy()
    for _ in range(100):                                                       # the reference's sweep, float64 and float32
        s = 0.5 - np.linalg.norm(x, axis=1)
        x[s < 0.002] -= (nn / (np.linalg.norm(nn, axis=1, keepdims=True) + 1e-7))[s < 0.002] * 0.005
        s32 = np.float32(0.5) - np.linalg.norm(x32, axis=1)
        x32[s32 < np.float32(0.002)] -= ((n / (np.linalg.norm(n, axis=1, keepdims=True) + np.float32(1e-7))) * np.float32(0.005))[s32 < np.float32(0.002)]
    err, bar = np.abs(out.cpu().numpy() - x).max(), _bar(np.abs(x32 - x).max())
    print(f'collision_push: |dx| {err:.3e} (bar {bar:.3e})')
    assert err <= bar
    still, p0 = MO.collision_push(out, torch.as_tensor(n, device=dev), field)  # nothing left to push: the input, bit for bit, after one round
    assert torch.equal(still, out) and int(p0.sum()) == 0
    lib, t = L.lib(), torch.zeros(4, 3, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    assert lib.d3h_collision_push(L.ptr(t), L.ptr(t), L.ptr(t), L.i32(-1), L.f32(0), L.f32(0), L.ptr(cnt), None, L.stream()) == -1
    assert lib.d3h_collision_push(L.ptr(t), L.ptr(t), L.ptr(t), L.i32(4), L.f32(0), L.f32(0), None, None, L.stream()) == -1
    assert lib.d3h_collision_push(None, L.ptr(t), L.ptr(t), L.i32(4), L.f32(0), L.f32(0), L.ptr(cnt), None, L.stream()) == -1
    L._keepalive.clear()


# ---- refine_long_edges ------------------------------------------------------------------------------------------------------------------------
def _d2(p, q):
    dx, dy, dz = q[0] - p[0], q[1] - p[1], q[2] - p[2]                         # numpy float32 scalars: one rounding per operation
    return (dx * dx + dy * dy) + dz * dz


def _margin(x, y, note):
    x, y = float(x), float(y)
    if x != y:
        note.append(abs(x - y) / max(x, y, 1e-300))


def refine_yardstick(v, faces, threshold, iterations=1, face_mask=None):
    """-> (v float32, faces, parent, margins): the docstring of d3h.meshrefine.refine_long_edges, one face at a time"""
    v = [np.asarray(r, np.float32) for r in np.asarray(v, np.float32)]
    faces = [tuple(int(i) for i in r) for r in np.asarray(faces).reshape(-1, 3)]
    parent = list(range(len(faces)))
    mask = None if face_mask is None else [bool(b) for b in face_mask]
    thr2 = np.float32(threshold) * np.float32(threshold)
    margins = []
    for _ in range(int(iterations)):
        n, marked = len(v), set()
        for fi, (a, b, c) in enumerate(faces):
            for x, y in ((a, b), (b, c), (c, a)):
                lo, hi = min(x, y), max(x, y)
                if lo == hi:
                    continue
                d = _d2(v[lo], v[hi])
                _margin(d, thr2, margins)
                if d > thr2 and (mask is None or mask[fi]):
                    marked.add((lo, hi))
        if not marked:
            break
        rank = {e: n + r for r, e in enumerate(sorted(marked))}
        v = v + [(v[lo] + v[hi]) * np.float32(0.5) for lo, hi in sorted(marked)]
        out, par, msk = [], [], []
        for fi, i in enumerate(faces):
            m = [rank.get((min(i[j], i[(j + 1) % 3]), max(i[j], i[(j + 1) % 3]))) if i[j] != i[(j + 1) % 3] else None for j in range(3)]
            k = sum(x is not None for x in m)
            if k == 0:
                kids = [i]
            elif k == 3:
                kids = [(i[0], m[0], m[2]), (m[0], i[1], m[1]), (m[2], m[1], i[2]), (m[0], m[1], m[2])]
            elif k == 1:
                j = [x is not None for x in m].index(True)
                a, b, c = i[j], i[(j + 1) % 3], i[(j + 2) % 3]
                kids = [(a, m[j], c), (m[j], b, c)]
            else:
                j = [x is None for x in m].index(True)
                a, b, c, p, q = i[j], i[(j + 1) % 3], i[(j + 2) % 3], m[(j + 1) % 3], m[(j + 2) % 3]
                dap, dbq = _d2(v[a], v[p]), _d2(v[b], v[q])
                _margin(dap, dbq, margins)
                first = dap < dbq or (not dbq < dap and a < b)
                kids = [(p, c, q)] + ([(a, b, p), (a, p, q)] if first else [(a, b, q), (b, p, q)])
            out += kids
            par += [parent[fi]] * len(kids)
            if mask is not None:
                msk += [mask[fi]] * len(kids)
        faces, parent, mask = out, par, (msk if mask is not None else None)
    return np.array(v, np.float32).reshape(-1, 3), np.array(faces, np.int64).reshape(-1, 3), np.array(parent, np.int64), margins


def _refine(dev, v, f, thr, iterations=1, mask=None, dtype=torch.int64):
    out = MR.refine_long_edges(torch.as_tensor(np.asarray(v, np.float32), device=dev), torch.as_tensor(np.asarray(f), dtype=dtype, device=dev).reshape(-1, 3),
                               thr, iterations, None if mask is None else torch.as_tensor(np.asarray(mask), dtype=torch.bool, device=dev))
    assert out[1].dtype == dtype and out[2].dtype == torch.int64
    return out[0].cpu().numpy(), out[1].cpu().numpy().astype(np.int64), out[2].cpu().numpy()


def _equal_yardstick(dev, v, f, thr, iterations=1, mask=None, dtype=torch.int64):
    yv, yf, yp, margins = refine_yardstick(v, f, thr, iterations, mask)
    assert not margins or min(margins) >= 1e-5, f'a comparison of this case is within {min(margins):.2e} relative: choose another seed'
    gv, gf, gp = _refine(dev, v, f, thr, iterations, mask, dtype)
    assert gf.shape == yf.shape and np.array_equal(gf, yf)
    assert np.array_equal(gp, yp)
    assert gv.shape == yv.shape and np.array_equal(gv.view(np.uint32), yv.view(np.uint32))
    return gv, gf, gp


def _area(v, f):
    v = np.asarray(v, np.float64)
    return 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum()


def _edges(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    return np.unique(e, axis=0, return_counts=True)


def _euler(f):
    return len(np.unique(f)) - len(_edges(f)[0]) + len(f)


def _open_vertex_set(f):
    e, c = _edges(f)
    return set(np.unique(e[c == 1]).tolist())


def _max_edge(v, f):
    e = _edges(f)[0]
    return np.linalg.norm(np.asarray(v, np.float64)[e[:, 0]] - np.asarray(v, np.float64)[e[:, 1]], axis=1).max()


def check_properties(v0, f0, v1, f1, parent, thr=None, rounds=None):
    """what holds whatever the child table is"""
    assert abs(_area(v1, f1) - _area(v0, f0)) <= 1e-6 * _area(v0, f0)
    assert _euler(f1) == _euler(f0)
    assert np.all(np.diff(parent) >= 0) and (len(f0) == 0 or (parent[0] == 0 and parent[-1] == len(f0) - 1))
    n = len(v0)
    assert np.array_equal(np.asarray(v1[:n], np.float32), np.asarray(v0, np.float32))
    # open vertices: the old ones plus the midpoints of split boundary edges (an old vertex cannot appear or vanish as an open one)
    o0, o1 = _open_vertex_set(f0), _open_vertex_set(f1)
    assert {i for i in o1 if i < n} == o0
    # ... whatever the number of rounds: every split of a boundary edge adds one open vertex and one boundary edge, and a midpoint of midpoints
    # still lies ON the boundary edge of the input it came from (float64 distance to the nearest one, against the float32 rounding of three halvings)
    e0, c0 = _edges(f0)
    e1, c1 = _edges(f1)
    new_open = np.array(sorted(i for i in o1 if i >= n), np.int64)
    assert len(new_open) == int((c1 == 1).sum()) - int((c0 == 1).sum())
    if len(new_open):
        a, b = np.float64(v0)[e0[c0 == 1][:, 0]][None], np.float64(v0)[e0[c0 == 1][:, 1]][None]
        p = np.float64(v1)[new_open][:, None]
        t = np.clip(((p - a) * (b - a)).sum(2) / np.maximum(((b - a) ** 2).sum(2), 1e-300), 0.0, 1.0)
        dist = np.sqrt(((p - (a + t[..., None] * (b - a))) ** 2).sum(2)).min(1)
        assert dist.max() <= 1e-6 * max(np.abs(v0).max(), 1.0), dist.max()
        if rounds == 1:                                                        # one round: exactly the midpoints
            mids = 0.5 * (a[0] + b[0])
            assert np.abs(p - mids[None]).max(2).min(1).max() <= 1e-6 * max(np.abs(v0).max(), 1.0)
    if thr is not None and rounds is not None and rounds >= math.ceil(math.log2(max(_max_edge(v0, f0) / thr, 1.0))):
        assert _max_edge(v1, f1) <= thr * (1 + 1e-6)


def check_refine_single_triangle_patterns(dev):
    """one triangle, each of the 8 marking patterns, in all three rotations: edge lengths 1 (short) and 3.x (long) against the threshold 2"""
    seen = set()
    for pattern in range(8):
        # side lengths: a triangle with sides la, lb, lc where long = marked; built from three chosen lengths that satisfy the triangle inequality
        L3 = [3.0 + 0.1 * j if pattern >> j & 1 else 1.7 - 0.1 * j for j in range(3)]
        la, lb, lc = L3                                                        # |p0 p1|, |p1 p2|, |p2 p0|
        x = (la * la + lc * lc - lb * lb) / (2 * la)
        p = np.array([[0, 0, 0], [la, 0, 0], [x, math.sqrt(max(lc * lc - x * x, 0.0)), 0]]) + 0.125
        for rot in range(3):
            f = np.array([[rot % 3, (rot + 1) % 3, (rot + 2) % 3]])
            gv, gf, gp = _equal_yardstick(dev, p, f, 2.0)
            k = bin(pattern).count('1')
            assert len(gf) == k + 1 and len(gv) == 3 + k
            check_properties(p, f, gv, gf, gp, 2.0, 1)
            seen.add((pattern, rot))
    assert len(seen) == 24


def check_refine_small_cases(dev):
    # two triangles sharing a marked edge: one new vertex for both
    v = np.array([[0, 0, 0], [3, 0, 0], [1.4, 1.1, 0], [1.6, -1.2, 0.1]])
    f = np.array([[0, 1, 2], [1, 0, 3]])
    gv, gf, gp = _equal_yardstick(dev, v, f, 2.5)
    assert len(gv) == 5 and len(gf) == 4 and (gf == 4).sum() == 4
    # an edge shared by three faces
    v3 = np.concatenate([v, [[1.5, 0.2, 1.3]]])
    f3 = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]])
    gv, gf, gp = _equal_yardstick(dev, v3, f3, 2.5)
    assert len(gv) == 6 and len(gf) == 6
    # a face (a, a, b): its edge (a, a) is never marked, its edge (a, b) is there twice
    fa = np.array([[0, 0, 1], [0, 1, 2]])
    gv, gf, gp = _equal_yardstick(dev, v, fa, 2.5)
    assert len(gv) == 5 and len(gf) == 5
    # exact ties of the two diagonals: an isosceles triangle with both legs marked, in both index orders
    iso = np.array([[-1, 0, 0], [1, 0, 0], [0, 4, 0]], np.float64)
    for fi in ([[0, 1, 2]], [[1, 2, 0]], [[2, 0, 1]], [[1, 0, 2]]):
        gv, gf, gp = _equal_yardstick(dev, iso, np.array(fi), 3.0)
        assert len(gf) == 3
    # nothing to do
    for it, thr in ((0, 0.1), (3, 100.0)):
        gv, gf, gp = _refine(dev, v, f, thr, it)
        assert np.array_equal(gv, v.astype(np.float32)) and np.array_equal(gf, f) and np.array_equal(gp, [0, 1])
    gv, gf, gp = _refine(dev, v, np.zeros((0, 3), np.int64), 0.1, 2)
    assert gf.shape == (0, 3) and gp.shape == (0,) and np.array_equal(gv, v.astype(np.float32))


STRIP_SEED, SHEET_SEED, BOOK_SEED, FAN_SEED = 3, 1, 4, 2


def check_refine_strip(dev, dtype):
    v, f = strip(257, STRIP_SEED)
    gv, gf, gp = _equal_yardstick(dev, v, f, 0.9, 2, dtype=dtype)
    check_properties(v, f, gv, gf, gp, 0.9, 2)


@functools.lru_cache(None)
def sheet_case():
    v, f = sheet(40, 40, seed=SHEET_SEED, jitter=0.3, pitch=0.03)
    e = _edges(f)[0]
    thr = float(np.median(np.linalg.norm(v[e[:, 0]] - v[e[:, 1]], axis=1)))
    disc = np.linalg.norm(v[f].mean(1)[:, :2] - v[:, :2].mean(0), axis=1) < 0.3
    return v, f, thr, disc


def check_refine_sheet(dev, masked):
    v, f, thr, disc = sheet_case()
    mask = disc if masked else None
    gv, gf, gp = _equal_yardstick(dev, v, f, thr, 3, mask)
    check_properties(v, f, gv, gf, gp, None if masked else thr, 3)
    if masked:
        assert np.all(np.bincount(gp, minlength=len(f))[~disc & ~np.isin(f, np.unique(f[disc])).any(1)] == 1)    # far from the disc: untouched
        e, c = _edges(gf)
        assert c.max() == 2                                                    # conforming: no T-junction, so no edge gained a third side


def check_refine_contended(dev):
    """many faces inserting one key at once (the book), a hub whose spokes are all inserted at once (the fan)"""
    v, f = book(300, BOOK_SEED)
    gv, gf, gp = _equal_yardstick(dev, v, f, 0.9, 2)
    check_properties(v, f, gv, gf, gp)
    v, f = fan(1000, FAN_SEED)
    gv, gf, gp = _equal_yardstick(dev, v, f, 0.5, 2)
    check_properties(v, f, gv, gf, gp, 0.5, 2)


def check_refine_rejects(dev):
    v, f = strip(10, 1)
    bad = f.copy()
    bad[4, 1] = len(v)
    with pytest.raises(RuntimeError, match='outside'):
        _refine(dev, v, bad, 0.5)
    bad[4, 1] = -1
    with pytest.raises(RuntimeError, match='outside'):
        _refine(dev, v, bad, 0.5)
    T = lambda a, dt: torch.as_tensor(a, dtype=dt, device=dev)
    with pytest.raises(RuntimeError):
        MR.refine_long_edges(T(v, torch.float64), T(f, torch.int64), 0.5)
    with pytest.raises(RuntimeError):
        MR.refine_long_edges(T(v, torch.float32), T(f, torch.int64), -1.0)
    with pytest.raises(RuntimeError):
        MR.refine_long_edges(T(v, torch.float32), T(f, torch.int64), 0.5, face_mask=torch.ones(3, dtype=torch.bool, device=dev))
    lib = L.lib()
    vt, ft = T(v, torch.float32), T(f, torch.int64)
    k = torch.zeros(64, dtype=torch.int64, device=dev)
    c = torch.zeros(64, dtype=torch.int32, device=dev)
    call = lambda **a: lib.d3h_refine_mark(a.get('v', L.ptr(vt)), a.get('f', L.ptr(ft)), L.i32(1), L.i64(a.get('nf', 10)), L.i64(a.get('nv', 12)), None,
                                           L.f32(a.get('thr', 0.5)), a.get('keys', L.ptr(k)), L.ptr(c), L.ptr(c), a.get('err', L.ptr(c)), L.stream())
    for bad_args in (dict(nf=-1), dict(nv=-1), dict(thr=float('nan')), dict(thr=-1.0), dict(v=None), dict(f=None), dict(keys=None), dict(err=None)):
        assert call(**bad_args) == -1, bad_args
    assert lib.d3h_refine_count(None, L.i32(1), L.i64(10), L.i64(12), None, L.i64(0), L.ptr(c), L.ptr(c), L.stream()) == -1
    assert lib.d3h_refine_split(L.ptr(vt), L.ptr(ft), L.i32(1), L.i64(10), L.i64(12), None, L.i64(0), L.ptr(c), None, L.i64(10), L.ptr(vt), L.ptr(ft), L.ptr(c),
                                L.stream()) == -1
    assert lib.d3h_refine_split(L.ptr(vt), L.ptr(ft), L.i32(1), L.i64(10), L.i64(12), None, L.i64(0), L.ptr(c), L.ptr(k), L.i64(9), L.ptr(vt), L.ptr(ft), L.ptr(c),
                                L.stream()) == -1
    L._keepalive.clear()


# ---- relax ------------------------------------------------------------------------------------------------------------------------------------
def relax_yardstick(v, f, free, iterations, dtype=np.float64):
    nbr = [set() for _ in range(len(v))]
    for a, b, c in np.asarray(f).tolist():
        for x, y in ((a, b), (b, c), (c, a)):
            nbr[x].add(y)
            nbr[y].add(x)
    x = np.asarray(v, dtype).copy()
    for _ in range(iterations):
        y = x.copy()
        for i in np.nonzero(free)[0]:
            if nbr[i]:
                y[i] = x[sorted(nbr[i])].sum(0, dtype=dtype) / dtype(len(nbr[i]))
        x = y
    return x


def _relax(dev, v, f, free, it):
    return MR.relax(torch.as_tensor(np.asarray(v, np.float32), device=dev), torch.as_tensor(f, device=dev), torch.as_tensor(free, device=dev), it).cpu().numpy()


def check_relax(dev):
    sv, sf = sheet(12, 9, seed=8, jitter=0.3, pitch=0.1)
    tv, tf = tetrahedron()
    rng = np.random.default_rng(9)
    for v, f in ((sv, sf), (tv, tf)):
        v = v.astype(np.float32)
        free = rng.uniform(size=len(v)) < 0.6
        free[0] = True
        for it in (1, 2, 32):
            got = _relax(dev, v, f, free, it)
            y64, y32 = relax_yardstick(v, f, free, it), relax_yardstick(v, f, free, it, np.float32)
            err, bar = np.abs(got - y64).max(), _bar(np.abs(y32 - y64).max())
            print(f'relax {len(v)} vertices, {it} rounds: {err:.3e} (bar {bar:.3e})')
            assert err <= bar
            assert np.array_equal(got[~free].view(np.uint32), v[~free].view(np.uint32))           # fixed vertices: bit-unchanged
        none = np.zeros(len(v), bool)
        assert np.array_equal(_relax(dev, v, f, none, 5).view(np.uint32), v.view(np.uint32))       # all fixed: the identity
        assert np.array_equal(_relax(dev, v, f, ~none, 0).view(np.uint32), v.view(np.uint32))
    with pytest.raises(RuntimeError):
        _relax(dev, sv, sf + 200, np.ones(len(sv), bool), 1)
    with pytest.raises(RuntimeError):
        _relax(dev, sv, sf, np.ones(3, bool), 1)


def check_relax_maximum_principle(dev):
    """the boundary of a sheet fixed in the plane z = c, the interior displaced by a staircase of +-h/2: max |z - c| never increases"""
    n, h, c = 14, 0.05, 0.37
    v, f = sheet(n, n, pitch=h)
    i, j = np.divmod(np.arange(len(v)), n + 1)
    inner = (i > 0) & (i < n) & (j > 0) & (j < n)
    v[:, 2] = c
    v[inner, 2] += np.where((i[inner] // 2 + j[inner] // 3) % 2 == 0, 0.5, -0.5) * h
    x = v.astype(np.float32)
    amp = [np.abs(x[:, 2].astype(np.float64) - np.float32(c)).max()]
    for _ in range(40):
        x = _relax(dev, x, f, inner, 1)
        amp.append(np.abs(x[:, 2].astype(np.float64) - np.float32(c)).max())
    assert all(b <= a for a, b in zip(amp, amp[1:])), amp
    assert amp[-1] < 0.5 * amp[0]


# ---- watertight -------------------------------------------------------------------------------------------------------------------------------
def _signed_volume(v, f):
    v = np.asarray(v, np.float64)
    return np.einsum('ij,ij->i', v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0


def check_watertight(dev, name):
    res = 32
    if name == 'cylinder':
        v, f = cylinder()
        h = 1.1 * 1.0 / res
    else:
        v, f, h = capsule_pieces(res)
    v = v.astype(np.float32)
    T = lambda a: torch.as_tensor(a, device=dev)
    seen, relax = [], MR.relax
    WT._mr.relax = lambda *a: (seen.append(a), relax(*a))[1]                    # the surface as it goes into the relaxation (one extraction only)
    try:
        wv, wf, cap = WT.watertight(T(v), T(f), res=res, relax_iters=32)
    finally:
        WT._mr.relax = relax
    (wv0, wf0, cap0, iters), = seen
    assert iters == 32 and torch.equal(wf, wf0) and torch.equal(cap, cap0)
    wv0, wv, wf, cap = wv0.cpu().numpy(), wv.cpu().numpy(), wf.cpu().numpy(), cap.cpu().numpy()
    assert len(MT.open_vertices(T(wf), len(wv))) == 0                          # closed
    e, c = _edges(wf)
    assert np.all(c == 2)
    labels = MT.connected_components(T(wf), len(wv)).cpu().numpy()
    assert len(np.unique(labels[np.unique(wf)])) == 1 and len(np.unique(wf)) == len(wv)
    assert _signed_volume(wv, wf) > 0                                          # wound outward
    d = dist_upper_bound(wv[~cap], v, f)
    assert d.max() <= h / 4 + FLOOR                                            # every non-cap vertex lies within h / 4 of the input
    assert np.array_equal(wv[~cap].view(np.uint32), wv0[~cap].view(np.uint32))
    assert cap.any()
    # every input vertex farther than 2 h from an open boundary has a vertex of the result within 2 h
    ov = np.array(sorted(_open_vertex_set(f)))
    far = np.linalg.norm(v[:, None].astype(np.float64) - v[ov][None], axis=2).min(1) > 2 * h
    near = np.sqrt(((v[far, None].astype(np.float64) - wv[None].astype(np.float64)) ** 2).sum(2)).min(1)
    print(f'watertight {name}: max distance input vertex -> result vertex {near.max() / h:.3f} h; {int(cap.sum())} cap vertices of {len(wv)}')
    assert far.any() and near.max() <= 2 * h
    if name == 'cylinder':                                                     # the two discs: closer to their planes after the relaxation than before
        for z in (-0.5, 0.5):
            sel = cap & (np.abs(wv0[:, 2] - z) < 2 * h)
            before, after = np.abs(wv0[sel, 2] - z), np.abs(wv[sel, 2] - z)
            print(f'watertight cylinder cap z = {z}: rms distance to the plane {np.sqrt((before ** 2).mean()) / h:.3f} h -> {np.sqrt((after ** 2).mean()) / h:.3f} h')
            assert sel.sum() > 20 and np.sqrt((after ** 2).mean()) < np.sqrt((before ** 2).mean()) and after.max() <= before.max() + FLOOR


# ---- the whole function -----------------------------------------------------------------------------------------------------------------------
def _capsule(nu=32):
    """closed capsule round the z axis, radius 0.25, cylinder part |z| <= 0.35, rings 0.025 apart on the cylinder; -> (v, f, zmid of every face)"""
    r, half = 0.25, 0.35
    zs = [-half - r * math.cos(t) for t in np.linspace(0, np.pi / 2, 9)[1:-1]] + list(np.linspace(-half, half, 29)) + \
        [half + r * math.sin(t) for t in np.linspace(0, np.pi / 2, 9)[1:-1]]
    rad = lambda z: r if abs(z) <= half else math.sqrt(max(r * r - (abs(z) - half) ** 2, 0.0))
    v = [[0.0, 0.0, -half - r]]
    for z in zs:
        v += [[rad(z) * math.cos(2 * np.pi * i / nu), rad(z) * math.sin(2 * np.pi * i / nu), z] for i in range(nu)]
    v.append([0.0, 0.0, half + r])
    f = [(0, 1 + (i + 1) % nu, 1 + i) for i in range(nu)]
    for k in range(len(zs) - 1):
        for i in range(nu):
            a, b = 1 + k * nu + i, 1 + k * nu + (i + 1) % nu
            f += [(a, b, b + nu), (a, b + nu, a + nu)]
    base = 1 + (len(zs) - 1) * nu
    f += [(base + i, base + (i + 1) % nu, len(v) - 1) for i in range(nu)]
    v, f = np.array(v, np.float64), np.array(f, np.int64)
    return v, f, v[f][:, :, 2].mean(1)


def _compact(v, f):
    used = np.unique(f)
    new = np.full(len(v), -1, np.int64)
    new[used] = np.arange(len(used))
    return v[used], new[f]


def write_scenario(root):
    """a capsule as the SMPL stand-in, an open cylindrical shell 0.03 outside its middle as the garment, the capsule's two ends as the visible body
    parts, its covered middle as smpl_cloth, a head box round the upper end; -> the five paths in the order of the function's arguments"""
    from script.connet_face_head import write_pc
    v, f, zm = _capsule()
    paths = [str(root / n) for n in ('body_concat.obj', 'cloth_concat.obj', 'smpl_cloth.obj', 'smpl.obj', 'bbox.npz')]
    write_pc(paths[0], *_compact(v, f[np.abs(zm) > 0.15])[:1], f=_compact(v, f[np.abs(zm) > 0.15])[1])
    gv, gf = cylinder(radius=0.28, height=0.4, nu=32, nz=8)
    write_pc(paths[1], gv, f=gf)
    cv, cf = _compact(v, f[np.abs(zm) < 0.125])
    write_pc(paths[2], cv, f=cf)
    write_pc(paths[3], v, f=f)
    head = v[v[:, 2] > 0.4]
    np.savez(paths[4], bbox_min=head.min(0), bbox_max=head.max(0))
    return paths


def check_whole_function(dev, tmp_path):
    import types
    import script.process_body_cloth_head_msdfcut as PB
    from script.connet_face_head import om_loadmesh
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(MT.__file__)))
    assert os.path.samefile(PB.__file__, os.path.join(pkg, 'script', 'process_body_cloth_head_msdfcut.py')), PB.__file__     # this build's, not the reference's
    src = tmp_path / 'in'
    src.mkdir()
    paths = write_scenario(src)
    root = tmp_path / 'processsplit_cloth0'
    kw = dict(wt_res=32, target_len=0.05, head_threshold=0.02)
    PB.process_body_msdf_distance_bodyedge(None, str(root), *paths, **kw)
    for n in ('merge_body_cloth.obj', 'merge_body_cloth.npz', 'inside_body_index.npz', 'deform_smpl.obj', 'body_edge_cut.obj', 'all_v_f.obj'):
        assert (root / n).exists(), n
    a, b = np.load(root / 'merge_body_cloth.npz'), np.load(root / 'inside_body_index.npz')
    assert sorted(a.files) == ['f', 'face_labels', 'v'] and sorted(b.files) == ['inside_body_index', 'outside_body_index']
    v, f, lab = a['v'], a['f'], a['face_labels']
    assert v.dtype == np.float64 and f.dtype == np.int32 and lab.dtype == np.int64 and b['inside_body_index'].dtype == np.int64
    assert f.min() >= 0 and f.max() < len(v) and len(np.unique(f)) == len(v)
    n0 = int((lab == 0).sum())
    assert 0 < n0 < len(lab) and np.all(lab[:n0] == 0) and np.all(lab[n0:] == 1)                      # 0 then 1
    ov, of = om_loadmesh(str(root / 'merge_body_cloth.obj'))
    assert np.array_equal(of, f) and np.abs(ov - v).max() <= 1e-6
    # label 0: a closed single component
    fb = f[:n0].astype(np.int64)
    nb = int(fb.max()) + 1
    assert np.all(_edges(fb)[1] == 2)
    assert len(np.unique(MT.connected_components(torch.as_tensor(fb, device=dev), nb).cpu().numpy())) == 1
    assert _signed_volume(v[:nb], fb) > 0
    # label 1: exactly refine_long_edges of the garment, two boundary loops
    gv, gf = om_loadmesh(paths[1])
    rv, rf, _ = _refine(dev, gv, gf.astype(np.int64), 4.0 / 3.0 * 0.05, 3)
    assert np.array_equal(f[n0:].astype(np.int64) - nb, rf) and np.array_equal(v[nb:], rv.astype(np.float64))
    e, c = _edges(rf)
    loops = MT.connected_components(torch.as_tensor(np.repeat(e[c == 1], [1], 0)[:, [0, 1, 1]], device=dev), len(rv)).cpu().numpy()
    assert len(np.unique(loops[np.unique(e[c == 1])])) == 2
    # the head box: no edge above head_threshold after head_iterations rounds (three halvings of edges that are at most 4/3 target_len suffice:
    # 0.0667 / 8 < 0.02)
    box = np.load(paths[4])
    inside = np.all((v[:nb] >= box['bbox_min'] - 0.01) & (v[:nb] <= box['bbox_max'] + 0.01), axis=1)
    hf = fb[inside[fb].all(1)]
    assert len(hf) > 100 and _max_edge(v[:nb], hf) <= 0.02 * (1 + 1e-6)
    # inside / outside: a partition of the body's vertices that agrees with a float64 evaluation of the garment field
    ins, out = b['inside_body_index'], b['outside_body_index']
    assert np.array_equal(np.sort(np.concatenate([ins, out])), np.arange(nb)) and len(ins) and len(out)
    w64, d64 = wsdf_yardstick(v[:nb].astype(np.float32), rv, rf, np.float64)
    sdf_in = np.where(np.abs(w64) > 0.5, 1.0, -1.0) * d64                     # pysdf's sign
    sure = np.abs(sdf_in + 0.002) > 1e-5
    assert (~sure).mean() <= 0.005
    got_in = np.zeros(nb, bool)
    got_in[ins] = True
    assert np.array_equal(got_in[sure], (sdf_in > -0.002)[sure])
    # the seq stage's loader takes the directory
    from dataset.dataset_split import Dataset_split, DirectorySource, MemorySource, SMPLX_KEYS, _SMPLX_WIDTH

    class FromDirectory(MemorySource):
        def detail(self, process_path):
            return DirectorySource.detail(self, process_path)
    img, msk = np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.uint8)
    smplx = {k: np.zeros((2, _SMPLX_WIDTH[k]), np.float32) for k in SMPLX_KEYS}
    smplx.update(face_offset=np.zeros((1, 8, 3), np.float32), joint_offset=np.zeros((1, 55, 3), np.float32), locator_offset=np.zeros((1, 55, 3), np.float32),
                 shape_param=np.zeros((1, 100), np.float32))
    cam = {'intrinsic': np.array([[100.0, 0, 4], [0, 100.0, 4], [0, 0, 1]]), 'extrinsic': np.eye(4), 'height': 8, 'width': 8}
    ds = Dataset_split(FromDirectory([(img, msk, msk, msk, img)] * 2, (0, 1), smplx, cam), types.SimpleNamespace(device=dev, train_res=[8, 8]), Detail=True,
                       process_path=str(root))
    assert ds.v.shape == (len(v), 3) and ds.f.shape == f.shape and int(ds.cloth_index.min()) == nb
    assert ds.outside_index.numel() == (len(v) - nb) + len(out)
    # a missing input raises with its path
    for k in range(5):
        gone = list(paths)
        gone[k] = str(src / 'nowhere.obj')
        with pytest.raises(FileNotFoundError, match='nowhere'):
            PB.process_body_msdf_distance_bodyedge(None, str(root), *gone, **kw)


def check_script_functions(dev, tmp_path):
    """the module's functions against the REFERENCE's own results on the same inputs (tests/golden/msdfcut.npz, tools/gen_golden.py msdfcut: its
    deform_body_collision, find_inside_point, merge_meshes_with_face_labels and face_in_bbox with the analytic sphere 0.5 - |x| as sdf_gt_fn): integer
    outputs exactly, positions under the parity rule, the number of pushes per vertex equal; then the device route against the callable route.
    find_open_edges / remove_faces_with_open_vertices are pinned by tests/golden/close_hole.npz (tests/meshtopo_cases.py) through d3h.meshtopo."""
    import script.process_body_cloth_head_msdfcut as PB
    from script.connet_face_head import MergedMesh
    g = msdfcut_gold()
    sphere = lambda x: 0.5 - np.linalg.norm(np.asarray(x, np.float64), axis=1)
    # the inputs on record are the ones this file generates
    pv, pn, _ = push_inputs()
    pts, body_index = inside_inputs()
    (v1, f1), (v2, f2), v_indices = label_inputs()
    for k, a in (('push.v', pv), ('push.n', pn), ('inside.v', pts), ('inside.body_index', body_index), ('labels.v1', v1), ('labels.f1', f1), ('labels.v2', v2),
                 ('labels.f2', f2), ('bbox.v_indices', v_indices)):
        assert np.array_equal(g[k], a), k
    # deform_body_collision, callable route: float64 as the reference
    count = lambda out: np.rint(np.linalg.norm(np.asarray(out, np.float64) - pv, axis=1) / 0.005).astype(int)
    host = PB.deform_body_collision(None, None, pv, pn, sphere)
    assert np.array_equal(count(host), count(g['push.out'])) and count(g['push.out']).max() >= 5
    x32 = pv.copy()
    for _ in range(12):                                                       # the same sweep in float32: the yardstick's own error
        s32 = np.float32(0.5) - np.linalg.norm(x32, axis=1)
        x32[s32 < np.float32(0.002)] -= ((pn / (np.linalg.norm(pn, axis=1, keepdims=True) + np.float32(1e-7))) * np.float32(0.005))[s32 < np.float32(0.002)]
    bar = _bar(np.abs(x32 - g['push.out']).max())
    assert np.abs(host - g['push.out']).max() <= bar
    # ... and the device route with the analytic field
    dev_out, pushes = MO.collision_push(torch.as_tensor(pv, device=dev), torch.as_tensor(pn, device=dev), lambda x: 0.5 - x.norm(dim=1))
    assert np.array_equal(pushes.cpu().numpy(), count(g['push.out']))
    err = np.abs(dev_out.cpu().numpy() - g['push.out']).max()
    print(f'deform_body_collision: device route |dx| {err:.3e}, callable route {np.abs(host - g["push.out"]).max():.3e} (bar {bar:.3e})')
    assert err <= bar and np.abs(dev_out.cpu().numpy() - host).max() <= bar
    # find_inside_point
    ins, out = PB.find_inside_point(pts, body_index, sphere, str(tmp_path))
    assert np.array_equal(ins, g['inside.inside']) and np.array_equal(out, g['inside.outside']) and ins.dtype == g['inside.inside'].dtype
    # merge_meshes_with_face_labels, face_in_bbox
    m, lab, mv, mf = PB.merge_meshes_with_face_labels(MergedMesh(v1, f1), MergedMesh(v2, f2))
    assert np.array_equal(lab, g['labels.labels']) and lab.dtype == g['labels.labels'].dtype
    assert np.array_equal(mf, g['labels.f']) and np.array_equal(mv, g['labels.v']) and np.array_equal(m.triangles, mf)
    fin, fout = PB.face_in_bbox(v_indices, f1)
    assert np.array_equal(fin, g['bbox.in']) and np.array_equal(fout, g['bbox.out'])
    # GarmentField is -mesh_wsdf, on arrays
    cv, cf = cylinder()
    gf = PB.GarmentField(cv, cf)
    q = np.random.default_rng(8).uniform(-1, 1, (100, 3))
    ref = -MO.mesh_wsdf(torch.as_tensor(q.astype(np.float32), device=dev), torch.as_tensor(cv.astype(np.float32), device=dev), torch.as_tensor(cf, device=dev))[0]
    assert np.array_equal(gf(q), ref.cpu().numpy())
