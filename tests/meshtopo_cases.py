"""Check functions of the stage hand-off topology -- connected components, vertex weld, open edges (csrc/meshtopo.hip, d3h/meshtopo.py) and the
drop-in script/connet_face_head.py -- shared by tests/test_meshtopo_emul.py (host emulation of the kernel sources) and tests/test_gpu_meshtopo.py
(MI355X).  Same shapes on both.  Every mesh is generated here from a seed; tests/golden/close_hole.npz holds the upstream project's own results on
the three process_close_hole scenarios and of its two open-edge functions (tools/gen_golden.py close_hole).

Every comparison is EXACT (integers, index lists, float64 box corners, text lines): there is no tolerance anywhere in this file.  The yardsticks:
  components   a sequential union-find in Python whose labels are the smallest vertex index of each component
  weld         a Python dict filled in vertex order; -0 keyed as +0; a row with a NaN is never looked up nor stored
  open edges   torch.unique over the 3F sorted edges with counts, the ends of those counted once
The emulator runs the threads of a launch one after another, so it cannot show a race: the strip, fan and one-point cases count on the GPU."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from d3h import _lib as L
from d3h import meshtopo as MT

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'close_hole.npz')


# ---- mesh generators ------------------------------------------------------------------------------------------------------------------------
def icosahedron():
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]],
                 np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2],
                  [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int64)
    return v, f


def grid(n, m):
    """n x m square cells in the xz plane, two triangles each: (n + 1)(m + 1) vertices, vertex (i, j) at index i (m + 1) + j"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(m + 1), indexing='ij')
    v = np.stack([i.reshape(-1), np.zeros(i.size), j.reshape(-1)], 1).astype(np.float64)
    a = (i[:-1, :-1] * (m + 1) + j[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([a, a + 1, a + m + 2], 1), np.stack([a, a + m + 2, a + m + 1], 1)]).astype(np.int64)
    return v, f


def fan(k):
    """k triangles round one hub; the hub has the LARGEST index (k + 1), the rim runs 0..k"""
    ang = np.linspace(0.0, 1.5 * np.pi, k + 1)
    v = np.concatenate([np.stack([np.cos(ang), np.zeros(k + 1), np.sin(ang)], 1), np.zeros((1, 3))])
    r = np.arange(k, dtype=np.int64)
    return v, np.stack([np.full(k, k + 1, np.int64), r, r + 1], 1)


def place(mesh, scale, offset):
    return mesh[0] * scale + np.asarray(offset, np.float64), mesh[1]


def join(parts, extra_vertices=None):
    vs, fs, base = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    if extra_vertices is not None:
        vs.append(np.asarray(extra_vertices, np.float64))
    return np.concatenate(vs), np.concatenate(fs)


def scramble(v, f, seed):
    """a seeded vertex permutation and face shuffle"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(v))
    v2 = np.empty_like(v)
    v2[perm] = v
    return v2, perm[f][rng.permutation(len(f))]


def mix():
    """components of 16, 12, 12, 12, 9, 9, 6 vertices and 3 isolated vertices, each at a height of its own (mean y at least 0.5 apart)"""
    parts = [place(grid(3, 3), 0.1, (0, 0.0, 0)), place(icosahedron(), 0.1, (1, 2.0, 0)), place(grid(2, 3), 0.1, (2, 0.5, 0)), place(fan(10), 0.3, (3, 1.0, 0)),
             place(grid(2, 2), 0.1, (4, 1.5, 0)), place(grid(2, 2), 0.1, (5, -0.5, 0)), place(grid(1, 2), 0.1, (6, -1.0, 0))]
    return join(parts, [[7, -2.0, 0], [7, -2.5, 0], [7, -3.0, 0]])


def close_hole_scenarios():
    """-> {name: (body_v, body_f, cloth_v, cloth_f, num)}: the inputs of the three process_close_hole scenarios of the golden fixture"""
    out = {}
    bv, bf = scramble(*mix(), seed=11)
    garment = join([place(grid(4, 4), 0.1, (0, 0.3, 2)), place(icosahedron(), 0.1, (1, 2.0, 0)), place(grid(1, 2), 0.1, (6, -1.0, 0))])
    out['a'] = (bv, bf) + scramble(*garment, seed=12) + (5,)              # the garment's icosahedron and strip share their coordinates with the body's
    body = join([place(grid(3, 3), 0.1, (0, 0.0, 0)), place(icosahedron(), 0.1, (1, 1.0, 0))])
    out['b'] = scramble(*body, seed=13) + scramble(*place(grid(4, 4), 0.1, (0, 0.3, 2)), seed=14) + (5,)       # nothing to hand over
    body = join([place(grid(3, 3), 0.1, (0, 0.0, 0)), place(icosahedron(), 0.1, (1, 1.0, 0)), place(grid(2, 2), 0.1, (4, -1.0, 0))])
    gv, gf = join([place(grid(4, 4), 0.1, (0, 0.3, 2)), place(grid(1, 2), 0.1, (6, -1.5, 0))])
    gv[1] = gv[0]                                                          # two vertices of one garment face at identical coordinates
    out['c'] = scramble(*body, seed=15) + scramble(gv, gf, seed=16) + (2,)
    return out


def open_edge_meshes():
    """-> {name: (faces, nv)}: the inputs of the golden's find_open_edges / remove_faces_with_open_vertices records"""
    v, f = scramble(*mix(), seed=21)
    g, gf = scramble(*grid(6, 6), seed=22)
    gf = np.concatenate([gf, [[3, 3, 40], [5, 6, 6]]])                     # faces (a,a,b) and (a,b,b)
    return {'mix': (f, len(v)), 'grid66': (gf, len(g))}


@functools.lru_cache(None)
def gold():
    return dict(np.load(GOLD))


# ---- yardsticks -----------------------------------------------------------------------------------------------------------------------------
def cc_yardstick(faces, nv):
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in np.asarray(faces).reshape(-1, 3).tolist():
        for p, q in ((a, b), (b, c)):
            rp, rq = find(p), find(q)
            if rp != rq:
                parent[max(rp, rq)] = min(rp, rq)
    return np.array([find(x) for x in range(nv)], np.int64).reshape(nv)


def rank_yardstick(labels):
    """the reference's order: components in the order of their first vertex, one-vertex ones dropped, a stable sort by size"""
    comps = {}
    for vtx, r in enumerate(labels.tolist()):
        comps.setdefault(r, []).append(vtx)
    ranked = sorted((c for c in comps.values() if len(c) > 1), key=len, reverse=True)
    return [c[0] for c in ranked], [len(c) for c in ranked]


def weld_yardstick(v):
    first, rep = {}, []
    for i, row in enumerate(np.asarray(v).tolist()):
        if any(c != c for c in row):
            rep.append(i)
            continue
        rep.append(first.setdefault(tuple(c + 0.0 for c in row), i))       # -0.0 + 0.0 is +0.0
    return np.array(rep, np.int64).reshape(len(rep))


def open_yardstick(faces):
    faces = torch.as_tensor(np.asarray(faces)).reshape(-1, 3).long()
    edges = torch.sort(torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), dim=1)[0]
    uniq, counts = torch.unique(edges, return_counts=True, dim=0)
    return torch.unique(uniq[counts == 1]).numpy()


# ---- components -----------------------------------------------------------------------------------------------------------------------------
def _random_faces(nv, nf, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, nv, (nf, 3))
    f[::5, 1] = f[::5, 0]                                                  # repeated-index faces among them
    f[::7, 2] = f[::7, 1]
    return f


@functools.lru_cache(None)
def cc_case(name):
    """-> (faces int64 [F,3], nv, yardstick labels)"""
    if name == 'mix':
        v, f = scramble(*mix(), seed=1)
        nv = len(v)
    elif name.startswith('edge'):
        nv = int(name[4:])
        f = _random_faces(nv, nv, 100 + nv)
    elif name == 'nv0':
        f, nv = np.zeros((0, 3), np.int64), 0
    elif name == 'nf0':
        f, nv = np.zeros((0, 3), np.int64), 100
    elif name == 'many':
        f, nv = _random_faces(5000, 3000, 2), 5000
    elif name in ('strip', 'strip_reversed'):
        v, f = grid(19999, 1)                                              # 2 x 20 000 vertices, numbered along the strip
        nv = len(v)
        f = nv - 1 - f if name == 'strip_reversed' else f
    elif name == 'fan':
        v, f = fan(30000)
        nv = len(v)
    else:
        raise KeyError(name)
    f = np.ascontiguousarray(f, np.int64).reshape(-1, 3)
    return f, nv, cc_yardstick(f, nv)


CC_CASES = ('mix', 'edge1', 'edge63', 'edge64', 'edge65', 'edge255', 'edge256', 'edge257', 'nv0', 'nf0', 'many', 'strip', 'strip_reversed', 'fan')


def check_components(dev, name):
    f, nv, want = cc_case(name)
    dtype = torch.int32 if len(name) % 2 else torch.int64                  # both index widths over the cases
    got = MT.connected_components(torch.from_numpy(f).to(dtype).to(dev), nv)
    assert got.dtype == torch.int32 and tuple(got.shape) == (nv,)
    got = got.cpu().numpy()
    ncomp = len(np.unique(want))
    print(f'{name}: nv {nv}, nf {len(f)}, {ncomp} components, labels differing from the yardstick: {int((got != want).sum())}')
    assert np.array_equal(got, want)
    assert np.array_equal(want[want], want) and (want <= np.arange(nv)).all()           # the yardstick labels are roots and component minima


def check_rank_and_faces(dev):
    """rank_components / faces_by_component on the mix against the reference's order (sizes 16 12 12 12 9 9 6, ties by the smallest vertex)"""
    f, nv, want = cc_case('mix')
    ft = torch.from_numpy(f).to(dev)
    labels = MT.connected_components(ft, nv)
    ranked, sizes = MT.rank_components(labels)
    roots, lens = rank_yardstick(want)
    assert lens == [16, 12, 12, 12, 9, 9, 6] and roots[1] < roots[2] < roots[3] and roots[4] < roots[5]
    assert ranked.tolist() == roots and sizes.tolist() == lens
    for sel in (slice(0, 5), slice(5, None), slice(0, 0), slice(2, 3)):
        got = MT.faces_by_component(ft, labels, ranked[sel]).cpu().numpy()
        ref = [face for r in roots[sel] for face in f.tolist() if want[face[0]] == r]          # rank order, file order inside
        assert got.tolist() == ref
    none = MT.rank_components(MT.connected_components(ft[:0], 4))
    assert none[0].numel() == 0 and none[1].numel() == 0


def check_components_reject_bad_index(dev):
    f = torch.tensor([[0, 1, 2], [1, 2, 7]], device=dev)
    with pytest.raises(RuntimeError, match='outside'):
        MT.connected_components(f, 7)
    with pytest.raises(RuntimeError, match='outside'):
        MT.connected_components(-f, 7)
    with pytest.raises(RuntimeError, match='outside'):
        MT.open_vertices(f, 7)


# ---- weld -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def weld_case(name):
    """-> positions float64 [n,3] whose values are exact in float32 too"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name[1:].isdigit():
        n = int(name[1:])
        v = rng.integers(-3, 4, (n, 3)) * 0.25                             # 343 lattice points: duplicates from n = 64 on
        if n == 1000:
            v[500:] = rng.standard_normal((500, 3)).astype(np.float32)     # half of the rows distinct
    elif name == 'lattice':
        pts = rng.standard_normal((1000, 3)).astype(np.float32).astype(np.float64)
        v = pts[rng.integers(0, 1000, 50000)]
    elif name == 'one_point':
        v = np.tile(np.array([[0.5, -1.25, 3.0]]), (20000, 1))
    elif name == 'signed_zero':
        v = rng.integers(-1, 2, (300, 3)).astype(np.float64)
        v[rng.random((300, 3)) < 0.5] *= -1.0                              # 0.0 and -0.0 in every column
        assert np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()
    elif name == 'nan':
        v = rng.integers(-2, 3, (400, 3)).astype(np.float64)
        v[rng.integers(0, 400, 60), rng.integers(0, 3, 60)] = np.nan
        v[7] = v[3] = [np.nan, 1.0, 1.0]                                   # two rows with the same NaN pattern: still different
    else:
        raise KeyError(name)
    v = np.ascontiguousarray(v, np.float64).reshape(-1, 3)
    return v, weld_yardstick(v)


WELD_CASES = ('n0', 'n1', 'n64', 'n65', 'n1000', 'lattice', 'one_point', 'signed_zero', 'nan')


def check_weld(dev, name, dtype, table_log2=0):
    v, rep = weld_case(name)
    n = len(v)
    vt = torch.from_numpy(v).to(dtype).to(dev)
    assert np.array_equal(vt.cpu().double().numpy(), v, equal_nan=True)                    # the case is the same in both types
    got = MT.weld_representatives(vt, table_log2)
    assert got.dtype == torch.int32 and tuple(got.shape) == (n,)
    print(f'{name} {dtype} table_log2 {table_log2}: n {n}, {len(np.unique(rep))} distinct, representatives differing: {int((got.cpu().numpy() != rep).sum())}')
    assert np.array_equal(got.cpu().numpy(), rep)
    keep, new_index = MT.weld(vt, table_log2)
    first = rep == np.arange(n)
    assert keep.dtype == torch.int64 and new_index.dtype == torch.int64
    assert np.array_equal(keep.cpu().numpy(), np.flatnonzero(first))                         # first occurrences, ascending
    assert np.array_equal(new_index.cpu().numpy(), (np.cumsum(first) - 1)[rep])
    ok = ~np.isnan(v).any(1)
    assert np.array_equal(v[keep.cpu().numpy()][new_index.cpu().numpy()][ok], v[ok])


def check_weld_forced_table(dev, dtype):
    """the smallest legal table on the 1000-row case: 1024 slots for about 780 distinct rows -- long probe runs, and runs that wrap round"""
    check_weld(dev, 'n1000', dtype, table_log2=10)
    check_weld(dev, 'n65', dtype, table_log2=7)                                              # 65 rows of at most 343 points in 128 slots
    check_weld(dev, 'one_point', dtype, table_log2=15)


def check_weld_table_too_small(dev):
    v = torch.from_numpy(weld_case('n1000')[0]).to(dev)
    lib = L.lib()
    assert lib.d3h_topo_table_log2(L.i64(1000), L.i32(9)) == -1 and lib.d3h_topo_table_log2(L.i64(1024), L.i32(10)) == -1
    assert lib.d3h_topo_table_log2(L.i64(1000), L.i32(10)) == 10 and lib.d3h_topo_table_log2(L.i64(1000), L.i32(0)) == 11
    assert lib.d3h_topo_table_log2(L.i64(0), L.i32(0)) == 0 and lib.d3h_topo_table_log2(L.i64(1), L.i32(0)) == 1 and lib.d3h_topo_table_log2(L.i64(1024), L.i32(0)) == 11
    table = torch.zeros(1024, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    rep = torch.zeros(1024, dtype=torch.int32, device=dev)
    p = lambda t: L._PTR(t.data_ptr())
    assert lib.d3h_weld_insert(p(v), L.i32(1), L.i64(1000), p(table), L.i32(9), p(err), L.stream()) == -1
    assert lib.d3h_weld_lookup(p(v), L.i32(1), L.i64(1000), p(table), L.i32(9), p(rep), p(err), L.stream()) == -1
    with pytest.raises(RuntimeError, match='bad argument'):
        MT.weld(v, table_log2=9)


def check_merge_and_repair(dev):
    v1 = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], dtype=torch.float64, device=dev)
    v2 = torch.tensor([[1.0, 0, 0], [0, 1, 0], [1, 1, 0], [-0.0, 0, 0]], dtype=torch.float64, device=dev)
    f1 = torch.tensor([[0, 1, 2]], device=dev)
    f2 = torch.tensor([[0, 1, 2], [3, 0, 1], [3, 3, 2], [0, 1, 3]], dtype=torch.int32, device=dev)
    v, f = MT.merge_and_repair(v1, f1, v2, f2)
    assert v.cpu().tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [1, 1, 0]]      # the unreferenced vertex 3 stays
    assert f.cpu().tolist() == [[0, 1, 2], [1, 2, 4], [0, 1, 2], [1, 2, 0]]
    assert MT.remove_degenerate(torch.tensor([[1, 1, 2], [1, 2, 1], [2, 1, 1], [0, 1, 2]], device=dev)).cpu().tolist() == [[0, 1, 2]]


# ---- open edges -----------------------------------------------------------------------------------------------------------------------------
def check_open_edges(dev):
    def run(f, nv, dtype=torch.int64):
        got = MT.open_vertices(torch.as_tensor(np.asarray(f)).reshape(-1, 3).to(dtype).to(dev), nv)
        assert got.dtype == torch.int64
        assert np.array_equal(got.cpu().numpy(), open_yardstick(f))
        return got.cpu().tolist()
    v, f = grid(3, 3)
    rim = [i * 4 + j for i in range(4) for j in range(4) if i in (0, 3) or j in (0, 3)]
    assert run(f, len(v)) == rim and len(rim) == 12
    assert run(icosahedron()[1], 12, torch.int32) == []
    assert run([[0, 1, 2], [1, 0, 3], [0, 1, 4]], 5) == [0, 1, 2, 3, 4]                       # edge (0,1) has three faces; the six others one each
    # edge (0,1) with four faces, every other edge with two: an edge of three or more faces is not open, so nothing is
    assert run([[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 4, 1], [2, 0, 3], [2, 1, 3]], 5) == []
    assert run([[0, 1, 2], [0, 1, 3], [0, 1, 4], [2, 0, 3], [2, 1, 3]], 5) == [0, 1, 4]       # three on (0,1): open only through (0,4) and (1,4)
    assert run([[2, 2, 5]], 6) == [2]                                                         # (2,2) once, (2,5) twice
    assert run([[0, 1, 2], [2, 2, 5]], 6, torch.int32) == [0, 1, 2]
    assert run(np.zeros((0, 3), np.int64), 9) == [] and run(np.zeros((0, 3), np.int64), 0) == []
    for seed, (n, m) in enumerate(((1, 1), (7, 9), (15, 16), (40, 13))):                      # 2 to 1040 faces: more than one block of edges
        g, gf = scramble(*grid(n, m), seed=30 + seed)
        run(gf, len(g), torch.int32 if seed % 2 else torch.int64)
    # a forced table: 96 edge slots' worth of keys in the smallest legal table
    v, f = scramble(*grid(4, 4), seed=40)
    m = MT.open_vertex_mask(torch.from_numpy(f).to(dev), len(v), table_log2=7)                 # 3 * 32 = 96 < 128
    assert np.array_equal(np.flatnonzero(m.cpu().numpy()), open_yardstick(f))
    with pytest.raises(RuntimeError, match='bad argument'):
        MT.open_vertex_mask(torch.from_numpy(f).to(dev), len(v), table_log2=6)


def _peel_yardstick(f, rounds):
    f = np.asarray(f)
    for _ in range(rounds):
        f = f[~np.isin(f, open_yardstick(f)).any(axis=1)]
    return f


def check_peel(dev):
    v, f = scramble(*grid(6, 6), seed=41)
    ft = torch.from_numpy(f).to(dev)
    for rounds, left in ((1, 32), (2, 8), (0, 72)):
        got = MT.peel_open_faces(ft, len(v), rounds=rounds).cpu().numpy()
        assert len(got) == left and np.array_equal(got, _peel_yardstick(f, rounds))
    assert np.array_equal(MT.peel_open_faces(ft, len(v)).cpu().numpy(), _peel_yardstick(f, 1))


def check_open_edges_golden(dev):
    """the recorded outputs of the reference's own find_open_edges and remove_faces_with_open_vertices"""
    g = gold()
    for name, (f, nv) in open_edge_meshes().items():
        assert np.array_equal(g[f'open.{name}.faces'], f) and int(g[f'open.{name}.nv']) == nv
        ft = torch.from_numpy(np.ascontiguousarray(f)).to(dev)
        assert np.array_equal(MT.open_vertices(ft, nv).cpu().numpy(), g[f'open.{name}.open_vertices'])
        assert np.array_equal(MT.peel_open_faces(ft, nv).cpu().numpy(), g[f'open.{name}.peeled'])


# ---- process_close_hole ---------------------------------------------------------------------------------------------------------------------
def write_obj_exact(path, v, f):
    with open(path, 'w') as fp:
        fp.write(''.join('v %.17g %.17g %.17g\n' % tuple(r) for r in np.asarray(v).tolist()))
        fp.write(''.join('f %d %d %d\n' % tuple(r) for r in (np.asarray(f) + 1).tolist()))


def read_obj_lines(path):
    """-> (the `v` lines as text, the faces 0-based)"""
    lines = open(path).read().splitlines()
    f = [[int(t) - 1 for t in ln.split()[1:]] for ln in lines if ln.startswith('f ')]
    return [ln for ln in lines if ln.startswith('v ')], np.asarray(f, np.int64).reshape(-1, 3)


def check_close_hole(dev, name, tmp_path):
    import script.connet_face_head as CF
    assert os.path.dirname(os.path.dirname(os.path.abspath(CF.__file__))) == os.path.dirname(os.path.dirname(os.path.abspath(MT.__file__)))
    g = gold()
    k = lambda s: g[f'{name}.{s}']
    bv, bf, cv, cf, num = close_hole_scenarios()[name]
    for got, want in ((bv, k('body_v')), (bf, k('body_f')), (cv, k('cloth_v')), (cf, k('cloth_f')), (num, k('num'))):
        assert np.array_equal(got, want)                                   # the fixture was made from the meshes generated above
    root = str(tmp_path)
    body_path, cloth_path = os.path.join(root, 'body.obj'), os.path.join(root, 'cloth.obj')
    write_obj_exact(body_path, bv, bf)
    write_obj_exact(cloth_path, cv, cf)
    rv, rf = CF.om_loadmesh(body_path)
    assert rv.dtype == np.float64 and np.array_equal(rv, bv) and np.array_equal(rf, bf)
    ret = CF.process_close_hole(None, root, body_path, cloth_path, num=int(num))
    assert [os.path.basename(p) for p in ret] == [str(s) for s in k('returned')] and all(os.path.dirname(p) == root for p in ret)
    box = np.load(ret[2])
    assert box['bbox_min'].dtype == np.float64 and np.array_equal(box['bbox_min'], k('bbox_min')) and np.array_equal(box['bbox_max'], k('bbox_max'))
    faces = {}
    for part, src in (('body_frombody', 'body'), ('cloth_frombody', 'body'), ('body_fromcloth', 'cloth'), ('cloth_fromcloth', 'cloth')):
        vl, faces[part] = read_obj_lines(os.path.join(root, part + '_faces.obj'))
        assert np.array_equal(faces[part], k(part + '_faces').reshape(-1, 3)), part
        assert vl == str(k(src + '_vlines')).splitlines(), part            # ALL vertices of the source mesh, the reference's text
    for side in ('cloth', 'body'):
        path = os.path.join(root, side + '_concat.obj')
        merged = bool(k(side + '_merged'))
        assert os.path.exists(path) == merged
        if not merged:
            continue
        m = CF.merge_and_repair_meshes(bv, faces[side + '_frombody'], cv, faces[side + '_fromcloth'])
        assert np.array_equal(np.asarray(m.vertices), k(side + '_concat_v')) and np.array_equal(np.asarray(m.triangles), k(side + '_concat_f'))
        vl, f = read_obj_lines(path)
        assert np.array_equal(f, k(side + '_concat_f')) and vl == ['v %f %f %f' % tuple(r) for r in k(side + '_concat_v').tolist()]
    if name == 'a':
        assert len(bv) + len(cv) - len(k('body_concat_v')) == 18           # the shared icosahedron and strip
        comps = CF.filter_and_sort_components(CF.find_connected_components(bv, bf))
        assert [len(c) for c in comps] == [16, 12, 12, 12, 9, 9, 6] and all(c == sorted(c) for c in comps)
        lo, hi = CF.body_head_box(comps[:5], bv)
        assert np.array_equal(lo, k('bbox_min')) and np.array_equal(hi, k('bbox_max'))
    if name == 'b':
        assert not bool(k('cloth_merged')) and not bool(k('body_merged')) and os.path.basename(ret[1]) == 'cloth.obj'
    if name == 'c':
        stacked = len(faces['cloth_frombody']) + len(faces['cloth_fromcloth'])
        assert len(k('cloth_concat_f')) == stacked - 1                     # the face with two vertices at one place is gone


def check_obj_reader(dev, tmp_path):
    import script.connet_face_head as CF
    p = os.path.join(str(tmp_path), 'm.obj')
    open(p, 'w').write('# c\nv 0 0 0\nv 1 0 0.5\nvn 0 0 1\nv 0 1 0\nvt 0 0\nf 1/1/1 2/2/1 3/3/1\nf 1//1 3//1 2//1\nf -3 -2 -1\n')
    v, f = CF.om_loadmesh(p)
    assert v.tolist() == [[0, 0, 0], [1, 0, 0.5], [0, 1, 0]] and f.tolist() == [[0, 1, 2], [0, 2, 1], [0, 1, 2]]
    open(p, 'a').write('f 1 2 3 1\n')
    with pytest.raises(ValueError):
        CF.om_loadmesh(p)
    CF.write_pc(p, v, f=f)
    assert open(p).read() == 'v 0.000000 0.000000 0.000000\nv 1.000000 0.000000 0.500000\nv 0.000000 1.000000 0.000000\nf 1 2 3\nf 1 3 2\nf 1 2 3\n'


def check_entry_points_validate(dev):
    """argument errors come back as codes, not as launches: null pointers, negative sizes, misaligned pointers"""
    lib = L.lib()
    zi = torch.zeros(64, dtype=torch.int32, device=dev)
    zl = torch.zeros(64, dtype=torch.int64, device=dev)
    zd = torch.zeros(64, dtype=torch.float64, device=dev)
    zb = torch.zeros(64, dtype=torch.uint8, device=dev)
    p = lambda t, off=0: L._PTR(t.data_ptr() + off)
    i64, i32, s = L.i64, L.i32, L.stream()
    assert lib.d3h_cc_init(None, i64(4), p(zi), s) == -1 and lib.d3h_cc_init(p(zi), i64(-1), p(zi), s) == -1 and lib.d3h_cc_init(p(zi), i64(4), None, s) == -1
    assert lib.d3h_cc_hook(None, i32(1), i64(1), p(zi), i64(4), p(zi), s) == -1 and lib.d3h_cc_hook(p(zl), i32(1), i64(-1), p(zi), i64(4), p(zi), s) == -1
    assert lib.d3h_cc_hook(p(zl), i32(1), i64(1), None, i64(4), p(zi), s) == -1 and lib.d3h_cc_hook(p(zl), i32(1), i64(1), p(zi), i64(-4), p(zi), s) == -1
    assert lib.d3h_cc_hook(p(zl, 4), i32(1), i64(1), p(zi), i64(4), p(zi), s) == -1 and lib.d3h_cc_hook(p(zl), i32(1), i64(1), p(zi), i64(4), None, s) == -1
    assert lib.d3h_cc_flatten(None, i64(4), p(zi), p(zi), s) == -1 and lib.d3h_cc_flatten(p(zi), i64(4), None, p(zi), s) == -1
    assert lib.d3h_cc_flatten(p(zi), i64(-1), p(zi), p(zi), s) == -1 and lib.d3h_cc_flatten(p(zi), i64(4), p(zi), None, s) == -1
    assert lib.d3h_weld_insert(None, i32(1), i64(4), p(zi), i32(0), p(zi), s) == -1 and lib.d3h_weld_insert(p(zd), i32(1), i64(-1), p(zi), i32(0), p(zi), s) == -1
    assert lib.d3h_weld_insert(p(zd), i32(1), i64(4), None, i32(0), p(zi), s) == -1 and lib.d3h_weld_insert(p(zd), i32(1), i64(4), p(zi), i32(0), None, s) == -1
    assert lib.d3h_weld_insert(p(zd, 4), i32(1), i64(4), p(zi), i32(0), p(zi), s) == -1 and lib.d3h_weld_insert(p(zd), i32(1), i64(4), p(zi), i32(2), p(zi), s) == -1
    assert lib.d3h_weld_insert(p(zd), i32(1), i64(4), p(zi), i32(31), p(zi), s) == -1 and lib.d3h_weld_insert(p(zd), i32(1), i64(4), p(zi), i32(-1), p(zi), s) == -1
    assert lib.d3h_weld_lookup(None, i32(1), i64(4), p(zi), i32(0), p(zi), p(zi), s) == -1 and lib.d3h_weld_lookup(p(zd), i32(1), i64(4), None, i32(0), p(zi), p(zi), s) == -1
    assert lib.d3h_weld_lookup(p(zd), i32(1), i64(4), p(zi), i32(0), None, p(zi), s) == -1 and lib.d3h_weld_lookup(p(zd), i32(1), i64(-4), p(zi), i32(0), p(zi), p(zi), s) == -1
    assert lib.d3h_edge_count(None, i32(1), i64(1), i64(4), p(zl), p(zi), i32(0), p(zi), s) == -1 and lib.d3h_edge_count(p(zl), i32(1), i64(-1), i64(4), p(zl), p(zi), i32(0), p(zi), s) == -1
    assert lib.d3h_edge_count(p(zl), i32(1), i64(1), i64(-4), p(zl), p(zi), i32(0), p(zi), s) == -1 and lib.d3h_edge_count(p(zl), i32(1), i64(1), i64(4), None, p(zi), i32(0), p(zi), s) == -1
    assert lib.d3h_edge_count(p(zl), i32(1), i64(1), i64(4), p(zl), None, i32(0), p(zi), s) == -1 and lib.d3h_edge_count(p(zl), i32(1), i64(1), i64(4), p(zl), p(zi), i32(1), p(zi), s) == -1
    assert lib.d3h_edge_count(p(zl), i32(1), i64(1), i64(4), p(zl), p(zi), i32(0), None, s) == -1
    assert lib.d3h_open_vertex_mask(None, p(zi), i32(3), i64(4), p(zb), s) == -1 and lib.d3h_open_vertex_mask(p(zl), None, i32(3), i64(4), p(zb), s) == -1
    assert lib.d3h_open_vertex_mask(p(zl), p(zi), i32(3), i64(4), None, s) == -1 and lib.d3h_open_vertex_mask(p(zl), p(zi), i32(3), i64(-4), p(zb), s) == -1
    assert lib.d3h_open_vertex_mask(p(zl), p(zi), i32(-1), i64(4), p(zb), s) == -1 and lib.d3h_open_vertex_mask(p(zl), p(zi), i32(31), i64(4), p(zb), s) == -1
    assert not zi.any() and not zl.any() and not zb.any()                  # nothing was launched
    for bad in (torch.zeros(3, 2, dtype=torch.int64, device=dev), torch.zeros(3, 3, device=dev)):
        with pytest.raises(RuntimeError):
            MT.connected_components(bad, 4)
    with pytest.raises(RuntimeError):
        MT.weld(torch.zeros(4, 3, dtype=torch.float16, device=dev))


# ---- the namespace merge the drop-in relies on (no kernels) ---------------------------------------------------------------------------------
def check_script_namespace(tmp_path):
    """a directory holding script/other.py BEHIND the package on sys.path: script.connet_face_head is this build's, script.other still imports"""
    import importlib
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(MT.__file__)))
    assert not os.path.exists(os.path.join(pkg, 'script', '__init__.py'))
    other_root = tmp_path / 'elsewhere'
    (other_root / 'script').mkdir(parents=True)
    (other_root / 'script' / 'other.py').write_text('VALUE = 42\n')
    (other_root / 'script' / 'connet_face_head.py').write_text('raise ImportError("shadowed: the package must come first")\n')
    saved_path = list(sys.path)
    saved_mods = {n: sys.modules.pop(n) for n in list(sys.modules) if n == 'script' or n.startswith('script.')}
    try:
        sys.path[:] = [p for p in sys.path if os.path.abspath(p or '.') != pkg]
        sys.path.insert(0, pkg)
        sys.path.append(str(other_root))
        importlib.invalidate_caches()
        cf = importlib.import_module('script.connet_face_head')
        other = importlib.import_module('script.other')
        assert os.path.abspath(cf.__file__) == os.path.join(pkg, 'script', 'connet_face_head.py') and callable(cf.process_close_hole)
        assert other.VALUE == 42 and os.path.abspath(other.__file__).startswith(str(other_root))
        assert sys.modules['script'].__file__ is None and len(list(sys.modules['script'].__path__)) >= 2          # a namespace package over both roots
        for fn in ('find_connected_components', 'filter_and_sort_components', 'body_head_box', 'merge_and_repair_meshes', 'om_loadmesh', 'write_pc'):
            assert callable(getattr(cf, fn))
    finally:
        sys.path[:] = saved_path
        for n in [n for n in sys.modules if n == 'script' or n.startswith('script.')]:
            del sys.modules[n]
        sys.modules.update(saved_mods)
