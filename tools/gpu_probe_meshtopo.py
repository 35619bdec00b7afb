"""Times of the three kernel groups of csrc/meshtopo.hip on the GPU, beside a host yardstick each.

    python tools/gpu_probe_meshtopo.py [--out FILE.md] [--commit TEXT] [--sizes 100000 1000000]      # default profiles/meshtopo_probe.md

Mesh: a square grid of about --sizes vertices (two triangles per cell) after a seeded vertex permutation and face shuffle, cut into 64 components by
dropping every face that crosses one of 7 + 7 grid lines; weld input: the float64 positions of that mesh stacked on a copy of their first half (a
third of the rows are duplicates).  Per size:
  components   d3h_cc_init + d3h_cc_hook + d3h_cc_flatten, launches only, and meshtopo.connected_components (allocation and the read-back of the error
               word included); yardstick scipy.sparse.csgraph.connected_components on the host (building the sparse matrix included)
  weld         d3h_weld_insert + d3h_weld_lookup, launches only, and meshtopo.weld; yardstick a Python dict over the rows, in vertex order
  open edges   d3h_edge_count + d3h_open_vertex_mask, launches only, and meshtopo.open_vertices; yardstick the reference's torch.unique route
               (process_body_cloth_head_msdfcut.py:92-102) on the same device
Results of the GPU route and of the yardstick are compared before anything is timed.

Timing: device rows are warmed up (3 calls), then 10 windows are timed with device events, each as many back-to-back calls as make it last about
20 ms; host rows are 3 timed calls of a host clock.  The table gives the per-call median and the min-max spread.  Records, not gates: no test
asserts any of them, and nothing in the repository claims a speed from them."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'd3human-code_amd')
sys.path.insert(0, PKG)
from d3h import _lib as L, meshtopo as MT          # noqa: E402

REPS = 10


def _window(fn, k):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / k


def timed(fn, reps=REPS, window_us=20000.0):
    """-> (median, min, max) in us per call, device events"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    k = max(1, min(200, int(window_us / max(_window(fn, 1), 1.0))))
    ts = [_window(fn, k) for _ in range(reps)]
    return statistics.median(ts), min(ts), max(ts)


def timed_host(fn, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts), min(ts), max(ts)


def make_mesh(nv_target, seed):
    n = int(round(nv_target ** 0.5)) - 1
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    v = np.stack([i.reshape(-1), np.zeros(i.size), j.reshape(-1)], 1) * (1.0 / n)
    ci, cj = i[:-1, :-1].reshape(-1), j[:-1, :-1].reshape(-1)
    a = ci * (n + 1) + cj
    f = np.concatenate([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)])
    step = max(n // 8, 1)
    keep = ((ci % step) != step - 1) | (ci // step >= 7)
    keep &= ((cj % step) != step - 1) | (cj // step >= 7)
    f = f[np.concatenate([keep, keep])]
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(v))
    v2 = np.empty_like(v)
    v2[perm] = v
    return v2, perm[f][rng.permutation(len(f))]


def open_by_unique(faces):
    edges = torch.sort(torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], dim=0), dim=1)[0]
    uniq, counts = torch.unique(edges, return_counts=True, dim=0)
    return torch.unique(uniq[counts == 1])


def main(dev='cuda'):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'meshtopo_probe.md'))
    ap.add_argument('--commit', default=None)
    ap.add_argument('--sizes', type=int, nargs='+', default=[100000, 1000000])
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = 'unknown'
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components as sp_cc
    lib = L.lib()
    lines = [f'# Mesh topology probe ({commit}; {torch.cuda.get_device_name(0)})', '',
             'Per-call times in microseconds: median (min - max).  Device rows: 10 windows of about 20 ms of back-to-back calls, device events; host rows: 3 calls, '
             'host clock.  "launches only" = the C entry points on preallocated buffers, nothing read back; the d3h.meshtopo rows include allocation and '
             'the one read-back per call.  Records, not gates.', '']
    p = lambda t: L._PTR(t.data_ptr())
    for nv_target in a.sizes:
        v_np, f_np = make_mesh(nv_target, seed=nv_target % 1000 + 1)
        nv, nf = len(v_np), len(f_np)
        f = torch.from_numpy(f_np).to(dev)
        w_np = np.concatenate([v_np, v_np[:nv // 2]])
        w = torch.from_numpy(w_np).to(dev)
        n = len(w_np)
        # ---- results first ----
        labels = MT.connected_components(f, nv)
        ncomp, sp_labels = sp_cc(sp.coo_matrix((np.ones(2 * nf), (f_np[:, [0, 1]].reshape(-1), f_np[:, [1, 2]].reshape(-1))), shape=(nv, nv)), directed=False)
        lab = labels.cpu().numpy()
        first = np.full(ncomp, nv)
        np.minimum.at(first, sp_labels, np.arange(nv))
        assert np.array_equal(lab, first[sp_labels]), 'components differ from scipy'
        keep, new_index = MT.weld(w)
        seen = {}
        rep = np.array([seen.setdefault(r, i) for i, r in enumerate(map(tuple, w_np.tolist()))])
        assert np.array_equal(keep.cpu().numpy(), np.flatnonzero(rep == np.arange(n))), 'weld differs from the dict'
        ov = MT.open_vertices(f, nv)
        assert torch.equal(ov, open_by_unique(f)), 'open vertices differ from torch.unique'
        lines += [f'## {nv} vertices, {nf} faces: {ncomp} components; weld input {n} rows, {len(keep)} distinct; {ov.numel()} open vertices', '',
                  '| group | what | median us | min | max |', '|---|---|---|---|---|']

        def row(group, what, t):
            lines.append(f'| {group} | {what} | {t[0]:.1f} | {t[1]:.1f} | {t[2]:.1f} |')
            print(lines[-1], flush=True)

        parent, label, err = torch.empty(nv, dtype=torch.int32, device=dev), torch.empty(nv, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        s = L.stream()

        def cc_launches():
            lib.d3h_cc_init(p(parent), L.i64(nv), p(err), s)
            lib.d3h_cc_hook(p(f), L.i32(1), L.i64(nf), p(parent), L.i64(nv), p(err), s)
            lib.d3h_cc_flatten(p(parent), L.i64(nv), p(label), p(err), s)
        row('components', 'd3h_cc_init + hook + flatten, launches only', timed(cc_launches))
        assert torch.equal(label, labels) and int(err.item()) == 0
        row('components', 'd3h.meshtopo.connected_components', timed(lambda: MT.connected_components(f, nv)))
        row('components', 'host: scipy.sparse.csgraph.connected_components (matrix build included)', timed_host(lambda: sp_cc(
            sp.coo_matrix((np.ones(2 * nf), (f_np[:, [0, 1]].reshape(-1), f_np[:, [1, 2]].reshape(-1))), shape=(nv, nv)), directed=False)))

        lg = lib.d3h_topo_table_log2(L.i64(n), L.i32(0))
        table, reps_ = torch.empty(1 << lg, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)

        def weld_launches():
            lib.d3h_weld_insert(p(w), L.i32(1), L.i64(n), p(table), L.i32(0), p(err), s)
            lib.d3h_weld_lookup(p(w), L.i32(1), L.i64(n), p(table), L.i32(0), p(reps_), p(err), s)
        row('weld', f'd3h_weld_insert + lookup (float64, 2^{lg} slots), launches only', timed(weld_launches))
        assert np.array_equal(reps_.cpu().numpy(), rep) and int(err.item()) == 0
        row('weld', 'd3h.meshtopo.weld', timed(lambda: MT.weld(w)))

        def dict_weld():
            d = {}
            return [d.setdefault(r, i) for i, r in enumerate(map(tuple, w_np.tolist()))]
        row('weld', 'host: Python dict over the rows', timed_host(dict_weld))

        lg = lib.d3h_topo_table_log2(L.i64(3 * nf), L.i32(0))
        keys, counts = torch.empty(1 << lg, dtype=torch.int64, device=dev), torch.empty(1 << lg, dtype=torch.int32, device=dev)
        mask = torch.empty(nv, dtype=torch.uint8, device=dev)

        def edge_launches():
            lib.d3h_edge_count(p(f), L.i32(1), L.i64(nf), L.i64(nv), p(keys), p(counts), L.i32(0), p(err), s)
            lib.d3h_open_vertex_mask(p(keys), p(counts), L.i32(lg), L.i64(nv), p(mask), s)
        row('open edges', f'd3h_edge_count + d3h_open_vertex_mask (2^{lg} slots), launches only', timed(edge_launches))
        assert torch.equal(torch.nonzero(mask).reshape(-1), ov) and int(err.item()) == 0
        row('open edges', 'd3h.meshtopo.open_vertices', timed(lambda: MT.open_vertices(f, nv)))
        row('open edges', 'same device: torch.unique over the 3F sorted edges (the reference\'s route)', timed(lambda: open_by_unique(f)))
        lines.append('')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
