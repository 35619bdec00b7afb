"""Host side of csrc/lbs.hip: nearest-template-vertex skin weights + blended inverse/forward skinning.

Mirrors deform/smplx_exavatar_deformer.py: interpolate_weights :363-383 (K=1), apply_lbs_inverse :385-421,
lbs_forward :434-486 -- for a whole batch of frames at once (the nearest-vertex ids depend only on the canonical
points, so they are computed once and shared by every frame).

K > 1 (the reference's `self.k`, :40,:366): knnk / KnnGrid.query_k search the K nearest template vertices (1 <= K <= 32, ascending in
(squared distance, index): among equal distances the lower index first) and lbs_points_k skins with the inverse-distance blend of their
weight rows (:367-381); its backward carries the gradient through the blend weights to the point.  K = 1 keeps its own entry points
(knn1, lbs_points) and kernels.
"""
import ctypes

import torch

from . import _lib as L


class KnnGrid:
    """uniform-grid binning of a fixed template for d3h_knn1_grid (csrc/lbs.hip): built once (a sort of the template), reused by every
    iteration.  The query returns exactly what the exhaustive d3h_knn1 returns."""

    def __init__(self, tmpl, max_cells_per_axis=128):
        t = tmpl.detach().contiguous().float()
        nv = t.shape[0]
        lo, hi = t.min(0).values, t.max(0).values
        ext = (hi - lo).clamp_min(1e-6)
        h = float((ext.prod() / max(nv, 1)) ** (1.0 / 3.0))
        h = max(h, float(ext.max()) / max_cells_per_axis) * 1.0001
        lo = lo - 0.5 * h                                               # every vertex strictly inside the box
        g = [int(v) for v in torch.ceil((hi - lo) / h + 0.5).clamp(1, max_cells_per_axis + 2).tolist()]
        self.h, self.g = h, g
        self.lo = (ctypes.c_float * 3)(*[float(v) for v in lo.tolist()])     # HOST argument of the C ABI
        lo = torch.tensor(list(self.lo), dtype=torch.float32, device=t.device)
        inv_h = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(h, dtype=torch.float32)
        c = torch.floor((t - lo) * inv_h.to(t.device)).long()
        for a in range(3):
            c[:, a].clamp_(0, g[a] - 1)
        cell = (c[:, 2] * g[1] + c[:, 1]) * g[0] + c[:, 0]
        order = torch.sort(cell, stable=True).indices                   # ascending original index inside a cell
        ncell = g[0] * g[1] * g[2]
        counts = torch.bincount(cell, minlength=ncell)
        self.cell_start = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32).contiguous()
        self.cell_pts = torch.cat([t[order], order.to(torch.int32).view(torch.float32)[:, None]], dim=1).contiguous()
        # seed of every cell: sorted position of the vertex nearest to the cell centre (one exhaustive search, once)
        ii = [torch.arange(n, device=t.device, dtype=torch.float32) for n in g]
        cz, cy, cx = torch.meshgrid(ii[2], ii[1], ii[0], indexing='ij')
        centres = (torch.stack([cx, cy, cz], -1).reshape(-1, 3) + 0.5) * h + lo
        inv = torch.empty(nv, dtype=torch.int64, device=t.device)
        inv[order] = torch.arange(nv, device=t.device)
        self.cell_seed = inv[knn1(centres.contiguous(), t).long()].to(torch.int32).contiguous()
        self.nv = nv
        self.key = (tmpl.data_ptr(), tmpl._version, tuple(tmpl.shape))
        self.src = tmpl                      # kept alive: the address in the key cannot be handed to another tensor meanwhile

    def matches(self, tmpl):
        return self.key == (tmpl.data_ptr(), tmpl._version, tuple(tmpl.shape))

    def query_counted(self, pts_cap, counts):
        """nearest template vertex of the first counts[0] + 3 counts[1] + 4 counts[2] rows of `pts_cap` (a buffer at its capacity), the row
        count read on the DEVICE (d3h/mtets.py: work queued before the host knows the sizes of the extraction) -> idx [capacity] int32.
        `counts`: the extraction's counter block of at least 11 int32 (entry 10 is its overflow flag: when set, nothing is written)"""
        pts = _capacity_points(pts_cap, 'query_counted')
        _check_counts(counts, pts, 'query_counted')
        idx = torch.empty(pts.shape[0], dtype=torch.int32, device=pts.device)
        L.call('knn1_grid_counted', pts, pts.shape[0], counts, self.cell_pts, self.cell_start, self.cell_seed, self.nv, self.lo, self.h, self.g[0],
               self.g[1], self.g[2], idx)
        return idx

    def query(self, pts, want_dist=False):
        pts = pts.detach().contiguous().float()
        idx = torch.empty(pts.shape[0], dtype=torch.int32, device=pts.device)
        dist = torch.empty(pts.shape[0], dtype=torch.float32, device=pts.device) if want_dist else None
        L.call('knn1_grid', pts, pts.shape[0], self.cell_pts, self.cell_start, self.cell_seed, self.nv, self.lo, self.h, self.g[0], self.g[1],
               self.g[2], idx, dist)
        return (idx, dist) if want_dist else idx

    def query_k(self, pts, K):
        """the K nearest template vertices of every point -> KnnResult(idx [P,K] int32, d2 [P,K]); exactly what knnk returns without a grid"""
        pts = _knnk_args(pts, K)
        P = pts.shape[0]
        idx = torch.empty(P, K, dtype=torch.int32, device=pts.device)
        d2 = torch.empty(P, K, dtype=torch.float32, device=pts.device)
        L.call('knnk_grid', pts, P, self.cell_pts, self.cell_start, self.nv, self.lo, self.h, self.g[0], self.g[1], self.g[2], K, idx, d2)
        return KnnResult(idx, d2)

    def query_k_counted(self, pts_cap, counts, K, out=None):
        """query_k over the first counts[0] + 3 counts[1] + 4 counts[2] rows of `pts_cap` (a buffer at its capacity), the row count read on the
        DEVICE -> KnnResult at the capacity; the other rows are not written (`out`: a KnnResult to write into).  `counts`: as in query_counted"""
        pts = _knnk_args(pts_cap, K, convert=False)
        cap = pts.shape[0]
        _check_counts(counts, pts, 'query_k_counted')
        if out is None:
            out = KnnResult(torch.empty(cap, K, dtype=torch.int32, device=pts.device), torch.empty(cap, K, dtype=torch.float32, device=pts.device))
        _check_knn_result(out, cap, K, 'query_k_counted')
        L.call('knnk_grid_counted', pts, cap, counts, self.cell_pts, self.cell_start, self.nv, self.lo, self.h, self.g[0], self.g[1], self.g[2], K,
               out.idx, out.d2)
        return out


K_MAX = 32        # KNNK_MAX of csrc/lbs.hip
J_MAX = 64        # MAXJ of csrc/lbs.hip
N_COUNTS = 11     # counted_rows() of csrc/lbs.hip reads entries 0..2 (the row counts) and 10 (the extraction's overflow flag)


def _check_counts(counts, pts, what):
    if not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 1 or counts.numel() < N_COUNTS or \
            not counts.is_contiguous() or counts.device != pts.device:
        raise RuntimeError(f'd3h {what}: counts must be the extraction\'s contiguous int32 counter block of at least {N_COUNTS} entries on the '
                           f'device of the points (the kernels read entries 0..2 and 10)')


def _capacity_points(pts_cap, what):
    pts = pts_cap.detach()
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.dtype != torch.float32 or not pts.is_contiguous():
        raise RuntimeError(f'd3h {what}: the capacity buffer must be contiguous float32 [capacity,3]')
    return pts


def _lbs_args(pts, idx, lbs_w, A0, A, trans, what):
    """the checks of _lbsk_args for the K = 1 entry points: everything the kernels index with is checked on the host, before any launch"""
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise RuntimeError(f'd3h {what}: points must be [P,3], got {tuple(pts.shape)}')
    P = pts.shape[0]
    if not torch.is_tensor(idx) or idx.dtype != torch.int32 or tuple(idx.shape) != (P,) or not idx.is_contiguous() or idx.device != pts.device:
        raise RuntimeError(f'd3h {what}: idx must be a contiguous int32 tensor of shape {(P,)} on the device of the points (knn1 returns one), got '
                           f'{tuple(idx.shape)} {idx.dtype}')
    if lbs_w.dim() != 2 or A0.dim() != 3 or tuple(A0.shape[1:]) != (4, 4) or A.dim() != 4 or tuple(A.shape[2:]) != (4, 4):
        raise RuntimeError(f'd3h {what}: lbs_w [V,J], A0 [J,4,4] and A [B,J,4,4] expected, got {tuple(lbs_w.shape)}, {tuple(A0.shape)}, {tuple(A.shape)}')
    nj, nb = lbs_w.shape[1], A.shape[0]
    if not 1 <= nj <= J_MAX or A0.shape[0] != nj or A.shape[1] != nj or nb < 1 or \
            trans.dim() not in (2, 3) or trans.shape[0] != nb or trans.shape[-1] != 3 or trans.numel() != nb * 3:
        raise RuntimeError(f'd3h {what}: {nj} joints in lbs_w (1..{J_MAX}), A0 {tuple(A0.shape)}, A {tuple(A.shape)}, trans {tuple(trans.shape)}')


class KnnResult:
    """K nearest template vertices of P points: idx [P,K] int32, d2 [P,K] float32 squared distances.  Unpacks as `idx, d2 = r`; a slice
    narrows the ROWS (`r[:p]`: the deformer's callers hand a search result on without looking into it)"""
    __slots__ = ('idx', 'd2')

    def __init__(self, idx, d2):
        self.idx, self.d2 = idx, d2

    def __iter__(self):
        return iter((self.idx, self.d2))

    def __len__(self):
        return self.idx.shape[0]

    def __getitem__(self, s):
        if isinstance(s, slice):
            return KnnResult(self.idx[s], self.d2[s])
        return (self.idx, self.d2)[s]

    @property
    def K(self):
        return self.idx.shape[1]


def _check_K(K):
    if not isinstance(K, int) or isinstance(K, bool) or not 1 <= K <= K_MAX:
        raise ValueError(f'd3h knn: K must be an int in 1..{K_MAX}, got {K!r}')


def _knnk_args(pts, K, convert=True):
    _check_K(K)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise RuntimeError(f'd3h knn: points must be [P,3], got {tuple(pts.shape)}')
    pts = pts.detach()
    if convert:
        return pts.contiguous().float()
    if pts.dtype != torch.float32 or not pts.is_contiguous():
        raise RuntimeError('d3h knn: the capacity buffer must be contiguous float32')
    return pts


def _check_knn_result(nn, P, K, what):
    idx, d2 = nn.idx, nn.d2
    if tuple(idx.shape) != (P, K) or tuple(d2.shape) != (P, K) or idx.dtype != torch.int32 or d2.dtype != torch.float32 or \
            not idx.is_contiguous() or not d2.is_contiguous():
        raise RuntimeError(f'd3h {what}: the search result must be contiguous idx int32 / d2 float32 of shape {(P, K)}, got '
                           f'{tuple(idx.shape)} {idx.dtype} / {tuple(d2.shape)} {d2.dtype}')


def knnk(pts, tmpl, K, grid=None):
    """the K nearest template vertices of every point, 1 <= K <= 32 -> KnnResult(idx [P,K] int32, d2 [P,K] squared L2), ascending in
    (distance, index): among equal distances the lower index stays and comes first (knn_cpu.cpp:39-66).  Slots tmpl.shape[0]..K-1 of a
    template with fewer than K vertices hold index 0 and distance 0; a query without a finite distance holds index 0 and distance +inf.
    `grid`: a KnnGrid of `tmpl` (same result)"""
    if grid is not None:
        return grid.query_k(pts, K)
    pts = _knnk_args(pts, K)
    if tmpl.dim() != 2 or tmpl.shape[1] != 3 or tmpl.shape[0] == 0:
        raise RuntimeError(f'd3h knnk: the template must be [V,3] with V >= 1, got {tuple(tmpl.shape)}')
    tmpl = tmpl.detach().contiguous().float()
    P = pts.shape[0]
    idx = torch.empty(P, K, dtype=torch.int32, device=pts.device)
    d2 = torch.empty(P, K, dtype=torch.float32, device=pts.device)
    L.call('knnk', pts, P, tmpl, tmpl.shape[0], K, idx, d2)
    return KnnResult(idx, d2)


def knn1(pts, tmpl, grid=None):
    """index (int32 [P]) of the nearest template vertex; squared L2, first minimum wins (knn_cpu.cpp:13-69).  `grid`: a KnnGrid of
    `tmpl` (fixed templates: same result, ~10x faster)"""
    if grid is not None:
        return grid.query(pts)
    pts = pts.detach().contiguous().float()
    tmpl = tmpl.detach().contiguous().float()
    idx = torch.empty(pts.shape[0], dtype=torch.int32, device=pts.device)
    L.call('knn1', pts, pts.shape[0], tmpl, tmpl.shape[0], idx, None)
    return idx


class _LBSFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, idx, lbs_w, A0, A, trans, pre):
        pts_c = pts.contiguous().float()
        A0c = A0.detach().reshape(-1, 16).contiguous().float()
        Ac = A.detach().reshape(A.shape[0], -1, 16).contiguous().float()
        tr = trans.detach().reshape(-1, 3).contiguous().float()
        nb, nj, P = Ac.shape[0], Ac.shape[1], pts_c.shape[0]
        if pre is not None:                 # computed by lbs_points_counted from the same arguments before the row count was known on the host
            if tuple(pre.shape) != (nb, P, 3) or not pre.is_contiguous():
                raise RuntimeError(f'd3h lbs_points: the pre-computed result is {tuple(pre.shape)}, expected {(nb, P, 3)}')
            out = pre
        else:
            out = torch.empty(nb, P, 3, dtype=torch.float32, device=pts.device)
            L.call('lbs_fwd', pts_c, P, idx, lbs_w, nj, A0c, Ac, tr, nb, out, None)
        ctx.save_for_backward(pts_c, idx, lbs_w, A0c, Ac)
        ctx.shapes = (A.shape, trans.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        pts, idx, lbs_w, A0c, Ac = ctx.saved_tensors
        nb, nj, P = Ac.shape[0], Ac.shape[1], pts.shape[0]
        g = g.contiguous().float()
        d_pts = torch.empty_like(pts)
        per_frame = torch.empty(nb, P, 3, dtype=torch.float32, device=pts.device) if nb > 1 else None      # summed in frame order: deterministic
        need_A, need_t = ctx.needs_input_grad[4], ctx.needs_input_grad[5]
        dA = L.zeros((nb, nj, 16), torch.float32, pts.device) if need_A else None
        dT = L.zeros((nb, 3), torch.float32, pts.device) if need_t else None
        L.call('lbs_bwd', pts, P, idx, lbs_w, nj, A0c, Ac, nb, g, d_pts, per_frame, dA, dT)
        a_shape, t_shape = ctx.shapes
        return (d_pts, None, None, None, dA.reshape(a_shape) if need_A else None, dT.reshape(t_shape) if need_t else None, None)


def lbs_points(pts, idx, lbs_w, A0, A, trans, pre=None):
    """pts [P,3] canonical-mesh points, idx [P] nearest template vertex, lbs_w [V,J], A0 [J,4,4] init-pose transforms,
    A [B,J,4,4] frame transforms, trans [B,3]  ->  posed points [B,P,3].  `pre`: the result already computed by lbs_points_counted (the
    launch is skipped, the autograd node is the same)"""
    _lbs_args(pts, idx, lbs_w, A0, A, trans, 'lbs_points')
    return _LBSFn.apply(pts, idx, lbs_w.contiguous().float(), A0, A, trans, pre)


def lbs_points_counted(pts_cap, counts, idx_cap, lbs_w, A0, A, trans):
    """lbs_points over the first r = counts[0] + 3 counts[1] + 4 counts[2] rows of `pts_cap` [capacity, 3], r read on the DEVICE: the launch
    is queued before the host knows r.  -> a flat float buffer whose leading B * r * 3 floats are the dense [B, r, 3] result (narrow it with
    counted_result once r is known and hand it to lbs_points(..., pre=)).  `counts`: the extraction's counter block of at least 11 int32;
    entry 10 is its overflow flag: when set, nothing is written"""
    pts = _capacity_points(pts_cap, 'lbs_points_counted')
    _check_counts(counts, pts, 'lbs_points_counted')
    _lbs_args(pts, idx_cap, lbs_w, A0, A, trans, 'lbs_points_counted')
    A0c = A0.detach().reshape(-1, 16).contiguous().float()
    Ac = A.detach().reshape(A.shape[0], -1, 16).contiguous().float()
    tr = trans.detach().reshape(-1, 3).contiguous().float()
    nb, nj, cap = Ac.shape[0], Ac.shape[1], pts_cap.shape[0]
    out = torch.empty(nb * cap * 3, dtype=torch.float32, device=pts_cap.device)
    L.call('lbs_fwd_counted', pts, cap, counts, idx_cap, lbs_w.contiguous().float(), nj, A0c, Ac, tr, nb, out)
    return out


def _lbsk_args(nn, lbs_w, tmpl, A0, A, trans, P, what):
    K = nn.idx.shape[1] if nn.idx.dim() == 2 else 0
    _check_K(K)
    _check_knn_result(nn, P, K, what)
    if lbs_w.dim() != 2 or tmpl.dim() != 2 or tmpl.shape[1] != 3 or tmpl.shape[0] != lbs_w.shape[0]:
        raise RuntimeError(f'd3h {what}: lbs_w [V,J] and tmpl [V,3] expected, got {tuple(lbs_w.shape)} and {tuple(tmpl.shape)}')
    A0c = A0.detach().reshape(-1, 16).contiguous().float()
    Ac = A.detach().reshape(A.shape[0], -1, 16).contiguous().float()
    tr = trans.detach().reshape(-1, 3).contiguous().float()
    if A0c.shape[0] != lbs_w.shape[1] or Ac.shape[1] != lbs_w.shape[1] or tr.shape[0] != Ac.shape[0]:
        raise RuntimeError(f'd3h {what}: {lbs_w.shape[1]} joints in lbs_w, A0 {tuple(A0.shape)}, A {tuple(A.shape)}, trans {tuple(trans.shape)}')
    return K, A0c, Ac, tr


class _LBSKFn(torch.autograd.Function):
    """K-blended skinning: _LBSFn with the weight rows of the K nearest vertices blended by inverse distance; d(pts) includes the path
    through the blend weights (the squared distances are functions of pts; the template is a constant)"""

    @staticmethod
    def forward(ctx, pts, idx, d2, lbs_w, tmpl, A0, A, trans, pre):
        pts_c = pts.contiguous().float()
        P = pts_c.shape[0]
        K, A0c, Ac, tr = _lbsk_args(KnnResult(idx, d2), lbs_w, tmpl, A0, A, trans, P, 'lbs_points_k')
        nb, nj = Ac.shape[0], Ac.shape[1]
        if pre is not None:                 # computed by lbs_points_k_counted from the same arguments before the row count was known on the host
            if tuple(pre.shape) != (nb, P, 3) or not pre.is_contiguous():
                raise RuntimeError(f'd3h lbs_points_k: the pre-computed result is {tuple(pre.shape)}, expected {(nb, P, 3)}')
            out = pre
        else:
            out = torch.empty(nb, P, 3, dtype=torch.float32, device=pts.device)
            L.call('lbsk_fwd', pts_c, P, idx, d2, K, lbs_w, nj, A0c, Ac, tr, nb, out, None)
        ctx.save_for_backward(pts_c, idx, d2, lbs_w, tmpl, A0c, Ac)
        ctx.shapes = (A.shape, trans.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        pts, idx, d2, lbs_w, tmpl, A0c, Ac = ctx.saved_tensors
        nb, nj, P, K = Ac.shape[0], Ac.shape[1], pts.shape[0], idx.shape[1]
        g = g.contiguous().float()
        need_p, need_A, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[6], ctx.needs_input_grad[7]
        d_pts = torch.empty_like(pts) if need_p else None
        per_frame = torch.empty(nb, P, 3, dtype=torch.float32, device=pts.device) if need_p and nb > 1 else None   # summed in frame order
        dA = L.zeros((nb, nj, 16), torch.float32, pts.device) if need_A else None
        dT = L.zeros((nb, 3), torch.float32, pts.device) if need_t else None
        L.call('lbsk_bwd', pts, P, idx, d2, K, tmpl, lbs_w, nj, A0c, Ac, nb, g, d_pts, per_frame, dA, dT)
        a_shape, t_shape = ctx.shapes
        return (d_pts, None, None, None, None, None, dA.reshape(a_shape) if need_A else None, dT.reshape(t_shape) if need_t else None, None)


def lbs_points_k(pts, nn, lbs_w, tmpl, A0, A, trans, pre=None):
    """lbs_points with the skin weights blended over the K nearest template vertices: nn = KnnResult(idx [P,K], d2 [P,K]) of knnk(pts, tmpl, K),
    a_k = u_k / sum u with u_k = 1 / (sqrt(d2_k + 1e-9) + 1e-9), w = sum_k a_k lbs_w[idx_k] (interpolate_weights :367-381)  ->  posed points
    [B,P,3].  tmpl [V,3]: the template nn was searched in, a constant; the gradient of pts includes the one through the blend weights.
    `pre`: the result already computed by lbs_points_k_counted"""
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise RuntimeError(f'd3h lbs_points_k: points must be [P,3], got {tuple(pts.shape)}')
    return _LBSKFn.apply(pts, nn.idx, nn.d2, lbs_w.detach().contiguous().float(), tmpl.detach().contiguous().float(), A0, A, trans, pre)


def lbs_points_k_counted(pts_cap, counts, nn_cap, lbs_w, tmpl, A0, A, trans):
    """lbs_points_k over the first r = counts[0] + 3 counts[1] + 4 counts[2] rows of `pts_cap` [capacity, 3] (nn_cap: query_k_counted of the same
    buffer), r read on the DEVICE.  -> a flat float buffer whose leading B * r * 3 floats are the dense [B, r, 3] result (counted_result).
    `counts`: as in lbs_points_counted"""
    pts = _capacity_points(pts_cap, 'lbs_points_k_counted')
    _check_counts(counts, pts, 'lbs_points_k_counted')
    cap = pts.shape[0]
    K, A0c, Ac, tr = _lbsk_args(nn_cap, lbs_w, tmpl, A0, A, trans, cap, 'lbs_points_k_counted')
    nb, nj = Ac.shape[0], Ac.shape[1]
    out = torch.empty(nb * cap * 3, dtype=torch.float32, device=pts.device)
    L.call('lbsk_fwd_counted', pts, cap, counts, nn_cap.idx, nn_cap.d2, K, lbs_w.detach().contiguous().float(), nj, A0c, Ac, tr, nb, out)
    return out


def counted_result(flat, nb, rows):
    return flat[:nb * rows * 3].view(nb, rows, 3)
