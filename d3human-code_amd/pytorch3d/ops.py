"""Shim for `from pytorch3d.ops import knn_points, knn_gather` (deform/smplx_exavatar_deformer.py:7, geometry/hmsdf.py:44) on the HIP
kernels of csrc/lbs.hip, with the contract of third_parties/pytorch3d/ops.py:123-259 for 3-D points and the squared L2 distance:

  knn_points(p1 [N,P1,3], p2 [N,P2,3], lengths1, lengths2, norm=2, K, version, return_nn, return_sorted) -> KNN(dists, idx, knn)

  - any 1 <= K <= 32; the K neighbours come in ascending order of (squared distance, index) -- among equal distances the lower index of p2
    stays and comes first (knn_cpu.cpp:39-66) -- which satisfies return_sorted=True and False alike;
  - dists [N,P1,K] float32 and idx [N,P1,K] int64 are zero where a cloud of p2 has fewer than K points (slots lengths2[n]..K-1) and where a
    cloud of p1 is shorter than P1 (rows lengths1[n]..P1-1);
  - dists is differentiable in p1 AND p2 (knn_cpu.cpp:75-128: d dists[n,i,k] / d p1[n,i] = 2 (p1[n,i] - p2[n,idx]), the opposite sign
    scattered into p2); idx is not differentiable;
  - return_nn: knn = knn_gather(p2, idx, lengths2), [N,P1,K,3].

Limits, each a NotImplementedError: norm=1 (L1), K > 32, point dimensions other than 3.  K = 1 without lengths and without a gradient to
carry is the single-neighbour kernel d3h_knn1 (the collision term and the deformer's default)."""
from collections import namedtuple

import torch

from d3h import _lib as L
from d3h import lbs as HL

_KNN = namedtuple('KNN', 'dists idx knn')


class _KnnPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, p2, lengths1, lengths2, K):
        N, P1 = p1.shape[:2]
        a, b = p1.detach().contiguous().float(), p2.detach().contiguous().float()
        dists = torch.zeros(N, P1, K, dtype=torch.float32, device=p1.device)
        idx = torch.zeros(N, P1, K, dtype=torch.int64, device=p1.device)
        for n, (l1, l2) in enumerate(zip(lengths1.tolist(), lengths2.tolist())):
            if l1 > 0 and l2 > 0:
                r = HL.knnk(a[n, :l1], b[n, :l2], K)          # slots l2..K-1: index 0, distance 0
                idx[n, :l1] = r.idx.long()
                dists[n, :l1] = r.d2
        ctx.save_for_backward(a, b, lengths1, lengths2, idx)
        ctx.mark_non_differentiable(idx)
        return dists, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_dists, grad_idx):
        p1, p2, lengths1, lengths2, idx = ctx.saved_tensors
        N, P1, K = idx.shape
        dev = p1.device
        live = (torch.arange(P1, device=dev)[None, :, None] < lengths1.to(dev)[:, None, None]) & \
               (torch.arange(K, device=dev)[None, None, :] < lengths2.to(dev)[:, None, None])            # knn_cpu.cpp:101-106
        nb = torch.gather(p2[:, :, None].expand(-1, -1, K, -1), 1, idx[..., None].expand(-1, -1, -1, 3))
        diff = 2.0 * (grad_dists.float() * live)[..., None] * (p1[:, :, None] - nb)                     # [N,P1,K,3]
        grad_p1 = diff.sum(2) if ctx.needs_input_grad[0] else None
        grad_p2 = None
        if ctx.needs_input_grad[1]:
            grad_p2 = torch.zeros_like(p2).scatter_add_(1, idx.reshape(N, P1 * K, 1).expand(-1, -1, 3), -diff.reshape(N, P1 * K, 3))
        return grad_p1, grad_p2, None, None, None


def _lengths(lengths, N, full, dev, what):
    if lengths is None:
        return torch.full((N,), full, dtype=torch.int64, device=dev)
    if lengths.shape != (N,) or int(lengths.min()) < 0 or int(lengths.max()) > full:
        raise ValueError(f'{what} must have shape ({N},) and values in [0, {full}]')
    return lengths.to(torch.int64)


def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, version=-1, return_nn=False, return_sorted=True):
    if p1.dim() != 3 or p2.dim() != 3:
        raise ValueError('pts1 and pts2 must be (N, P, D) tensors.')
    if p1.shape[0] != p2.shape[0]:
        raise ValueError('pts1 and pts2 must have the same batch dimension.')
    if p1.shape[2] != p2.shape[2]:
        raise ValueError('pts1 and pts2 must have the same point dimension.')
    if norm not in (1, 2):
        raise ValueError('Support for 1 or 2 norm.')
    if norm != 2:
        raise NotImplementedError('d3h knn_points: norm=2 (squared L2) only; the L1 distance is not implemented')
    if p1.shape[2] != 3:
        raise NotImplementedError(f'd3h knn_points: point dimension 3 only, got D = {p1.shape[2]}')
    if not isinstance(K, int) or K < 1:
        raise ValueError(f'K must be a positive integer, got {K!r}')
    if K > HL.K_MAX:
        raise NotImplementedError(f'd3h knn_points: K <= {HL.K_MAX} only, got K = {K}')
    B, P = p1.shape[:2]
    carries_grad = torch.is_grad_enabled() and (p1.requires_grad or p2.requires_grad)
    if K == 1 and lengths1 is None and lengths2 is None and not carries_grad:
        if p2.shape[1] == 0:
            raise ValueError('d3h knn_points: p2 has no points')
        idx = torch.empty(B, P, dtype=torch.int32, device=p1.device)
        dist = torch.empty(B, P, dtype=torch.float32, device=p1.device)
        for b in range(B):
            a, t = p1[b].detach().contiguous().float(), p2[b].detach().contiguous().float()
            L.call('knn1', a, P, t, t.shape[0], idx[b], dist[b])
        nn = None
        if return_nn:
            nn = torch.gather(p2, 1, idx.long()[..., None].expand(-1, -1, p2.shape[-1]))[:, :, None]
        return _KNN(dist[..., None], idx.long()[..., None], nn)
    lengths1 = _lengths(lengths1, B, P, p1.device, 'lengths1')
    lengths2 = _lengths(lengths2, B, p2.shape[1], p1.device, 'lengths2')
    dists, idx = _KnnPoints.apply(p1, p2, lengths1, lengths2, K)
    return _KNN(dists, idx, knn_gather(p2, idx, lengths2) if return_nn else None)


def knn_gather(x, idx, lengths=None):
    """x [N,M,U], idx [N,L,K] of knn_points -> [N,L,K,U] with out[n,l,k] = x[n, idx[n,l,k]]; slots k >= lengths[n] (a cloud with fewer than K
    points) are 0 (third_parties/pytorch3d/ops.py:209-259)"""
    if x.dim() != 3 or idx.dim() != 3:
        raise ValueError('x must be (N, M, U) and idx (N, L, K).')
    N, M, U = x.shape
    _N, Lq, K = idx.shape
    if N != _N:
        raise ValueError('x and idx must have same batch dimension.')
    out = torch.gather(x[:, :, None].expand(-1, -1, K, -1), 1, idx[..., None].expand(-1, -1, -1, U))
    if lengths is not None and int(lengths.min()) < K:
        dead = lengths.to(x.device)[:, None] <= torch.arange(K, device=x.device)[None]                 # [N,K]
        out = out.masked_fill(dead[:, None, :, None], 0.0)
    return out
