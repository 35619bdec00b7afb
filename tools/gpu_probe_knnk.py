"""Stand-alone times of the K-nearest search and the K-blended skinning on the GPU, beside their K = 1 counterparts in the same run
(orientation only: DESIGN.md §3, profiles/knnk_kernel_times.txt).

    python tools/gpu_probe_knnk.py [points] [vertices] [frames]        # defaults 50000 10475 4

Ellipsoid-shell template, queries within a few cell widths of it (what an extracted surface is to the SMPL-X template), skin-weight rows
with 4 non-zeros of 55.  Every entry is warmed up, then timed with device events over `REPS` launches behind one synchronise."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'd3human-code_amd'))
from d3h import lbs as HL        # noqa: E402

REPS = 50


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS * 1e3       # us per call


def main():
    P, V, B = (int(v) for v in (sys.argv[1:4] + ['50000', '10475', '4'][len(sys.argv) - 1:]))
    dev = 'cuda'
    g = torch.Generator().manual_seed(0)
    u = torch.randn(V, 3, generator=g)
    tmpl = (u / u.norm(dim=1, keepdim=True) * torch.tensor([0.3, 0.8, 0.2])).to(dev).contiguous()
    pts = (tmpl[torch.randint(0, V, (P,), generator=g).to(dev)] + 0.02 * torch.randn(P, 3, generator=g).to(dev)).contiguous()
    W = torch.zeros(V, 55)
    W.scatter_(1, torch.randint(0, 55, (V, 4), generator=g), torch.rand(V, 4, generator=g) + 0.1)
    W = (W / W.sum(1, keepdim=True)).to(dev).contiguous()

    def rigid(n):
        q, _ = torch.linalg.qr(torch.eye(3) + 0.2 * torch.randn(n, 3, 3, generator=g))
        A = torch.zeros(n, 4, 4)
        A[:, :3, :3], A[:, :3, 3], A[:, 3, 3] = q, 0.1 * torch.randn(n, 3, generator=g), 1.0
        return A
    A0 = rigid(55).to(dev)
    A = torch.stack([rigid(55) for _ in range(B)]).to(dev).requires_grad_(True)
    trans = torch.zeros(B, 3, device=dev, requires_grad=True)
    gout = torch.randn(B, P, 3, generator=g).to(dev)
    grid = HL.KnnGrid(tmpl)
    print(f'{P} points x {V} vertices x {B} frames; us per call, mean of {REPS} (device events); forward+backward = one autograd round trip '
          f'(the two kernels, the frame sum and the host code between them)')
    rows = []
    for K in (1, 2, 4, 8):
        if K == 1:
            t_grid = timed(lambda: grid.query(pts))
            t_full = timed(lambda: HL.knn1(pts, tmpl))
            nn = grid.query(pts)
            fwd = lambda p: HL.lbs_points(p, nn, W, A0, A, trans)
        else:
            t_grid = timed(lambda: grid.query_k(pts, K))
            t_full = timed(lambda: HL.knnk(pts, tmpl, K))
            nn = grid.query_k(pts, K)
            fwd = lambda p: HL.lbs_points_k(p, nn, W, tmpl, A0, A, trans)
        with torch.no_grad():
            t_fwd = timed(lambda: fwd(pts))

        def both():
            p = pts.detach().requires_grad_(True)
            (fwd(p) * gout).sum().backward()
        t_both = timed(both)
        rows.append((K, t_grid, t_full, t_fwd, t_both))
        print(f'K={K}: grid search {t_grid:8.1f}   exhaustive search {t_full:8.1f}   skinning forward {t_fwd:8.1f}   forward+backward(+loss) {t_both:8.1f}')
    return rows


if __name__ == '__main__':
    assert torch.cuda.is_available(), 'needs the GPU'
    main()
