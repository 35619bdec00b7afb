"""Host side of csrc/denoise.hip: the cross-bilateral denoiser of render.optixutils (autograd).

bilateral_denoise(col [B,H,W,3], nrm [B,H,W,3], zdz [B,H,W,2], sigma) -> [B,H,W,4]: the weighted colour sum and max(sum of weights, 1e-4); the
caller divides.  Only col gets a gradient; the backward is the exact adjoint as a gather (no atomics: bit-reproducible)."""
import torch

from . import _lib as L


def _run(v, nrm, zdz, sigma, backward, channels):
    B, H, W = nrm.shape[:3]
    out = torch.empty(B, H, W, channels, dtype=torch.float32, device=nrm.device)
    L.check(L.lib().d3h_bilateral_denoise(L.ptr(v), L.ptr(nrm), L.ptr(zdz), L.i32(B), L.i32(H), L.i32(W), L.f32(sigma), L.i32(backward), L.ptr(out),
                                          L.stream()), 'bilateral_denoise_bwd' if backward else 'bilateral_denoise_fwd')
    return out


class _DenoiseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, col, nrm, zdz, sigma):
        if col.dim() != 4 or col.shape[-1] != 3 or nrm.shape != col.shape or tuple(zdz.shape) != (*col.shape[:3], 2):
            raise RuntimeError(f'bilateral_denoiser: expected col [B,H,W,3], nrm [B,H,W,3], zdz [B,H,W,2]; got {tuple(col.shape)}, {tuple(nrm.shape)}, '
                               f'{tuple(zdz.shape)}')
        if not float(sigma) > 0.0:
            raise RuntimeError(f'bilateral_denoiser: sigma must be positive, got {sigma}')
        c = lambda t: t.detach().float().contiguous()
        nrm, zdz = c(nrm), c(zdz)
        ctx.save_for_backward(nrm, zdz)
        ctx.sigma = float(sigma)
        return _run(c(col), nrm, zdz, sigma, 0, 4)

    @staticmethod
    def backward(ctx, g):
        nrm, zdz = ctx.saved_tensors
        return _run(g.contiguous().float(), nrm, zdz, ctx.sigma, 1, 3), None, None, None


def bilateral_denoise(col, nrm, zdz, sigma):
    return _DenoiseFn.apply(col, nrm, zdz, sigma)
