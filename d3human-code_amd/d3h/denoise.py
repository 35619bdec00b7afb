"""Host side of csrc/denoise.hip: the cross-bilateral denoiser of render.optixutils (autograd).

bilateral_denoise(col [B,H,W,3], nrm [B,H,W,3], zdz [B,H,W,2], sigma) -> [B,H,W,4]: the weighted colour sum and max(sum of weights, 1e-4); the
caller divides.  Only col gets a gradient; the backward is the exact adjoint as a gather (no atomics: bit-reproducible).

bilateral_denoise_many([col_a, col_b], nrm, zdz, sigma) -> the same for one or two images that share the guides (the demodulated path: diffuse and
specular light), one launch each way: the guide planes are staged and the tap weights computed once.  Each image's output and gradient equal the
single-image call's bit for bit."""
import torch

from . import _lib as L


def _run(v, nrm, zdz, sigma, backward, channels):
    B, H, W = nrm.shape[:3]
    out = torch.empty(B, H, W, channels, dtype=torch.float32, device=nrm.device)
    L.call('bilateral_denoise', v, nrm, zdz, B, H, W, sigma, backward, out)
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


def _check(col, nrm, zdz, sigma):
    if col.dim() != 4 or col.shape[-1] != 3 or nrm.shape != col.shape or tuple(zdz.shape) != (*col.shape[:3], 2):
        raise RuntimeError(f'bilateral_denoiser: expected col [B,H,W,3], nrm [B,H,W,3], zdz [B,H,W,2]; got {tuple(col.shape)}, {tuple(nrm.shape)}, '
                           f'{tuple(zdz.shape)}')
    if not float(sigma) > 0.0:
        raise RuntimeError(f'bilateral_denoiser: sigma must be positive, got {sigma}')


def _run_n(vs, nrm, zdz, sigma, backward, channels):
    B, H, W = nrm.shape[:3]
    outs = [torch.empty(B, H, W, channels, dtype=torch.float32, device=nrm.device) for _ in vs]
    L.call('bilateral_denoise_n', L.ptr_array(vs), len(vs), nrm, zdz, B, H, W, sigma, backward, L.ptr_array(outs))
    return outs


class _DenoiseManyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nrm, zdz, sigma, *cols):
        for col in cols:
            _check(col, nrm, zdz, sigma)
        c = lambda t: t.detach().float().contiguous()
        nrm, zdz = c(nrm), c(zdz)
        ctx.save_for_backward(nrm, zdz)
        ctx.sigma = float(sigma)
        return tuple(_run_n([c(col) for col in cols], nrm, zdz, sigma, 0, 4))

    @staticmethod
    def backward(ctx, *gs):
        nrm, zdz = ctx.saved_tensors
        return (None, None, None, *_run_n([g.contiguous().float() for g in gs], nrm, zdz, ctx.sigma, 1, 3))


def bilateral_denoise_many(cols, nrm, zdz, sigma):
    cols = list(cols)
    if len(cols) not in (1, 2):
        raise RuntimeError(f'bilateral_denoiser: one or two images share a set of guides, got {len(cols)}')
    return list(_DenoiseManyFn.apply(nrm, zdz, sigma, *cols))
