"""Host side of csrc/envshade.hip: ray-traced environment shading with multiple importance sampling (autograd).

env_shade(bvh, mask, ro, gb_pos, gb_normal, gb_view_pos, gb_kd, gb_ks, light, pdf, rows, cols, perms, BSDF, n_samples_x, seed, bwd_seed,
shadow_scale) -> (diff [B,H,W,3], spec [B,H,W,3]).  `bvh` is a d3h.raytrace.Bvh (shadow rays), `BSDF` 0 'pbr' / 1 'diffuse' / 2 'white', `perms`
[R, n_samples_x^2] int32.  The forward samples with `seed`, the backward re-runs the sampling with `bwd_seed` and recomputes everything: nothing is
saved but the inputs.  Gradients: gb_pos, gb_normal, gb_kd, gb_ks (plain stores; None for gb_pos, gb_kd, gb_ks in the two Lambert modes, where they
are zero) and light (float atomics per texel).  Sample directions, pdfs and visibility carry no gradient.  Inputs of any stride are made float32
and contiguous here (the reference passes rast[..., -1] as mask and lgt.rows[:, 0] as rows)."""
import torch

from . import _lib as L


def _prep(bvh, mask, gb, light, pdf, rows, cols, perms, n):
    B, H, W = gb[1].shape[:3]
    c = lambda t: t.detach().float().contiguous()
    mask = c(mask).reshape(-1)
    if mask.numel() != B * H * W:
        raise RuntimeError(f'env_shade: mask has {mask.numel()} elements for {B} x {H} x {W} pixels')
    gbuf = [mask] + [c(t) for t in gb]
    for t in gbuf[1:]:
        if tuple(t.shape) != (B, H, W, 3):
            raise RuntimeError(f'env_shade: expected [B,H,W,3] g-buffer tensors, got {tuple(t.shape)}')
    light, pdf, rows, cols = c(light), c(pdf), c(rows).reshape(-1), c(cols)
    if light.dim() != 3 or light.shape[-1] != 3 or pdf.dim() != 2 or cols.shape != pdf.shape or rows.numel() != pdf.shape[0]:
        raise RuntimeError(f'env_shade: expected light [h,w,3], pdf [H,W], rows [H], cols [H,W]; got {tuple(light.shape)}, {tuple(pdf.shape)}, '
                           f'{tuple(rows.shape)}, {tuple(cols.shape)}')
    perms = perms.detach().contiguous()
    if perms.dtype != torch.int32 or perms.dim() != 2 or perms.shape[0] < 1 or perms.shape[1] != n * n:
        raise RuntimeError(f'env_shade: perms must be int32 [R >= 1, {n * n}], got {perms.dtype} {tuple(perms.shape)}')
    head = [bvh.nodes, bvh.tri9, bvh.F, L.ptr_array(gbuf), light, light.shape[0], light.shape[1], pdf, rows, cols, pdf.shape[0], pdf.shape[1], perms,
            perms.shape[0], B * H * W]
    return (B, H, W), light, head


class _EnvShadeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bvh, mask, ro, gb_pos, gb_normal, gb_view_pos, gb_kd, gb_ks, light, pdf, rows, cols, perms, BSDF, n, seed, bwd_seed, shadow_scale):
        (B, H, W), _, head = _prep(bvh, mask, (ro, gb_pos, gb_normal, gb_view_pos, gb_kd, gb_ks), light, pdf, rows, cols, perms, n)
        dev = gb_pos.device
        diff = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
        spec = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
        L.call('env_shade_fwd', *head, BSDF, n, seed & 0xffffffff, shadow_scale, diff, spec)
        ctx.save_for_backward(mask, ro, gb_pos, gb_normal, gb_view_pos, gb_kd, gb_ks, light, pdf, rows, cols, perms)
        ctx.meta = (bvh, int(BSDF), int(n), int(bwd_seed), float(shadow_scale))
        return diff, spec

    @staticmethod
    def backward(ctx, g_diff, g_spec):
        mask, ro, gb_pos, gb_normal, gb_view_pos, gb_kd, gb_ks, light, pdf, rows, cols, perms = ctx.saved_tensors
        bvh, BSDF, n, seed, shadow_scale = ctx.meta
        (B, H, W), light_c, head = _prep(bvh, mask, (ro, gb_pos, gb_normal, gb_view_pos, gb_kd, gb_ks), light, pdf, rows, cols, perms, n)
        dev = gb_pos.device
        new = lambda: torch.empty(B, H, W, 3, dtype=torch.float32, device=dev)
        d_nrm = new()
        d_pos, d_kd, d_ks = (new(), new(), new()) if BSDF == 0 else (None, None, None)
        d_light = L.zeros(tuple(light_c.shape), torch.float32, dev)
        L.call('env_shade_bwd', *head, BSDF, n, seed & 0xffffffff, shadow_scale, g_diff.contiguous().float(), g_spec.contiguous().float(), d_pos,
               d_nrm, d_kd, d_ks, d_light)
        fit = lambda d, t: None if d is None else d.reshape(t.shape)
        return (None, None, None, fit(d_pos, gb_pos), fit(d_nrm, gb_normal), None, fit(d_kd, gb_kd), fit(d_ks, gb_ks), d_light.reshape(light.shape),
                None, None, None, None, None, None, None, None, None)


def env_shade(bvh, mask, ro, gb_pos, gb_normal, gb_view_pos, gb_kd, gb_ks, light, pdf, rows, cols, perms, BSDF, n_samples_x, seed, bwd_seed, shadow_scale):
    if BSDF not in (0, 1, 2):
        raise RuntimeError(f'env_shade: BSDF must be 0 (pbr), 1 (diffuse) or 2 (white), got {BSDF}')
    if int(n_samples_x) < 1:
        raise RuntimeError(f'env_shade: n_samples_x must be >= 1, got {n_samples_x}')
    return _EnvShadeFn.apply(bvh, mask, ro, gb_pos, gb_normal, gb_view_pos, gb_kd, gb_ks, light, pdf, rows, cols, perms, int(BSDF), int(n_samples_x), int(seed),
                             int(bwd_seed), float(shadow_scale))
