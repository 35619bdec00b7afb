"""Host side of csrc/bsdf.hip: the eight per-pixel BSDF functions of render.renderutils (autograd), and their torch compositions.

Every tensor input is [B,H,W,C] or broadcast along any of B / H / W (the stride-0 convention of csrc/d3h_bcast.h); inputs are made float32 and
contiguous here, outputs are float32.  The backward recomputes from the inputs, asks the kernel only for the gradients autograd needs
(`ctx.needs_input_grad`: the others are NULL pointers whose stores the kernel skips) and returns the gradient of a broadcast input in that
input's own shape: summed inside the kernel where the input is broadcast along H and W, by a torch sum over a full-resolution buffer otherwise.

The `py_*` functions are the same formulas as torch compositions (what `use_python=True` selects in render.renderutils).  They follow the
reference's python twins, render/renderutils/bsdf.py: cosines clamped to [1e-4, 1 - 1e-4], alpha to [min_roughness^2, 1], the front-facing
selects, F.normalize."""
import ctypes
import math

import torch

from . import _lib as L
from .imgops import _bc_strides

# op id of csrc/bsdf.hip -> (name, channels of each input, channels of the output)
_OPS = {
    0: ('_fresnel_shlick', (3, 3, 1), 3),
    1: ('_ndf_ggx', (1, 1), 1),
    2: ('_lambda_ggx', (1, 1), 1),
    3: ('_masking_smith', (1, 1, 1), 1),
    4: ('lambert', (3, 3), 1),
    5: ('frostbite_diffuse', (3, 3, 3, 1), 1),
    6: ('pbr_specular', (3, 3, 3, 3, 1), 3),
    7: ('pbr_bsdf', (3, 3, 3, 3, 3, 3), 3),
}


def _as4(t, c, name):
    while t.dim() < 4:
        t = t[None]
    if t.dim() != 4 or t.shape[-1] not in (1, c):
        raise RuntimeError(f'{name}: expected [B,H,W,{c}] or a broadcastable equivalent, got {tuple(t.shape)}')
    return t if t.shape[-1] == c else t.expand(*t.shape[:-1], c)


class _BsdfFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, op, min_roughness, frostbite, *ins):
        name, cin, cout = _OPS[op]
        ins4 = [_as4(t, c, name) for t, c in zip(ins, cin)]
        shp = [max(t.shape[k] for t in ins4) for k in range(3)]
        keep, strides = _bc_strides(ins4, shp, name)
        B, H, W = shp
        n = len(keep)
        out = torch.empty(B, H, W, cout, dtype=torch.float32, device=keep[0].device)
        L.call('bsdf_fwd', op, n, L.ptr_array(keep), strides, B, H, W, min_roughness, frostbite, out)
        ctx.save_for_backward(*keep)
        ctx.meta = (op, float(min_roughness), int(frostbite), shp, [tuple(t.shape) for t in ins])
        return out

    @staticmethod
    def backward(ctx, g):
        keep = list(ctx.saved_tensors)
        op, min_roughness, frostbite, shp, in_shapes = ctx.meta
        name, cin, _ = _OPS[op]
        B, H, W = shp
        n = len(keep)
        _, strides = _bc_strides(keep, shp, name)
        # an input broadcast along H and W (view_pos [B,1,1,3], light_pos [1,1,1,3]) is summed inside the kernel into a zeroed [B or 1,1,1,C]
        red = [int(H * W > 1 and t.shape[1] == 1 and t.shape[2] == 1) for t in keep]
        grads = [None if not ctx.needs_input_grad[3 + k] else L.zeros((keep[k].shape[0], 1, 1, c), torch.float32, g.device) if red[k]
                 else torch.empty(B, H, W, c, dtype=torch.float32, device=g.device) for k, c in enumerate(cin)]
        L.call('bsdf_bwd', op, n, L.ptr_array(keep), strides, B, H, W, min_roughness, frostbite, g.contiguous().float(), L.ptr_array(grads),
               (ctypes.c_int * n)(*red))
        outs = []
        for gr, shape in zip(grads, in_shapes):
            if gr is not None:
                gr = gr.sum_to_size((1,) * (4 - len(shape)) + shape).reshape(shape)
            outs.append(gr)
        return (None, None, None, *outs)


def fresnel_shlick(f0, f90, cosTheta):
    return _BsdfFn.apply(0, 0.0, 0, f0, f90, cosTheta)


def ndf_ggx(alphaSqr, cosTheta):
    return _BsdfFn.apply(1, 0.0, 0, alphaSqr, cosTheta)


def lambda_ggx(alphaSqr, cosTheta):
    return _BsdfFn.apply(2, 0.0, 0, alphaSqr, cosTheta)


def masking_smith(alphaSqr, cosThetaI, cosThetaO):
    return _BsdfFn.apply(3, 0.0, 0, alphaSqr, cosThetaI, cosThetaO)


def lambert(nrm, wi):
    return _BsdfFn.apply(4, 0.0, 0, nrm, wi)


def frostbite_diffuse(nrm, wi, wo, linearRoughness):
    return _BsdfFn.apply(5, 0.0, 0, nrm, wi, wo, linearRoughness)


def pbr_specular(col, nrm, wo, wi, alpha, min_roughness=0.08):
    return _BsdfFn.apply(6, min_roughness, 0, col, nrm, wo, wi, alpha)


def pbr_bsdf(kd, arm, pos, nrm, view_pos, light_pos, min_roughness=0.08, frostbite=False):
    return _BsdfFn.apply(7, min_roughness, int(bool(frostbite)), kd, arm, pos, nrm, view_pos, light_pos)


# ---- the same functions as torch compositions ---------------------------------------------------------------------------------------
EPS = 1e-4


def _dot(a, b):
    return (a * b).sum(-1, keepdim=True)


def _unit(x):
    return torch.nn.functional.normalize(x, dim=-1)


def _cos(c):
    return c.clamp(EPS, 1.0 - EPS)


def py_fresnel_shlick(f0, f90, cosTheta):
    return f0 + (f90 - f0) * (1.0 - _cos(cosTheta)) ** 5.0


def py_ndf_ggx(alphaSqr, cosTheta):
    c = _cos(cosTheta)
    d = (c * alphaSqr - c) * c + 1
    return alphaSqr / (d * d * math.pi)


def py_lambda_ggx(alphaSqr, cosTheta):
    c2 = _cos(cosTheta) ** 2
    return 0.5 * (torch.sqrt(1 + alphaSqr * (1.0 - c2) / c2) - 1.0)


def py_masking_smith(alphaSqr, cosThetaI, cosThetaO):
    return 1 / (1 + py_lambda_ggx(alphaSqr, cosThetaI) + py_lambda_ggx(alphaSqr, cosThetaO))


def py_lambert(nrm, wi):
    return _dot(nrm, wi).clamp(min=0.0) / math.pi


def py_frostbite_diffuse(nrm, wi, wo, linearRoughness):
    wi_n, wo_n = _dot(wi, nrm), _dot(wo, nrm)
    wi_h = _dot(wi, _unit(wo + wi))
    f90 = 0.5 * linearRoughness + 2.0 * wi_h * wi_h * linearRoughness
    res = py_fresnel_shlick(1.0, f90, wi_n) * py_fresnel_shlick(1.0, f90, wo_n) * (1.0 - (0.51 / 1.51) * linearRoughness)
    return torch.where((wi_n > 0.0) & (wo_n > 0.0), res, torch.zeros_like(res))


def py_pbr_specular(col, nrm, wo, wi, alpha, min_roughness=0.08):
    a2 = alpha.clamp(min_roughness * min_roughness, 1.0) ** 2
    h = _unit(wo + wi)
    wo_n, wi_n = _dot(wo, nrm), _dot(wi, nrm)
    w = py_fresnel_shlick(col, 1, _dot(wo, h)) * py_ndf_ggx(a2, _dot(nrm, h)) * py_masking_smith(a2, wo_n, wi_n) * 0.25 / wo_n.clamp(min=EPS)
    return torch.where((wo_n > EPS) & (wi_n > EPS), w, torch.zeros_like(w))


def py_pbr_bsdf(kd, arm, pos, nrm, view_pos, light_pos, min_roughness=0.08, frostbite=False):
    wo, wi = _unit(view_pos - pos), _unit(light_pos - pos)
    spec, rough, metal = arm[..., 0:1], arm[..., 1:2], arm[..., 2:3]
    ks = (0.04 * (1.0 - metal) + kd * metal) * (1 - spec)
    lobe = py_frostbite_diffuse(nrm, wi, wo, rough) if frostbite else py_lambert(nrm, wi)
    return kd * (1.0 - metal) * lobe + py_pbr_specular(ks, nrm, wo, wi, rough * rough, min_roughness)
