"""Generate tests/golden/renderutils_bsdf.npz: the reference's python twins of the per-pixel BSDF functions (render/renderutils/bsdf.py, loaded
by path: pure torch, runs on the CPU) on seeded inputs.  Dev container only; only DATA is stored.

Run: python tools/gen_golden_renderutils.py

For each of the eight functions (pbr_bsdf in both of its modes) the file holds, under '<case>.':
  in.<name>   the float32 inputs
  gout        a seeded random cotangent (float32, the output's shape)
  out         the twin's float64 output on those inputs
  d.<name>    the twin's float64 input gradients under that cotangent
  ref32_err   the largest max|f32 twin - f64 twin| / max|f64| over the output and the gradients: the reference's own float32 distance

Inputs: B, H, W = 2, 5, 13 (130 pixels: two full waves and a ragged tail of two, odd W).  nrm / wi / wo are unit vectors, wi and wo drawn as
normalize(0.6 nrm + unit), so roughly a third of them lie on the back side; alpha uniform in [0, 1.1] (both clamps are hit), cosTheta uniform
in [-0.2, 1.2], pos in [-0.5, 0.5]^3, view_pos [2,1,1,3] and light_pos [1,1,1,3] (broadcast)."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import refharness                                     # noqa: E402

B, H, W = 2, 5, 13
OUT = os.path.join(ROOT, 'tests', 'golden', 'renderutils_bsdf.npz')


def load_twins():
    spec = importlib.util.spec_from_file_location('ref_renderutils_bsdf', os.path.join(refharness.REF, 'render', 'renderutils', 'bsdf.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def make_inputs(gen):
    u = lambda *s, lo=0.0, hi=1.0: torch.rand(*s, generator=gen) * (hi - lo) + lo
    unit = lambda *s: torch.nn.functional.normalize(torch.randn(*s, generator=gen), dim=-1)
    full = (B, H, W)
    nrm = unit(*full, 3)
    toward = lambda: torch.nn.functional.normalize(0.6 * nrm + unit(*full, 3), dim=-1)
    cos = lambda: u(*full, 1, lo=-0.2, hi=1.2)
    pos = u(*full, 3, lo=-0.5, hi=0.5)
    view_pos = u(B, 1, 1, 3, lo=-1.0, hi=1.0) + torch.tensor([0.0, 0.0, 3.0])
    light_pos = u(1, 1, 1, 3, lo=-1.0, hi=1.0) + torch.tensor([0.0, 2.5, 1.0])
    # pbr_bsdf: a normal drawn around the light direction, so that about a third of the pixels face away from the light or the camera
    nrm_l = torch.nn.functional.normalize(0.6 * torch.nn.functional.normalize(light_pos - pos, dim=-1) + unit(*full, 3), dim=-1)
    pbr = {'kd': u(*full, 3), 'arm': u(*full, 3, hi=1.05), 'pos': pos, 'nrm': nrm_l, 'view_pos': view_pos, 'light_pos': light_pos}
    return {
        'fresnel_shlick': {'f0': u(*full, 3), 'f90': u(*full, 3), 'cosTheta': cos()},
        'ndf_ggx': {'alphaSqr': u(*full, 1, lo=0.01), 'cosTheta': cos()},
        'lambda_ggx': {'alphaSqr': u(*full, 1, lo=0.01), 'cosTheta': cos()},
        'masking_smith': {'alphaSqr': u(*full, 1, lo=0.01), 'cosThetaI': cos(), 'cosThetaO': cos()},
        'lambert': {'nrm': nrm, 'wi': toward()},
        'frostbite': {'nrm': nrm, 'wi': toward(), 'wo': toward(), 'linearRoughness': u(*full, 1)},
        'pbr_specular': {'col': u(*full, 3), 'nrm': nrm, 'wo': toward(), 'wi': toward(), 'alpha': u(*full, 1, hi=1.1)},
        'pbr_bsdf_lambert': pbr,
        'pbr_bsdf_frostbite': pbr,
    }


def twin_fn(m, case):
    return {
        'fresnel_shlick': m.bsdf_fresnel_shlick, 'ndf_ggx': m.bsdf_ndf_ggx, 'lambda_ggx': m.bsdf_lambda_ggx,
        'masking_smith': m.bsdf_masking_smith_ggx_correlated, 'lambert': m.bsdf_lambert, 'frostbite': m.bsdf_frostbite,
        'pbr_specular': lambda *a: m.bsdf_pbr_specular(*a, min_roughness=0.08),
        'pbr_bsdf_lambert': lambda *a: m.bsdf_pbr(*a, 0.08, 0),
        'pbr_bsdf_frostbite': lambda *a: m.bsdf_pbr(*a, 0.08, 1),
    }[case]


def run(fn, ins, gout, dtype):
    leaves = [v.to(dtype).clone().requires_grad_(True) for v in ins.values()]
    out = fn(*leaves)
    grads = torch.autograd.grad(out, leaves, gout.to(dtype))
    return out.detach(), [g.detach() for g in grads]


def main():
    m = load_twins()
    gen = torch.Generator().manual_seed(20240607)
    res = {}
    for case, ins in make_inputs(gen).items():
        fn = twin_fn(m, case)
        with torch.no_grad():
            shape = fn(*ins.values()).shape
        gout = torch.randn(*shape, generator=gen)
        o64, g64 = run(fn, ins, gout, torch.float64)
        o32, g32 = run(fn, ins, gout, torch.float32)
        err = max(((a.double() - b).abs().max() / b.abs().max()).item() for a, b in zip([o32] + g32, [o64] + g64))
        assert all(torch.isfinite(t).all() for t in [o64] + g64)
        assert err < 1e-5, f'{case}: the float32 and float64 twins are {err:.2e} apart: a branch flipped between the precisions; re-seed'
        for k, v in ins.items():
            res[f'{case}.in.{k}'] = v.numpy()
        res[f'{case}.gout'] = gout.numpy()
        res[f'{case}.out'] = o64.numpy()
        for k, g in zip(ins, g64):
            res[f'{case}.d.{k}'] = g.numpy()
        res[f'{case}.ref32_err'] = np.float64(err)
        print(f'{case:20s} out {tuple(shape)}  zero rows {int((o64.abs().sum(-1) == 0).sum())}/{B * H * W}  ref32_err {err:.2e}')
    np.savez_compressed(OUT, **res)
    size = os.path.getsize(OUT)
    assert size <= 512 * 1024, size
    print('wrote', OUT, size, 'bytes')


if __name__ == '__main__':
    main()
