"""The image-space loss kernels of csrc/image_ops.hip -- pixel_losses_fwd/bwd (+ finish), seq_losses_fwd/bwd, image_loss_fwd/bwd and the
sliding-window SSIM pair with its occupancy cells -- against FLOAT64, per element and at their edges.  Shared by tests/test_loss64_emul.py
(host emulation) and tests/test_gpu_loss64.py (MI355X).  The measured tables: profiles/loss64_emul.md, profiles/loss64_gpu.md
(`python tests/loss64_cases.py cpu|cuda` prints them).

The references.  The torch compositions of parity_cases.check_pixel_losses / check_seq_losses (restated here with the layout as a parameter),
evaluated on the float32 inputs (r32) and on their float64 copies (r64), with two pieces replaced:
  * SSIM is oracle.image_ops.ssim with the KERNEL'S 11 weights (kernel_window(): (float)exp(double), a sequential float sum, a float divide, as
    ssim_window() in csrc/image_ops.hip) handed to both references, and C1, C2 the float32 products 0.01f 0.01f, 0.03f 0.03f widened.  The
    oracle's own float32 window differs from the kernel's by up to 1.1e-7 relative per weight; neither is wrong, and a test that lets them
    differ measures the window.  The distance to a float64 run with the EXACTLY normalised window is recorded without a bar.
  * the image loss is ImgLoss, a torch.autograd.Function in the dtype of its inputs: forward loss.cu:31-37,95-131, backward loss.cu:38-62
    AS WRITTEN -- the float constants 0.439583f and 0.583333f (widened), a gradient under log_srgb only strictly inside (0, 65535),
    sign(0) = 0 for l1 and smape, and without a tone mapper the gradient passes through the clamp.  The six-digit constants are up to
    7.6e-7 + 3.4e-7 |ln x| <= 2.7e-6 relative away from the analytic derivative for x = log(a + 1) in [0.0031308, 11.1], so float64 autograd
    of the forward is the wrong reference for the small-gradient bands; check_restated_backward holds the two to 3e-6 per element (host only).
Never a comparison with an earlier output of the kernel, except where two ROUTES must agree bit for bit (occupancy cells against none: d_a on
both devices; the SSIM sum on the emulation only -- it is one float atomic per workgroup, whose order is fixed there and not on the GPU, where
the sums of both routes are each held to (b)).

(a) Per-element tensors, one thread per element, no atomics -- d_st of pixel_losses and seq_losses, d_img and d_tgt of image_loss, d_a and
    d_b of ssim, the `masked` output:
        |kernel - r64|_2  <=  RATIO |r32 - r64|_2,   RATIO = 3,
    per tensor of every run, and per DECADE BAND of |r64| pooled over the runs of a group (MIN_BAND = 64, the joining rule of
    mtets64_cases.merged_bands).  No absolute floor.  A tensor of fewer than MIN_BAND elements is pooled only.  The loss weights and the
    per-pixel weights on `masked` carry factors 10^k, k uniform in -6..2.  Exactly zero: the channels of d_st no loss reads, d_st of the
    rgb channels where ref.a == 0, d_a of an image whose occupancy cells are all empty.  Under prep = () `masked` is shaded.rgb ref.a bit
    for bit.
(b) The scalar sums (the ten entries of pixel_losses, the six of seq_losses, the image_loss value, the SSIM sum):
        |kernel - r64|  <=  scale ( L 2^-24 sum_p |term_p|  +  sum_p form_p ),
    terms in float64.  L counts the roundings that act on PARTIAL SUMS, each at most 2^-24 of sum |term|:
        the grid-stride trips of one thread (ceil(npix / (256 grid)); SSIM: the 32 rows of a wave's band)
      + block_sum: 6 shuffle steps of wave_sum, 3 adds of the four wave totals
      + the workgroup totals: pixel_losses_finish_kernel adds ceil(grid / 256) partials per thread and runs block_sum again (+ 9); the other
        three add one float atomic per workgroup (+ grid)
      + 1 for the mean factor the wrapper multiplies in.
    form_p is the rounding error of FORMING term p, first order, evaluated in float64.  It is not a fixed number of ulps of |term_p|: a
    term is a difference of rounded operands (|a - t| of two tone-mapped colours, E[x^2] - E[x]^2 of SSIM), so its error keeps the size of
    the operands.  Per operand: a product px ref.a rounds once; log(a + 1) inherits the rounding of a + 1 (2^-24 absolute, whatever a is);
    the tone map then has error delta(A) = 2^-24 [14 (1 + e) + (E_POW + E_LOG + 4) (A + 0.055)] (12.92 is the largest slope of the sRGB
    curve, e the roundings in front of the clamp).  E_LOG and E_POW, in units of 2^-24 relative, are TWICE the largest error measured
    for logf over [1, 65536] and powf(x, 1 / 2.4f), powf(x, 0.583333f) over [0.0031308, 11.1] on either device (measured, not quoted from a
    table: measure_log_pow does it, profiles/loss64_*.md record the figures, and a test on each device asserts 2 x measured <= used).
    SSIM: each second moment carries 23 (+ 2 e) roundings over non-negative addends, each mean 22 (+ e), so v11 = E[a a] - mu1^2 is off by
    up to 69 2^-24 E[a a]: ssim_forms propagates that through (A1 A2) / (B1 B2).  At mean 0.95 this a-priori figure is ~1e-2 of the term:
    that is what the formula permits in float32, and the table shows how little of it the kernel uses.
    Power: where a case says so, the float64 terms of every workgroup's 256 pixels (every wave's SSIM band) sum to more than the bound, so a
    dropped workgroup or band cannot pass.  Asserted on the float64 terms of the non-negative sums.
(c) Exceptions to RATIO by name in TENSOR_RATIO / BAND_RATIO: tensor, band, the figures of both devices, the reason; the bar is the largest
    measured figure x 1.5 and the float32 yardstick is never rescaled.

Input hygiene (asserted on the inputs, no tolerance of a comparison): no tone-mapped operand has log(a + 1) within 1e-5 relative of
0.0031308 nor a product within 1e-5 of 65535 unless exactly there; for l1 and smape a pair is bit-identical or differs by >= 1e-4 relative
after the map, in float32 and in float64; normals are exactly zero or have |n| >= 1e-15 and stay 1 % away from both epsilons.  Nothing
is masked out of a comparison.
"""
import ctypes
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from parity_cases import T                     # noqa: F401  (first: through conftest it puts the repository root on sys.path when this file runs as a script)
from mtets64_cases import MIN_BAND, ZERO_BAND, merged_bands
from oracle import image_ops as O

RATIO = 3.0
U = 2.0 ** -24
E_LOG = 5.2           # units of 2^-24 relative, 2 x the largest measured: logf 2.578 on the MI355X, 1.176 on the emulation (measure_log_pow)
E_POW = 4.1           # powf: 2.007 on the MI355X, 0.996 on the emulation
TENSOR_RATIO = {}     # (group, tensor) -> bar                        (c), per tensor of a run: none
# (c), per pooled band only, keyed (group, tensor) -> (highest decades of the bands, bar, measured); every other band and every tensor of a run keeps 3.
# Both are sums that cancel to (nearly) nothing, of which kernel and float32 reference return the rounding noise of their own order of the adds;
# a handful of elements decides the band.  Bars: the largest measured figure x 1.5; the float32 yardstick is not rescaled.
#   pixel, d_st, the band of |r64| == 0: the gradient of the normal terms where the reference normal is exactly zero and the geometric normal
#     is not.  The upstream gradient is then parallel to the unit normal o and its projection (I - o o^T) g / |n| is o (1 - |o|^2) / |n|:
#     exactly 0 in float64, 2^-24 |g| / |n| of noise in float32 with |n| down to 2e-12.  One element of `pixel npix256 full nref3 l1/log_srgb
#     ssim` holds -93.1 in the kernel and 0.0 in torch's float32 (which in turn holds 8.0 where the kernel holds 0.0 elsewhere).
#   occ, d_a, the band 1e-18 .. 1e-14: gradients ten pixels away from a single lit pixel, where the filtered moment gradients (terms of
#     +-1e3 mu) change sign; 40 of its elements come from `occ 200x400 centre hand`, the worst -4.8e-15 with the kernel 1.7e-19 and the
#     float32 reference 2.7e-20 away.
BAND_RATIO = {('pixel', 'd_st'): ((ZERO_BAND,), 9.9, 'MI355X 6.59, emulation 6.59 (1 572 561 elements)'),
              ('occ', 'd_a'): ((-15,), 7.9, 'MI355X 5.28 (104 elements), emulation 5.28 (81 elements)')}
MEASURED = {}

BANDS = {}            # (dev, group) -> {tensor: {decade: [count, sum (k - r64)^2, sum (r32 - r64)^2, sum r64^2]}}
DONE = {}             # (dev, group, tensor) -> run tags pooled so far
FRACTION = {}         # (dev, tag, scalar) -> |kernel - r64| / bound of rule (b)
COMPLETE = set()      # (dev, group, tag)
_REF = {}

f32c = lambda v: float(np.float32(v))
KNEE, INV24, S1055, S0055, S1292 = f32c(0.0031308), float(np.float32(1.0) / np.float32(2.4)), f32c(1.055), f32c(0.055), f32c(12.92)
B439, B583 = f32c(0.439583), f32c(0.583333)
EPS_SMAPE, EPS_RELMSE, HDR = f32c(0.01), f32c(0.1), 65535.0
SSIM_C1 = float(np.float32(0.01) * np.float32(0.01))
SSIM_C2 = float(np.float32(0.03) * np.float32(0.03))
LOSSES, TONES = ('l1', 'mse', 'smape', 'relmse'), ('none', 'log_srgb')
SHIFT, SCALE = [-.030, -.088, -.188], [.458, .448, .450]                   # lpips.py's ScalingLayer


def _seed(*a):
    return zlib.crc32('/'.join(str(x) for x in a).encode())


def _gen(*a):
    return torch.Generator().manual_seed(_seed(*a))


def _decades(shape, gen):
    """factors 10^k, k uniform in -6..2"""
    return (10.0 ** (torch.rand(shape, generator=gen, dtype=torch.float64) * 8 - 6)).float()


def kernel_window():
    """the 11 weights of ssim_window() (csrc/image_ops.hip), operation for operation, in numpy float32"""
    w = np.exp(-((np.arange(11) - 5) ** 2).astype(np.float64) / (2.0 * 1.5 * 1.5)).astype(np.float32)
    s = np.float32(0.0)
    for x in w:
        s = np.float32(s + x)
    return (w / s).astype(np.float32)


def exact_window():
    g = np.exp(-((np.arange(11) - 5) ** 2).astype(np.float64) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


WIN = kernel_window()


# ---- rule (a) --------------------------------------------------------------------------------------------------------------------------------
def _bands(dev, group, tensor, dk, d32, r64):
    acc = BANDS.setdefault((dev, group), {}).setdefault(tensor, {})
    a = np.abs(r64)
    dec = np.full(a.shape, ZERO_BAND, np.int64)
    dec[a > 0] = np.floor(np.log10(a[a > 0])).astype(np.int64)
    for b in np.unique(dec):
        m = dec == b
        row = acc.setdefault(int(b), [0, 0.0, 0.0, 0.0])
        row[0] += int(m.sum())
        row[1] += float((dk[m] ** 2).sum())
        row[2] += float((d32[m] ** 2).sum())
        row[3] += float((r64[m] ** 2).sum())


def _compare(dev, group, tag, tensor, k, r32, r64, report):
    assert tuple(k.shape) == tuple(r64.shape) == tuple(r32.shape), (tag, tensor, tuple(k.shape), tuple(r64.shape))
    k, r32, r64 = (t.detach().cpu().double().reshape(-1).numpy() for t in (k, r32, r64))
    assert np.isfinite(k).all(), (tag, tensor, 'not finite')
    assert np.isfinite(r64).all() and np.isfinite(r32).all(), (tag, tensor, 'the reference is not finite')
    dk, d32 = k - r64, r32 - r64
    nk, n32, n64 = float(np.linalg.norm(dk)), float(np.linalg.norm(d32)), float(np.linalg.norm(r64))
    ratio = nk / n32 if n32 > 0 else (0.0 if nk == 0 else float('inf'))
    rel = (lambda x: x / n64) if n64 > 0 else (lambda x: x)
    alone = k.size >= MIN_BAND
    report(f'[loss64] {dev:4s} {tag:58s} {tensor:7s} e_k {rel(nk):.3e} e_32 {rel(n32):.3e} ratio {ratio:.2f}' +
           ('' if n64 > 0 else ' (|r64| = 0: absolute)') + ('' if alone else ' (pooled only)'))
    if tag not in DONE.setdefault((dev, group, tensor), set()):
        DONE[(dev, group, tensor)].add(tag)
        _bands(dev, group, tensor, dk, d32, r64)
    if alone:
        assert nk <= TENSOR_RATIO.get((group, tensor), RATIO) * n32, (tag, tensor, nk, n32, ratio)


def band_bar(group, tensor, top):
    exc = BAND_RATIO.get((group, tensor))
    return exc[1] if exc is not None and top in exc[0] else RATIO


def _top_decades(acc):
    """the highest decade of every band merged_bands returns, in its order"""
    rows = [[[b], acc[b][0]] for b in sorted(acc)]
    i = 0
    while len(rows) > 1 and i < len(rows):
        if rows[i][1] >= MIN_BAND:
            i += 1
            continue
        j = i + 1 if i + 1 < len(rows) else i - 1
        rows[j] = [sorted(rows[j][0] + rows[i][0]), rows[j][1] + rows[i][1]]
        del rows[i]
    return [r[0][-1] for r in rows]


def check_bands(dev, group, report=print):
    acc = BANDS.get((dev, group))
    assert acc, f'no run of group {group} recorded on {dev}'
    worst = []
    for tensor in sorted(acc):
        merged, tops = merged_bands(acc[tensor]), _top_decades(acc[tensor])
        assert len(tops) == len(merged)
        for (label, (n, sk, s32, s64)), top in zip(merged, tops):
            ratio = (sk / s32) ** 0.5 if s32 > 0 else (0.0 if sk == 0 else float('inf'))
            den = s64 ** 0.5 if s64 > 0 else 1.0
            bar = band_bar(group, tensor, top)
            report(f'[loss64] {dev:4s} band {group:10s} {tensor:7s} |r64| in {label:18s} n {n:8d} e_k {sk ** 0.5 / den:.3e} e_32 {s32 ** 0.5 / den:.3e} ratio {ratio:.2f} bar {bar:g}')
            if bar != RATIO:
                MEASURED[(dev, group, tensor, label)] = ratio
            if n >= MIN_BAND and sk > bar ** 2 * s32:
                worst.append((tensor, label, n, ratio, bar))
    assert not worst, worst


# ---- rule (b) --------------------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def chain_pixel(npix):
    grid = min(_cdiv(npix, 256), 2048)                  # d3h_pixel_losses_fwd
    return _cdiv(npix, 256 * grid) + 9 + _cdiv(grid, 256) + 9 + 1


def chain_seq(npix):
    grid = min(_cdiv(npix, 256), 1024)                  # d3h_seq_losses_fwd
    return _cdiv(npix, 256 * grid) + 9 + grid + 1


def chain_image(npix):
    grid = min(max(_cdiv(npix, 256), 1), 2048)          # d3h_grid
    return _cdiv(npix, 256 * grid) + 9 + grid + 1


def chain_ssim(N, H, W):
    return 32 + 9 + _cdiv(W, 64) * _cdiv(H, 128) * N + 1


def _scalar(dev, tag, name, k, r64, terms, forms, L, scale, report, power=None):
    """rule (b) for one mean.  terms, forms: float64 per pixel; power: None, or the float64 |sum of terms| of the smallest workgroup / band"""
    k, r64 = float(k.detach()) if torch.is_tensor(k) else float(k), float(r64)
    assert math.isfinite(k), (tag, name, 'not finite')
    bound = scale * (L * U * float(terms.abs().sum()) + float(forms.sum()))
    err = abs(k - r64)
    frac = err / bound if bound > 0 else (0.0 if err == 0 else float('inf'))
    FRACTION[(dev, tag, name)] = frac
    report(f'[loss64] {dev:4s} {tag:58s} {name:11s} scalar sum: value {r64:.9e} |kernel - r64| {err:.3e} bound {bound:.3e} fraction {frac:.4f} L {L}' +
           ('' if power is None else f' smallest-unit / bound {scale * power / bound if bound > 0 else float("inf"):.3g}'))
    assert err <= bound, (tag, name, k, r64, err, bound)
    if power is not None:
        assert scale * power > bound, (tag, name, 'a dropped workgroup / band would pass: the case shows nothing', scale * power, bound)


def block_power(terms):
    """smallest |sum| of the float64 terms over a workgroup's 256 consecutive pixels (full workgroups only; None without one)"""
    t = terms.reshape(-1)
    full = t.numel() // 256
    return float(t[:full * 256].reshape(full, 256).sum(1).abs().min()) if full else None


def band_power(vmap):
    """smallest |sum| of the float64 SSIM map over one wave's band (32 rows x 64 columns of a plane); vmap [N,H,W]"""
    N, H, W = vmap.shape
    p = F.pad(vmap, (0, (-W) % 64, 0, (-H) % 32))
    s = p.reshape(N, p.shape[1] // 32, 32, p.shape[2] // 64, 64).sum((2, 4))
    return float(s.abs().min())


# ---- logf / powf -----------------------------------------------------------------------------------------------------------------------------
def measure_log_pow(dev, n=20000):
    """largest relative error, in units of 2^-24, of the float32 log over [1, 65536] and pow(x, 1 / 2.4f), pow(x, 0.583333f) over [0.0031308, 11.1]
    against float64: on the emulation the C library's logf / powf the host build of the kernels calls; on the GPU torch's float32 log / pow,
    which hipcc builds on the device library's logf / powf as it does for csrc/image_ops.hip (same compiler, no fast-math on either)"""
    gen = _gen('logpow')
    xs = torch.exp(torch.rand(n, generator=gen, dtype=torch.float64) * math.log(65536.0)).float()
    ps = torch.exp(torch.rand(n, generator=gen, dtype=torch.float64) * math.log(11.1 / 0.0031308) + math.log(0.0031308)).float()
    if dev == 'cpu':
        m = ctypes.CDLL('libm.so.6')
        m.logf.restype = m.powf.restype = ctypes.c_float
        m.logf.argtypes, m.powf.argtypes = [ctypes.c_float], [ctypes.c_float, ctypes.c_float]
        lg = torch.tensor([m.logf(float(x)) for x in xs], dtype=torch.float64)
        pw = [torch.tensor([m.powf(float(x), e) for x in ps], dtype=torch.float64) for e in (INV24, B583)]
    else:
        lg = torch.log(xs.to(dev)).cpu().double()
        pw = [torch.pow(ps.to(dev), e).cpu().double() for e in (INV24, B583)]
    rl = lambda got, ref: float(((got - ref).abs() / ref.abs().clamp_min(1e-300))[ref != 0].max() / U)
    e_log = rl(lg, torch.log(xs.double()))
    e_pow = max(rl(p, torch.pow(ps.double(), e)) for p, e in zip(pw, (INV24, B583)))
    return e_log, e_pow


def check_log_pow(dev, report=print):
    e_log, e_pow = measure_log_pow(dev)
    report(f'[loss64] {dev:4s} logf over [1, 65536]: {e_log:.3f} x 2^-24 relative; powf over [0.0031308, 11.1]: {e_pow:.3f} x 2^-24; used in rule (b): E_LOG {E_LOG:g}, E_POW {E_POW:g}')
    assert 2 * e_log <= E_LOG and 2 * e_pow <= E_POW, (e_log, e_pow)


# ---- the image loss, restated ----------------------------------------------------------------------------------------------------------------
def _srgb(x):
    return torch.where(x > KNEE, torch.pow(torch.clamp(x, min=KNEE), INV24) * S1055 - S0055, S1292 * torch.clamp(x, min=0.0))


def tone(v, tonemap):
    v = torch.clamp(v, 0.0, HDR)
    return _srgb(torch.log(v + 1.0)) if tonemap == 'log_srgb' else v


def loss_elem(a, t, loss):
    d = a - t
    if loss == 'mse':
        return d * d
    if loss == 'smape':
        return d.abs() / (a + t + EPS_SMAPE)
    if loss == 'relmse':
        return d * d / (a * a + t * t + EPS_RELMSE)
    return d.abs()


def img_terms(img, tgt, loss, tonemap):
    """loss.cu:95-131 per pixel: the channel mean of the loss of the tone-mapped colours"""
    return loss_elem(tone(img, tonemap), tone(tgt, tonemap), loss).sum(-1) / 3.0


class ImgLoss(torch.autograd.Function):
    """mean over the pixels of img_terms; backward loss.cu:38-62,137-193 as written (module docstring)"""

    @staticmethod
    def forward(ctx, img, tgt, loss, tonemap):
        ctx.save_for_backward(img, tgt)
        ctx.cfg = (loss, tonemap)
        return img_terms(img, tgt, loss, tonemap).sum() / (img.numel() // 3)

    @staticmethod
    def backward(ctx, g):
        img, tgt = ctx.saved_tensors
        loss, tonemap = ctx.cfg
        go = g * (1.0 / (img.numel() // 3)) / 3.0
        a, t = torch.clamp(img, 0.0, HDR), torch.clamp(tgt, 0.0, HDR)
        la, lt = a, t
        if tonemap == 'log_srgb':
            la, lt = torch.log(a + 1.0), torch.log(t + 1.0)
            a, t = _srgb(la), _srgb(lt)
        d = a - t
        if loss == 'mse':
            ga = go * 2.0 * d
            gt = -ga
        elif loss == 'smape':
            den, s = t + a + EPS_SMAPE, torch.sign(d)
            ga = go * s * (2.0 * t + EPS_SMAPE) / (den * den)
            gt = -go * s * (2.0 * a + EPS_SMAPE) / (den * den)
        elif loss == 'relmse':
            den = t * t + a * a + EPS_RELMSE
            ga = go * 2.0 * d * (t * (t + a) + EPS_RELMSE) / (den * den)
            gt = -go * 2.0 * d * (a * (t + a) + EPS_RELMSE) / (den * den)
        else:
            ga = go * torch.sign(d)
            gt = -ga
        if tonemap == 'log_srgb':
            def back(x0, lx, gx):
                z = torch.zeros_like(gx)
                gs = torch.where(lx > KNEE, gx * B439 / torch.pow(torch.clamp(lx, min=KNEE), B583), torch.where(lx > 0, gx * S1292, z))
                return torch.where((x0 > 0) & (x0 < HDR), gs / (x0 + 1.0), z)
            ga, gt = back(img, la, ga), back(tgt, lt, gt)
        return ga, gt, None, None


def check_restated_backward(report=print):
    """host only: ImgLoss.backward in float64 against float64 autograd of its forward, per element, away from the knee, the clamp bounds and d = 0"""
    gen = _gen('restated')
    n = 4000
    img = torch.exp(torch.rand(n, 3, generator=gen, dtype=torch.float64) * math.log(6e4 / 1e-4) + math.log(1e-4))
    tgt = img * (1.0 + 0.5 * (torch.rand(n, 3, generator=gen, dtype=torch.float64) - 0.5).sign() * (0.01 + torch.rand(n, 3, generator=gen, dtype=torch.float64)))
    tgt = tgt.clamp(1e-5, 6.4e4)
    for x in (img, tgt):
        lx = torch.log(x + 1)
        x[((lx - KNEE).abs() < 1e-3 * KNEE)] *= 1.01
    worst = 0.0
    for loss in LOSSES:
        for tm in TONES:
            a, b = img.clone().requires_grad_(True), tgt.clone().requires_grad_(True)
            ga, gb = torch.autograd.grad(ImgLoss.apply(a, b, loss, tm), [a, b])
            a2, b2 = img.clone().requires_grad_(True), tgt.clone().requires_grad_(True)
            ra, rb = torch.autograd.grad(img_terms(a2, b2, loss, tm).sum() / n, [a2, b2])
            for got, ref in ((ga, ra), (gb, rb)):
                assert bool((ref != 0).all())
                rel = float(((got - ref).abs() / ref.abs()).max())
                worst = max(worst, rel)
                assert rel <= 3e-6, (loss, tm, rel)
    report(f'[loss64] host restated image-loss backward against float64 autograd of the forward: largest relative difference {worst:.3e} (bar 3e-6)')


def tone_delta(A, tonemap, e):
    """absolute rounding error bound of a tone-mapped (or merely clamped) operand of value A whose argument carries e roundings"""
    if tonemap == 'log_srgb':
        return U * (14.0 * (1 + e) + (E_POW + E_LOG + 4.0) * (A + 0.055))
    return U * e * A


def img_forms(img, tgt, loss, tonemap, e_img, e_tgt):
    """float64 first-order bound of the error of forming one pixel's image-loss term (module docstring)"""
    A, Tt = tone(img, tonemap), tone(tgt, tonemap)
    da, dt = tone_delta(A, tonemap, e_img), tone_delta(Tt, tonemap, e_tgt)
    d = (A - Tt).abs()
    l = loss_elem(A, Tt, loss)
    if loss == 'mse':
        f = 2 * d * (da + dt) + 2 * U * l
    elif loss == 'smape':
        den = A + Tt + EPS_SMAPE
        f = ((2 * Tt + EPS_SMAPE) * da + (2 * A + EPS_SMAPE) * dt) / (den * den) + 4 * U * l
    elif loss == 'relmse':
        den = A * A + Tt * Tt + EPS_RELMSE
        f = 2 * d * ((Tt * (Tt + A) + EPS_RELMSE) * da + (A * (Tt + A) + EPS_RELMSE) * dt) / (den * den) + 7 * U * l
    else:
        f = da + dt + U * l
    return f.sum(-1) / 3.0 + 3 * U * l.sum(-1) / 3.0


# ---- SSIM: float64 terms and their forming error ---------------------------------------------------------------------------------------------
def ssim_forms(a, b, e=0):
    """a, b float64 [.., C, H, W] -> (the SSIM map, the first-order bound of the float32 rounding error of forming each of its values);
    e: roundings already in the operands"""
    C = a.shape[-3]
    win = O.ssim_window2d(C, torch.float64, a.device, WIN)
    conv = lambda x: F.conv2d(x, win, padding=5, groups=C)
    mu1, mu2, ea, eb = conv(a), conv(b), conv(a.abs()), conv(b.abs())
    saa, sbb, sab = conv(a * a), conv(b * b), conv(a * b)
    S, Q = saa + sbb, ea * ea + eb * eb
    C1, C2 = SSIM_C1, SSIM_C2
    A1, A2, B1, B2 = 2 * mu1 * mu2 + C1, 2 * (sab - mu1 * mu2) + C2, mu1 * mu1 + mu2 * mu2 + C1, (saa - mu1 * mu1) + (sbb - mu2 * mu2) + C2
    v = (A1 * A2) / (B1 * B2)
    km, ks = 2 * (22 + e) + 2, (23 + 2 * e) + 2 * (22 + e) + 2          # roundings behind mu^2 (and mu1 mu2), and behind a variance
    dA1, dB1 = km * Q + 2 * C1, km * Q + 2 * B1
    dA2, dB2 = ks * S + A2.abs(), ks * S + 2 * B2
    form = U * (A2.abs() / (B1 * B2) * dA1 + A1.abs() / (B1 * B2) * dA2 + v.abs() * dB1 / B1 + v.abs() * dB2 / B2 + 3 * v.abs())
    return v, form


# ---- 1. SSIM alone ---------------------------------------------------------------------------------------------------------------------------
GEOMETRY = [(1, 1), (5, 7), (11, 11), (32, 64), (33, 65), (37, 59), (37, 69), (129, 70)]
CONTENT = [f'm{m}-c{c}' for m in ('0.05', '0.5', '0.95') for c in ('1e-3', '1e-2', '0.3')] + ['const', 'wide']
SSIM_GS = 0.37                                  # the upstream gradient of the mean


def ssim_case(H, W, N, content):
    return dict(H=H, W=W, N=N, content=content, group='ssim-same' if content == 'same' else 'ssim', tag=f'ssim {H}x{W} N{N} {content}',
                power=content in ('m0.05-c1e-3', 'm0.05-c1e-2'))


SSIM_CASES = [ssim_case(H, W, N, c) for (H, W) in GEOMETRY for N in (1, 3) for c in CONTENT + ['same']]


def _smooth(N, H, W, gen):
    """a smooth field in [-1, 1]: three random low-frequency waves per plane"""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    f = torch.zeros(N, H, W, dtype=torch.float64)
    for _ in range(3):
        k = (torch.rand(N, 2, generator=gen, dtype=torch.float64) - 0.5) * 0.5
        ph = torch.rand(N, generator=gen, dtype=torch.float64) * 6.28
        f += torch.sin(k[:, :1, None] * y + k[:, 1:, None] * x + ph[:, None, None]) / 3
    return f


def ssim_inputs(c):
    key = ('in', c['tag'])
    if key in _REF:
        return _REF[key]
    N, H, W, content = c['N'], c['H'], c['W'], c['content']
    gen = _gen('ssim', c['tag'])
    noise = lambda: torch.rand(N, H, W, generator=gen, dtype=torch.float64) * 2 - 1
    if content == 'const':
        a, b = torch.full((N, H, W), 0.6, dtype=torch.float64), torch.full((N, H, W), 0.55, dtype=torch.float64)
    elif content == 'wide':
        a, b = noise() * 0.8 + 0.6, noise() * 0.8 + 0.6                          # [-0.2, 1.4]
    elif content == 'same':
        a = 0.5 + 0.3 * (0.7 * _smooth(N, H, W, gen) + 0.3 * noise())
        b = a.clone()
    else:
        m, ct = float(content.split('-')[0][1:]), float(content.split('-c')[1])
        s = _smooth(N, H, W, gen)
        a, b = m + ct * (0.7 * s + 0.3 * noise()), m + ct * (0.7 * s + 0.3 * noise())
    _REF[key] = (a.float()[None], b.float()[None])
    return _REF[key]


def ssim_reference(c):
    if c['tag'] in _REF:
        return _REF[c['tag']]
    a32, b32 = ssim_inputs(c)
    res = {}
    for name, dt, win in (('r32', torch.float32, WIN), ('r64', torch.float64, WIN), ('exact', torch.float64, exact_window())):
        a, b = a32.to(dt).clone().requires_grad_(True), b32.to(dt).clone().requires_grad_(True)
        v = O.ssim(a, b, win, SSIM_C1, SSIM_C2)
        da, db = torch.autograd.grad(v * SSIM_GS, [a, b])
        res[name] = (v.detach(), da, db)
    res['terms'], res['forms'] = ssim_forms(a32.double(), b32.double())
    _REF[c['tag']] = res
    return res


def run_ssim(dev, c, need_b, report=print):
    from d3h import imgops
    a32, b32 = ssim_inputs(c)
    r = ssim_reference(c)
    N, H, W, group = c['N'], c['H'], c['W'], c['group']
    tag = c['tag'] + (' d_b' if need_b else '')
    if c['content'] == 'same':
        assert torch.equal(a32, b32)
    a, b = a32.clone().to(dev).requires_grad_(True), b32.clone().to(dev).requires_grad_(bool(need_b))
    v = imgops.ssim(a, b)
    got = torch.autograd.grad(v * SSIM_GS, [a, b] if need_b else [a])
    v = v.detach()
    vmap = r['terms'][0]
    power = band_power(vmap) if c['power'] else None
    _scalar(dev, tag, 'ssim', v, r['r64'][0], vmap, r['forms'], chain_ssim(N, H, W), 1.0 / (N * H * W), report, power)
    _compare(dev, group, tag, 'd_a', got[0], r['r32'][1], r['r64'][1], report)
    if need_b:
        _compare(dev, group, tag, 'd_b', got[1], r['r32'][2], r['r64'][2], report)
    ex = r['exact']
    n64 = float(ex[1].norm())
    report(f'[loss64] {dev:4s} {tag:58s} exact-window (no bar): |value - exact| {abs(float(v) - float(ex[0])):.3e}; d_a relative L2 '
           f'{float((got[0].detach().cpu().double() - ex[1]).norm()) / n64 if n64 > 0 else float("nan"):.3e}; reference with the kernel window: '
           f'{abs(float(r["r64"][0]) - float(ex[0])):.3e}, {float((r["r64"][1] - ex[1]).norm()) / n64 if n64 > 0 else float("nan"):.3e}')
    COMPLETE.add((dev, group, tag))


# ---- 2. occupancy cells ----------------------------------------------------------------------------------------------------------------------
OCC_PLACE = {'px31-63': [(31, 32, 63, 64)], 'px32-64': [(32, 33, 64, 65)], 'px0-0': [(0, 1, 0, 1)], 'corner': [(170, 200, -45, None)],
             'centre': [(100, 101, 200, 201)], 'empty': []}


def occ_case(W, place, images=1, source='hand'):
    return dict(H=200, W=W, place=place, images=images, source=source, group='occ', tag=f'occ 200x{W} {place} {source}' + (f' images{images}' if images > 1 else ''))


OCC_CASES = [occ_case(W, p, source=s) for W in (400, 398) for p, s in (('px31-63', 'hand'), ('px32-64', 'pixel_losses'), ('px0-0', 'hand'), ('corner', 'pixel_losses'),
                                                                         ('centre', 'hand'), ('empty', 'pixel_losses'), ('empty', 'hand'))]
OCC_CASES_GPU_ONLY = [occ_case(400, 'centre', images=2, source='pixel_losses'), occ_case(398, 'corner', images=2)]


def occ_inputs(c):
    """-> shaded [B,H,W,4], cref [B,H,W,4] float32: alpha is non-zero in the placed boxes of image 0 only (every further image is empty)"""
    key = ('in', c['tag'])
    if key in _REF:
        return _REF[key]
    B, H, W = c['images'], c['H'], c['W']
    gen = _gen('occ', c['tag'])
    st = torch.rand(B, H, W, 4, generator=gen) * 0.9 + 0.05
    cref = torch.rand(B, H, W, 4, generator=gen) * 0.9 + 0.05
    alpha = torch.zeros(B, H, W)
    for (y0, y1, x0, x1) in OCC_PLACE[c['place']]:
        alpha[0, y0:y1, x0:x1] = torch.rand(alpha[0, y0:y1, x0:x1].shape, generator=gen) * 0.5 + 0.5
    cref[..., 3] = alpha
    _REF[key] = (st, cref)
    return _REF[key]


def hand_occupancy(a, b):
    """[B,3,H,W] x 2 -> int32 [B, ceil(H / 32), ceil(W / 64)]: 1 where a cell holds a non-zero pixel of a or b in any plane"""
    nz = ((a != 0) | (b != 0)).any(1).float()
    H, W = nz.shape[-2:]
    p = F.pad(nz, (0, (-W) % 64, 0, (-H) % 32))
    return (p.reshape(p.shape[0], p.shape[1] // 32, 32, p.shape[2] // 64, 64).amax((2, 4)) > 0).to(torch.int32)


def cheb_to_occupied(occ):
    """per cell the Chebyshev distance (in cells, capped at 9) to the nearest occupied cell of its image"""
    B, OH, OW = occ.shape
    d = torch.full((B, OH, OW), 9, dtype=torch.int64)
    ys, xs = torch.meshgrid(torch.arange(OH), torch.arange(OW), indexing='ij')
    for bi, y, x in occ.nonzero().tolist():
        d[bi] = torch.minimum(d[bi], torch.maximum((ys - y).abs(), (xs - x).abs()))
    return d


def run_occ(dev, c, report=print):
    """d3h_ssim_fwd / d3h_ssim_bwd called directly with the moment-gradient planes and d_a filled with NaN beforehand: whatever the forward
    leaves unwritten stays NaN, so a finite result shows that the backward never reads it"""
    from d3h import _lib as L
    st, cref = occ_inputs(c)
    B, H, W, tag = c['images'], c['H'], c['W'], c['tag']
    N, n = 3 * B, 3 * B * H * W
    OH, OW = _cdiv(H, 32), _cdiv(W, 64)
    a_ref = (st[..., :3] * cref[..., 3:]).permute(0, 3, 1, 2).contiguous()
    b_ref = (cref[..., :3] * cref[..., 3:]).permute(0, 3, 1, 2).contiguous()
    hand = hand_occupancy(a_ref, b_ref)
    if c['source'] == 'pixel_losses':
        sums = torch.empty(10, dtype=torch.float32, device=dev)
        sa, sb = (torch.full((B, 3, H, W), float('nan'), dtype=torch.float32, device=dev) for _ in range(2))
        occ = torch.zeros(B, OH, OW, dtype=torch.int32, device=dev)
        L.call('pixel_losses_fwd', st.to(dev), 4, 0, -1, -1, -1, -1, -1, cref.to(dev), None, 0, B, H, W, 0, 1, sums, sa, sb, None, None, occ)
        assert torch.equal(sa.cpu(), a_ref) and torch.equal(sb.cpu(), b_ref), (tag, 'the SSIM operands of pixel_losses')
        assert torch.equal(occ.cpu(), hand), (tag, 'the occupancy cells of pixel_losses differ from the cells of its own operands')
    else:
        sa, sb, occ = a_ref.to(dev), b_ref.to(dev), hand.to(dev)
    dist = cheb_to_occupied(hand)
    if c['place'] != 'empty':
        assert {1, 2, 3} <= set(dist[0].reshape(-1).tolist()), (tag, 'no cells at distance 1, 2 and 3 of an occupied one')
    gs = torch.full((1,), SSIM_GS / n, dtype=torch.float32, device=dev)
    res = {}
    for route, oc in (('occ', occ), ('none', None)):
        gmom = torch.full((5 * n,), float('nan'), dtype=torch.float32, device=dev)
        out = torch.full((1,), float('nan'), dtype=torch.float32, device=dev)
        L.call('ssim_fwd', sa, sb, N, H, W, None, gmom, 0, out, oc, 3)
        d_a = torch.full((B, 3, H, W), float('nan'), dtype=torch.float32, device=dev)
        L.call('ssim_bwd', sa, sb, N, H, W, gmom, 0, None, gs, 1.0, d_a, None, oc, 3)
        res[route] = (out.cpu(), d_a.cpu(), gmom[:n].cpu())
    out, d_a, g0 = res['occ']
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(d_a).all()), (tag, 'NaN from a plane the forward left unwritten, or an unwritten output')
    assert bool(torch.isfinite(res['none'][2]).all()), (tag, 'without cells every band writes its moment gradients')
    # the test sees what it claims: cells further than 2 from every occupied one are left unwritten, all others are written
    unwritten = torch.isnan(g0.reshape(B, 3, H, W)).any(1)
    far_px = (dist >= 3).repeat_interleave(32, 1).repeat_interleave(64, 2)[:, :H, :W]
    assert torch.equal(unwritten, far_px), (tag, 'moment-gradient planes: written cells differ from "within two cells of an occupied one"')
    assert torch.equal(d_a, res['none'][1]), (tag, 'd_a with occupancy cells differs from the run without')
    empty_img = ~(hand.reshape(B, -1) != 0).any(1)
    assert not bool(d_a[empty_img].any()), (tag, 'd_a of an image without an occupied cell')
    # references
    if tag not in _REF:
        r = {}
        for name, dt in (('r32', torch.float32), ('r64', torch.float64)):
            a = a_ref.to(dt).clone().requires_grad_(True)
            v = O.ssim(a, b_ref.to(dt), WIN, SSIM_C1, SSIM_C2)
            r[name] = (v.detach(), torch.autograd.grad(v * SSIM_GS, a)[0])
        r['terms'], r['forms'] = ssim_forms(a_ref.double(), b_ref.double(), e=1)
        _REF[tag] = r
    r = _REF[tag]
    for route in ('occ', 'none'):
        _scalar(dev, f'{tag} [{route}]', 'ssim', float(res[route][0]) / n, r['r64'][0], r['terms'], r['forms'], chain_ssim(N, H, W), 1.0 / n, report)
    if dev == 'cpu':                       # the float atomics of the workgroups arrive in launch order on the emulation only
        assert torch.equal(out, res['none'][0]), (tag, 'the SSIM sum with occupancy cells differs from the run without')
    _compare(dev, 'occ', tag, 'd_a', d_a, r['r32'][1], r['r64'][1], report)
    COMPLETE.add((dev, 'occ', tag))


# ---- colours, normals ------------------------------------------------------------------------------------------------------------------------
def colours(shape, gen):
    """float32 colours over the classes: < 0, exactly 0, (0, 3e-3) (linear sRGB branch after log(a + 1)), ordinary (twice), 1e3..6.5e4,
    exactly 65535, above"""
    cls = torch.randint(0, 8, shape, generator=gen)
    r = torch.rand(shape, generator=gen, dtype=torch.float64)
    logu = lambda lo, hi: torch.exp(r * math.log(hi / lo) + math.log(lo))
    v = torch.where(cls == 0, -0.2 * r - 1e-3, torch.zeros(shape, dtype=torch.float64))
    v = torch.where(cls == 2, logu(1e-5, 3e-3), v)
    v = torch.where((cls == 3) | (cls == 4), 4e-3 + r * 1.396, v)
    v = torch.where(cls == 5, logu(1e3, 6.5e4), v)
    v = torch.where(cls == 6, torch.full_like(v, HDR), v)
    v = torch.where(cls == 7, logu(7e4, 1e6), v)
    return v.float()


def normals(shape, gen):
    """[.., 3] float32: exactly zero (one in eight), else a random direction of length 2 10^k, k in -15..0"""
    d = torch.randn(*shape, 3, generator=gen, dtype=torch.float64)
    d = d / d.norm(dim=-1, keepdim=True)
    k = torch.randint(-15, 1, shape, generator=gen).double()
    v = d * (2.0 * 10.0 ** k)[..., None]
    v[torch.randint(0, 8, shape, generator=gen) == 0] = 0.0
    return v.float()


def alpha3(shape, gen):
    """{0, 1, interior} in equal parts"""
    c = torch.randint(0, 3, shape, generator=gen)
    return torch.where(c == 0, torch.zeros(shape), torch.where(c == 1, torch.ones(shape), torch.rand(shape, generator=gen) * 0.9 + 0.05))


def _nudge(step):
    """up by a percent or so; from the fourth attempt down by 0.37 (a colour clamped at 65535 whose partner sits just below moves only that way)"""
    return 1.013 + 0.01 * step if step < 3 else 0.37


def settle_pairs(prod, other, fix, spec):
    """input hygiene of one colour pair set.  prod(dt) / other(dt): the two operands of the image loss in dtype dt; fix(mask, step): move the
    offending source colours.  Offenders: log(a + 1) within 1e-5 of the knee, a product within 1e-5 of 65535 without being there, and (l1,
    smape) a pair neither bit-identical nor >= 1e-4 apart after the map"""
    def offenders():
        bad = None
        for dt in (torch.float32, torch.float64):
            a, t = prod(dt), other(dt)
            b = torch.zeros(a.shape, dtype=torch.bool)
            for x in (a, t):
                lx = torch.log(torch.clamp(x, 0.0, HDR).double() + 1)
                b |= (lx - KNEE).abs() <= 1e-5 * KNEE
                b |= ((x.double() - HDR).abs() <= 1e-5 * HDR) & (x.double() != HDR)
            if spec[0] in ('l1', 'smape'):
                A, Tt = (tone(a, spec[1]).double(), tone(t, spec[1]).double())
                b |= (A != Tt) & ((A - Tt).abs() < 1e-4 * torch.maximum(A.abs(), Tt.abs()))
            bad = b if bad is None else bad | b
        if spec[0] in ('l1', 'smape'):                       # identical in one precision means identical in the other
            A32, T32 = tone(prod(torch.float32), spec[1]), tone(other(torch.float32), spec[1])
            A64, T64 = tone(prod(torch.float64), spec[1]), tone(other(torch.float64), spec[1])
            bad |= (A32 == T32) != (A64 == T64)
        return bad
    for step in range(8):
        bad = offenders()
        if not bool(bad.any()):
            return
        fix(bad, step)
    assert not bool(offenders().any()), 'input hygiene: offenders left after 8 nudges'


# ---- 3. pixel_losses -------------------------------------------------------------------------------------------------------------------------
LAYOUTS = {
    'shaded': (4, {'shaded': (0, 4)}),
    'full': (23, {'shaded': (1, 4), 'geometric_normal': (6, 4), 'msdf_image': (10, 1), 'kd_grad': (11, 4), 'ks_grad': (15, 4), 'normal_grad': (19, 4)}),
    'pads': (24, {'shaded': (1, 4), 'geometric_normal': (5, 4), 'msdf_image': (9, 1), 'kd_grad': (10, 4), 'ks_grad': (14, 4), 'normal_grad': (18, 4)}),
}
SHAPES = {1: (1, 1, 1), 255: (1, 15, 17), 256: (2, 8, 16), 257: (1, 1, 257), 524289: (1, 3, 174763)}       # 524289 = 2 256 1024 + 1: a second trip at 2048 workgroups
PREPS = {'none': None, 'plain': (), 'lpips': (SHIFT, SCALE)}


def pixel_case(npix, layout='full', nref=3, loss='l1', tm='log_srgb', ssim=True, prep='none'):
    if layout == 'shaded':
        nref = 0
    return dict(npix=npix, layout=layout, nref=nref, spec=(loss, tm), ssim=ssim, prep=prep, group='pixel', power=npix >= 256,
                tag=f'pixel npix{npix} {layout} nref{nref} {loss}/{tm}' + (' ssim' if ssim else '') + ('' if prep == 'none' else ' prep-' + prep))


PIXEL_CASES = [pixel_case(n, ssim=(n != 524289), layout='shaded' if n == 524289 else 'full') for n in SHAPES] + \
              [pixel_case(257, loss=l, tm=t, layout=('full', 'pads', 'shaded')[i % 3], nref=(3, 4, 0)[(i // 2) % 3], ssim=bool(i % 2), prep=('none', 'plain', 'lpips')[(i + 1) % 3])
               for i, (l, t) in enumerate((l, t) for l in LOSSES for t in TONES)] + \
              [pixel_case(256, 'pads', 4, 'smape', 'log_srgb', True, 'lpips'), pixel_case(255, 'full', 0, 'relmse', 'none', True, 'plain'),
               pixel_case(257, 'shaded', 0, 'mse', 'log_srgb', True, 'plain'), pixel_case(1, 'pads', 4, 'relmse', 'log_srgb', False, 'lpips'),
               pixel_case(524289, 'shaded', 0, 'smape', 'none', False, 'plain')]
PIXEL_CASES = list({c['tag']: c for c in PIXEL_CASES}.values())


def pixel_inputs(c):
    key = ('in', c['tag'])
    if key in _REF:
        return _REF[key]
    B, H, W = SHAPES[c['npix']]
    C, lay = LAYOUTS[c['layout']]
    gen = _gen('pixel', c['tag'])
    st = torch.rand(B, H, W, C, generator=gen) * 1.4 - 0.2
    cs = lay['shaded'][0]
    st[..., cs:cs + 3] = colours((B, H, W, 3), gen)
    cref = torch.cat([colours((B, H, W, 3), gen), alpha3((B, H, W, 1), gen)], -1)
    same = torch.rand(B, H, W, 3, generator=gen) < 0.1                     # bit-identical pairs (d = 0 on all three sides)
    st[..., cs:cs + 3] = torch.where(same, cref[..., :3], st[..., cs:cs + 3])
    if 'msdf_image' in lay:
        cm = lay['msdf_image'][0]
        m = torch.rand(B, H, W, generator=gen) * 2 - 1
        m[torch.randint(0, 4, (B, H, W), generator=gen) == 0] = 0.0        # msdf exactly 0 under every alpha class
        st[..., cm] = m
    if 'geometric_normal' in lay:
        cg = lay['geometric_normal'][0]
        st[..., cg:cg + 3] = normals((B, H, W), gen)
    nref = None
    if c['nref']:
        nref = torch.rand(B, H, W, c['nref'], generator=gen)
        nref[..., :3] = normals((B, H, W), gen)
    al = cref[..., 3:]

    def fix(bad, step):
        sub = st[..., cs:cs + 3]
        sub[bad] = sub[bad] * _nudge(step) + (1e-4 if step < 3 else 0.0)
    settle_pairs(lambda dt: st[..., cs:cs + 3].to(dt) * al.to(dt), lambda dt: cref[..., :3].to(dt) * al.to(dt), fix, c['spec'])
    w = torch.randn(10, generator=gen).sign() * _decades((10,), gen)
    wm = torch.randn(B, H, W, 3, generator=gen) * _decades((B, H, W, 1), gen)
    _REF[key] = (st, cref, nref, w, wm)
    return _REF[key]


def pixel_side(x, cref, nref, lay, spec, want_ssim):
    """parity_cases.check_pixel_losses.torch_side with the layout as a parameter, ImgLoss and the kernel-window SSIM"""
    ch = lambda k: x[..., lay[k][0]:lay[k][0] + lay[k][1]]
    zero = torch.zeros((), dtype=x.dtype)
    sh, al = ch('shaded'), cref[..., 3:]
    v = [F.mse_loss(sh[..., 3:], al), ImgLoss.apply(sh[..., 0:3] * al, cref[..., 0:3] * al, *spec)]
    if 'msdf_image' in lay:
        mi = ch('msdf_image')
        v += [F.l1_loss(mi.clamp(min=0) * (al == 0).to(x.dtype), torch.zeros_like(al)), F.l1_loss(mi.clamp(max=0) * (al == 1).to(x.dtype), torch.ones_like(al))]
    else:                                                    # the kernel's sums of an absent buffer are 0
        v += [zero, zero]
    if nref is not None and 'geometric_normal' in lay:
        out_n = F.normalize(ch('geometric_normal')[..., 0:3], p=2, dim=-1) * torch.tensor([1.0, -1.0, -1.0], dtype=x.dtype)
        gt_n = F.normalize(nref[..., 0:3], p=2, dim=-1)
        v += [F.mse_loss(out_n, gt_n), F.cosine_similarity(out_n.reshape(-1, 3), gt_n.reshape(-1, 3), dim=1).mean()]
    else:
        v += [zero, zero]
    if 'kd_grad' in lay:
        kg, sg, ng = ch('kd_grad'), ch('ks_grad'), ch('normal_grad')
        v += [torch.mean((kg[..., 0] + kg[..., 1] + kg[..., 2]) / 3 * kg[..., -1]), torch.mean(sg[..., :-1] * sg[..., -1:]), torch.mean(ng[..., :-1] * ng[..., -1:])]
    else:
        v += [zero, zero, zero]
    if want_ssim:
        v.append(O.ssim((sh[..., 0:3] * al).permute(0, 3, 1, 2), (cref[..., 0:3] * al).permute(0, 3, 1, 2), WIN, SSIM_C1, SSIM_C2))
    else:
        v.append(zero)
    return torch.stack(v)


def masked_side(x, cref, lay, prep, dt):
    m = x[..., lay['shaded'][0]:lay['shaded'][0] + 3] * cref[..., 3:]
    if prep:
        m = ((2 * m - 1) - torch.tensor([f32c(s) for s in prep[0]], dtype=dt)) / torch.tensor([f32c(s) for s in prep[1]], dtype=dt)
    return m


def pixel_terms(x, cref, nref, lay, spec, want_ssim):
    """float64 -> per sum (terms [npix], forms [npix], mean factor); sums of absent buffers: None"""
    npix = x[..., 0].numel()
    ch = lambda k: x[..., lay[k][0]:lay[k][0] + lay[k][1]].reshape(npix, -1)
    sh, al, rc = ch('shaded'), cref[..., 3].reshape(npix), cref[..., :3].reshape(npix, 3)
    out = []
    da = sh[:, 3] - al
    out.append((da * da, 2 * U * da * da, 1.0 / npix))
    out.append((img_terms(sh[:, :3] * al[:, None], rc * al[:, None], *spec), img_forms(sh[:, :3] * al[:, None], rc * al[:, None], *spec, 1, 1), 1.0 / npix))
    if 'msdf_image' in lay:
        m = ch('msdf_image')[:, 0]
        t2, t3 = (m.clamp(min=0) * (al == 0)).abs(), (m.clamp(max=0) * (al == 1) - 1).abs()
        out += [(t2, 0 * t2, 1.0 / npix), (t3, U * t3, 1.0 / npix)]
    else:
        out += [None, None]
    if nref is not None and 'geometric_normal' in lay:
        sgn = torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64)
        o, t = F.normalize(ch('geometric_normal')[:, :3], dim=-1) * sgn, F.normalize(nref.reshape(npix, -1)[:, :3], dim=-1)
        d = o - t
        t4 = (d * d).sum(-1)
        f4 = (2 * d.abs() * 7 * U * (o.abs() + t.abs())).sum(-1) + 4 * U * t4
        x1, x2 = o / o.norm(dim=-1, keepdim=True).clamp_min(1e-8), t / t.norm(dim=-1, keepdim=True).clamp_min(1e-8)
        out += [(t4, f4, 1.0 / (3 * npix)), ((x1 * x2).sum(-1), 30 * U * (x1 * x2).abs().sum(-1), 1.0 / npix)]
    else:
        out += [None, None]
    if 'kd_grad' in lay:
        for k, div, sc in (('kd_grad', 3.0, 1.0 / npix), ('ks_grad', 1.0, 1.0 / (3 * npix)), ('normal_grad', 1.0, 1.0 / (3 * npix))):
            p = ch(k)
            out.append(((p[:, 0] + p[:, 1] + p[:, 2]) / div * p[:, 3], 4 * U * p[:, :3].abs().sum(-1) / div * p[:, 3].abs(), sc))
    else:
        out += [None, None, None]
    if want_ssim:
        B, H, W = x.shape[:3]
        a = (x[..., lay['shaded'][0]:lay['shaded'][0] + 3] * cref[..., 3:]).permute(0, 3, 1, 2)
        b = (cref[..., :3] * cref[..., 3:]).permute(0, 3, 1, 2)
        vmap, form = ssim_forms(a, b, e=1)
        out.append((vmap.reshape(-1), form.reshape(-1), 1.0 / (3 * npix)))
    else:
        out.append(None)
    return out


def pixel_reference(c):
    if c['tag'] in _REF:
        return _REF[c['tag']]
    st, cref, nref, w, wm = pixel_inputs(c)
    lay, prep = LAYOUTS[c['layout']][1], PREPS[c['prep']]
    res = {}
    for name, dt in (('r32', torch.float32), ('r64', torch.float64)):
        x = st.to(dt).clone().requires_grad_(True)
        cr, nr = cref.to(dt), None if nref is None else nref.to(dt)
        v = pixel_side(x, cr, nr, lay, c['spec'], c['ssim'])
        tot = (v * w.to(dt)).sum()
        m = None
        if prep is not None:
            m = masked_side(x, cr, lay, prep, dt)
            tot = tot + (m * wm.to(dt)).sum()
        res[name] = (v.detach(), torch.autograd.grad(tot, x)[0], None if m is None else m.detach())
    res['terms'] = pixel_terms(st.double(), cref.double(), None if nref is None else nref.double(), lay, c['spec'], c['ssim'])
    _REF[c['tag']] = res
    return res


def run_pixel(dev, c, report=print):
    from d3h import imgops
    st, cref, nref, w, wm = pixel_inputs(c)
    C, lay = LAYOUTS[c['layout']]
    prep, tag, npix = PREPS[c['prep']], c['tag'], c['npix']
    B, H, W = SHAPES[npix]
    r = pixel_reference(c)
    x = st.clone().to(dev).requires_grad_(True)
    d = imgops.pixel_losses(x, lay, cref.to(dev), None if nref is None else nref.to(dev), c['spec'], want_ssim=c['ssim'], masked_prep=prep)
    tot = (d['vec'] * w.to(dev)).sum()
    if prep is not None:
        tot = tot + (d['masked'] * wm.to(dev)).sum()
    d_st, = torch.autograd.grad(tot, x)
    got = d['vec'].detach().cpu()
    for q, (name, tf) in enumerate(zip(imgops.PIXEL_LOSS_KEYS, r['terms'])):
        if tf is None:
            assert float(got[q]) == 0.0 and float(r['r64'][0][q]) == 0.0, (tag, name, 'the sum of an absent buffer')
            continue
        terms, forms, scale = tf
        L = chain_ssim(3 * B, H, W) if name == 'ssim' else chain_pixel(npix)
        power = None
        if c['power'] and name in ('mask_mse', 'img', 'msdf_neg_l1'):
            power = block_power(terms)
        _scalar(dev, tag, name, got[q], r['r64'][0][q], terms, forms, L, scale, report, power)
    _compare(dev, 'pixel', tag, 'd_st', d_st, r['r32'][1], r['r64'][1], report)
    # exact zeros
    g = d_st.cpu()
    used = torch.zeros(C, dtype=torch.bool)
    used[lay['shaded'][0]:lay['shaded'][0] + 4] = True
    for k in ('msdf_image', 'kd_grad', 'ks_grad', 'normal_grad'):
        if k in lay:
            used[lay[k][0]:lay[k][0] + lay[k][1]] = True
    if nref is not None and 'geometric_normal' in lay:
        used[lay['geometric_normal'][0]:lay['geometric_normal'][0] + 3] = True
    assert not bool(g[..., ~used].any()), (tag, 'a gradient in a channel no loss reads')
    assert not bool(r['r64'][1][..., ~used].any())
    cs = lay['shaded'][0]
    a0 = cref[..., 3] == 0
    assert not bool(g[..., cs:cs + 3][a0].any()), (tag, 'a colour gradient where ref.a == 0')
    if prep is not None:
        mk = d['masked'].detach()
        if prep == ():
            assert torch.equal(mk.cpu(), st[..., cs:cs + 3] * cref[..., 3:]), (tag, 'masked is not shaded.rgb ref.a bit for bit')
        _compare(dev, 'pixel', tag, 'masked', mk, r['r32'][2], r['r64'][2], report)
    COMPLETE.add((dev, 'pixel', tag))


# ---- 4. seq_losses ---------------------------------------------------------------------------------------------------------------------------
SEQ_LAYOUT = (12, {'shaded': (1, 4), 'geometric_normal': (6, 4)})
SEQ_SHAPES = {1: (1, 1, 1), 257: (1, 1, 257), 798: (2, 21, 19), 262145: (1, 5, 52429)}            # 262145 = 256 1024 + 1: a second trip at 1024 workgroups


def seq_case(npix, loss, tm):
    return dict(npix=npix, spec=(loss, tm), group='seq', power=npix >= 256, tag=f'seq npix{npix} {loss}/{tm}')


SEQ_CASES = [seq_case(798, l, t) for l in LOSSES for t in TONES] + [seq_case(1, 'l1', 'log_srgb'), seq_case(257, 'mse', 'none'), seq_case(257, 'smape', 'log_srgb'),
                                                                    seq_case(262145, 'l1', 'log_srgb'), seq_case(262145, 'relmse', 'none')]


def seq_inputs(c):
    key = ('in', c['tag'])
    if key in _REF:
        return _REF[key]
    B, H, W = SEQ_SHAPES[c['npix']]
    C, lay = SEQ_LAYOUT
    gen = _gen('seq', c['tag'])
    st = torch.rand(B, H, W, C, generator=gen) * 1.3 - 0.15
    st[..., 1:4] = colours((B, H, W, 3), gen)
    st[..., 9] = alpha3((B, H, W), gen)                                        # coverage {0, interior, 1}
    label = (torch.rand(B, H, W, generator=gen) > 0.5).float()
    gts = []
    for _ in range(3):
        gts.append(torch.cat([colours((B, H, W, 3), gen), (torch.rand(B, H, W, 1, generator=gen) > 0.4).float()], -1))
    same = (torch.rand(B, H, W, generator=gen) < 0.1) & (st[..., 9] == 1)      # bit-identical pairs of the `all` term
    st[..., 1:4] = torch.where(same[..., None], gts[0][..., :3], st[..., 1:4])

    def masks(dt):
        al, lb = st[..., 9].to(dt), label.to(dt)
        return torch.stack([al, lb * al, (1 - lb) * al], 0)[..., None]

    def fix(bad, step):
        b = bad.any(0)
        sub = st[..., 1:4]
        sub[b] = sub[b] * _nudge(step) + (1e-4 if step < 3 else 0.0)
    settle_pairs(lambda dt: st[..., 1:4].to(dt)[None] * masks(dt), lambda dt: torch.stack([g[..., :3] for g in gts], 0).to(dt), fix, c['spec'])
    w = torch.randn(6, generator=gen).sign() * _decades((6,), gen)
    _REF[key] = (st, label, gts, w)
    return _REF[key]


def seq_side(x, label, gts, spec):
    """parity_cases.check_seq_losses.torch_side on ImgLoss"""
    alpha = x[..., 9]
    masks = [alpha[..., None], (label * alpha)[..., None], ((1 - label) * alpha)[..., None]]
    rgb = x[..., 1:4]
    v = [F.mse_loss(m, g[..., 3:]) for m, g in zip(masks, gts)]
    v += [ImgLoss.apply(rgb * m, g[..., 0:3], *spec) for m, g in zip(masks, gts)]
    return torch.stack(v)


def seq_reference(c):
    if c['tag'] in _REF:
        return _REF[c['tag']]
    st, label, gts, w = seq_inputs(c)
    res = {}
    for name, dt in (('r32', torch.float32), ('r64', torch.float64)):
        x = st.to(dt).clone().requires_grad_(True)
        v = seq_side(x, label.to(dt), [g.to(dt) for g in gts], c['spec'])
        res[name] = (v.detach(), torch.autograd.grad((v * w.to(dt)).sum(), x)[0])
    x, lb = st.double(), label.double()
    npix = c['npix']
    al = x[..., 9]
    ms = [al, lb * al, (1 - lb) * al]
    terms = []
    for m, g in zip(ms, gts):
        dm = (m - g[..., 3].double()).reshape(-1)
        terms.append((dm * dm, 2 * dm.abs() * U * m.reshape(-1).abs() + 2 * U * dm * dm, 1.0 / npix))
    for m, g in zip(ms, gts):
        a, t = (x[..., 1:4] * m[..., None]).reshape(npix, 3), g[..., :3].double().reshape(npix, 3)
        terms.append((img_terms(a, t, *c['spec']), img_forms(a, t, *c['spec'], 2, 0), 1.0 / npix))
    res['terms'] = terms
    _REF[c['tag']] = res
    return res


def run_seq(dev, c, report=print):
    from d3h import imgops
    st, label, gts, w = seq_inputs(c)
    r, tag, npix = seq_reference(c), c['tag'], c['npix']
    x = st.clone().to(dev).requires_grad_(True)
    got = imgops.seq_losses(x, SEQ_LAYOUT[1], label.to(dev), *[g.to(dev) for g in gts], c['spec'])
    d_st, = torch.autograd.grad((got * w.to(dev)).sum(), x)
    for q, (name, (terms, forms, scale)) in enumerate(zip(imgops.SEQ_LOSS_KEYS, r['terms'])):
        _scalar(dev, tag, name, got[q], r['r64'][0][q], terms, forms, chain_seq(npix), scale, report, block_power(terms) if c['power'] else None)
    _compare(dev, 'seq', tag, 'd_st', d_st, r['r32'][1], r['r64'][1], report)
    g = d_st.cpu()
    assert not bool(g[..., 0].any()) and not bool(g[..., 4:9].any()) and not bool(g[..., 10:].any()), (tag, 'a gradient in a channel no loss reads')
    COMPLETE.add((dev, 'seq', tag))


# ---- 5. image_loss alone ---------------------------------------------------------------------------------------------------------------------
IMG_SHAPES = {'1': ((1, 1, 1), 1), '257': ((1, 1, 257), 1), 'bcast': ((3, 1, 257), 1)}          # name -> (image shape, batch of the target)


def image_case(shape, loss, tm):
    return dict(shape=shape, spec=(loss, tm), group='image', tag=f'image {shape} {loss}/{tm}')


IMAGE_CASES = [image_case(s, l, t) for s in IMG_SHAPES for l in LOSSES for t in TONES]


def image_inputs(c):
    key = ('in', c['tag'])
    if key in _REF:
        return _REF[key]
    (B, H, W), Bt = IMG_SHAPES[c['shape']]
    gen = _gen('image', c['tag'])
    img, tgt = colours((B, H, W, 3), gen), colours((Bt, H, W, 3), gen)
    same = torch.rand(B, H, W, 3, generator=gen) < 0.1
    img = torch.where(same, tgt.expand(B, H, W, 3), img)

    def fix(bad, step):
        img[bad] = img[bad] * _nudge(step) + (1e-4 if step < 3 else 0.0)
    settle_pairs(lambda dt: img.to(dt), lambda dt: tgt.to(dt).expand(B, H, W, 3), fix, c['spec'])
    w = float(_decades((1,), gen))
    _REF[key] = (img, tgt, w)
    return _REF[key]


def run_image(dev, c, report=print):
    from d3h import imgops
    img, tgt, w = image_inputs(c)
    tag = c['tag']
    npix = img.numel() // 3
    if tag not in _REF:
        res = {}
        for name, dt in (('r32', torch.float32), ('r64', torch.float64)):
            a, t = img.to(dt).clone().requires_grad_(True), tgt.to(dt).clone().requires_grad_(True)
            v = ImgLoss.apply(a, t.expand(a.shape), *c['spec'])
            res[name] = (v.detach(),) + torch.autograd.grad(v * w, [a, t])
        a, t = img.double().reshape(npix, 3), tgt.double().expand(img.shape).reshape(npix, 3)
        res['terms'] = (img_terms(a, t, *c['spec']), img_forms(a, t, *c['spec'], 0, 0))
        _REF[tag] = res
    r = _REF[tag]
    a, t = img.clone().to(dev).requires_grad_(True), tgt.clone().to(dev).requires_grad_(True)
    v = imgops.image_loss(a, t, *c['spec'])
    d_img, d_tgt = torch.autograd.grad(v * w, [a, t])
    assert tuple(d_tgt.shape) == tuple(tgt.shape), (tag, 'the gradient of a broadcast target has the target\'s shape')
    _scalar(dev, tag, 'image_loss', v, r['r64'][0], r['terms'][0], r['terms'][1], chain_image(npix), 1.0 / npix, report,
            block_power(r['terms'][0]) if npix >= 256 else None)
    _compare(dev, 'image', tag, 'd_img', d_img, r['r32'][1], r['r64'][1], report)
    _compare(dev, 'image', tag, 'd_tgt', d_tgt, r['r32'][2], r['r64'][2], report)
    COMPLETE.add((dev, 'image', tag))


# ---- inputs have the edges they claim (no kernel) ---------------------------------------------------------------------------------------------
def check_inputs(report=print):
    gen = _gen('edges')
    v = colours((4000,), gen).double()
    lx = torch.log(v.clamp(0, HDR) + 1)
    for name, m in (('< 0', v < 0), ('== 0', v == 0), ('linear sRGB branch', (v > 0) & (lx < KNEE)), ('ordinary', (lx > KNEE) & (v < 2)), ('1e3..6.5e4', (v >= 1e3) & (v < HDR)),
                    ('== 65535', v == HDR), ('> 65535', v > HDR)):
        assert int(m.sum()) > 100, name
    n = normals((4000,), gen).double().norm(dim=-1)
    assert int((n == 0).sum()) > 100 and bool((n[n > 0] >= 1e-15).all())
    for lo, hi in ((1e-15, 1e-12), (1e-12, 1e-8), (1e-8, 2.1)):
        assert int(((n > lo) & (n < hi)).sum()) > 100, (lo, hi)
    for eps in (1e-12, 1e-8):
        assert not bool(((n - eps).abs() < 0.01 * eps).any())
    st, cref, nref, w, wm = pixel_inputs(pixel_case(257))
    al, m = cref[..., 3], st[..., 10]
    for cls in (al == 0, al == 1, (al > 0) & (al < 1)):
        for ms in (m < 0, m == 0, m > 0):
            assert bool((cls & ms).any()), 'msdf sign x alpha class'
    k = _decades((1000,), gen).log10()
    assert float(k.min()) < -5.9 and float(k.max()) > 1.9
    wk = WIN.astype(np.float64)
    assert abs(wk.sum() - 1 - 4.4e-8) < 2e-8, wk.sum()                             # the kernel's window sums to 1 + 4.4e-8
    report(f'[loss64] inputs: colour classes, normal lengths, msdf x alpha classes present; kernel window sums to 1 + {wk.sum() - 1:.2e}')


# ---- groups and the profile files ------------------------------------------------------------------------------------------------------------
GROUPS = ['ssim', 'ssim-same', 'occ', 'pixel', 'seq', 'image']


def group_runs(dev, group):
    """-> [(tag, callable(report))] of a group on a device"""
    if group in ('ssim', 'ssim-same'):
        return [(c['tag'] + (' d_b' if nb else ''), (lambda rep, c=c, nb=nb: run_ssim(dev, c, nb, rep))) for c in SSIM_CASES if c['group'] == group for nb in (0, 1)]
    if group == 'occ':
        return [(c['tag'], (lambda rep, c=c: run_occ(dev, c, rep))) for c in OCC_CASES + (OCC_CASES_GPU_ONLY if dev != 'cpu' else [])]
    cases, fn = {'pixel': (PIXEL_CASES, run_pixel), 'seq': (SEQ_CASES, run_seq), 'image': (IMAGE_CASES, run_image)}[group]
    return [(c['tag'], (lambda rep, c=c: fn(dev, c, rep))) for c in cases]


def check_group(dev, group, report=print):
    """the banded bar of a group; makes the runs that have not gone through all their comparisons yet"""
    for tag, run in group_runs(dev, group):
        if (dev, group, tag) not in COMPLETE:
            run(lambda s: None)
    check_bands(dev, group, report)


def main(dev):
    """every case with the figures as markdown tables on stdout; a missed bar is printed in bold and the run goes on"""
    import time
    lines, bands = [], []
    t0 = time.time()

    def attempt(what, f, *a):
        try:
            f(*a)
        except AssertionError as e:
            print(f'**bar missed in {what}: {str(e)[:400]}**\n')

    attempt('logf / powf', check_log_pow, dev, lines.append)
    if dev == 'cpu':
        attempt('restated backward', check_restated_backward, lines.append)
        attempt('inputs', check_inputs, lines.append)
    for g in GROUPS:
        for tag, run in group_runs(dev, g):
            attempt(tag, run, lines.append)
    for g in GROUPS:
        attempt(f'bands of group {g}', check_bands, dev, g, bands.append)
    print(f'Device `{dev}`; every run, reference and table: {time.time() - t0:.0f} s of host time.\n')
    print('## Exceptions to the ratio 3 (rule (c))\n')
    for (g, t), v in TENSOR_RATIO.items():
        print(f'- per tensor of a run: group `{g}`, tensor `{t}`: bar {v}')
    for (g, t), (tops, bar, note) in BAND_RATIO.items():
        here = ', '.join(f'band {lab.strip()}: {r:.2f}' for (d_, g_, t_, lab), r in MEASURED.items() if (d_, g_, t_) == (dev, g, t))
        print(f'- per decade band: group `{g}`, tensor `{t}`, bands {" and ".join("0" if d == ZERO_BAND else "1e%d" % d for d in tops)} only: bar {bar}.  Measured in this run: {here}.  When the bar was set: {note}')
    if not TENSOR_RATIO and not BAND_RATIO:
        print('none')
    print('\n## logf / powf, the restated backward, the inputs\n')
    for s in lines:
        if ' e_k ' not in s and ' scalar sum: ' not in s and 'exact-window' not in s:
            print('- ' + ' '.join(s.split()[1:]))
    print('\n## Per decade band of |float64 value|, pooled over the runs of a group (asserted: ratio <= bar)\n')
    print('| group | tensor | band | elements | e_k | e_32 | ratio | bar |\n|---|---|---|---|---|---|---|---|')
    for s in bands:
        w = s.split()
        i = w.index('n')
        print(f'| {w[3]} | {w[4]} | {" ".join(w[7:i])} | {w[i + 1]} | {w[i + 3]} | {w[i + 5]} | {w[i + 7]} | {w[i + 9]} |')
    print('\n## Rule (b): per scalar sum over its runs (asserted in every run: fraction <= 1; L: the derived chain of roundings on partial sums)\n')
    print('| group | sum | runs | largest fraction of the bound | in run | L | smallest workgroup or band / bound (asserted > 1 where given) |\n|---|---|---|---|---|---|---|')
    per = {}
    for s in lines:
        if ' scalar sum: ' in s:
            head, tail = s.split(' scalar sum: ')
            w, t = head.split(), tail.split()
            run = ' '.join(w[2:-1])
            row = per.setdefault((w[2], w[-1]), [0, -1.0, '', [], []])
            row[0] += 1
            if float(t[9]) > row[1]:
                row[1], row[2] = float(t[9]), run
            row[3].append(int(t[11]))
            row[4] += [float(t[15])] if len(t) > 15 else []
    for (g, name), (n, frac, run, Ls, pw) in per.items():
        print(f'| {g} | {name} | {n} | {frac:.4f} | {run} | {min(Ls)} .. {max(Ls)} | {min(pw):.3g} |' if pw else f'| {g} | {name} | {n} | {frac:.4f} | {run} | {min(Ls)} .. {max(Ls)} | |')
    ra, rx = {}, {}
    for s in lines:
        if ' e_k ' in s:
            head, tail = s.split(' e_k ')
            w, t = head.split(), tail.split()
            ra[(' '.join(w[2:-1]), w[-1])] = (float(t[0]), float(t[2]), float(t[4]), ' '.join(t[5:]))
        elif 'exact-window' in s:
            f = s.split('exact-window')[1].replace(';', ' ').replace(',', ' ').split()
            rx[' '.join(s.split('exact-window')[0].split()[2:])] = (f[5], f[9])
    cell = lambda r: '' if r is None else f'{r[0]:.1e} {r[1]:.1e} {r[2]:.2f}'
    print('\n## Rule (a), SSIM alone: per run `e_k e_32 ratio` (asserted: ratio <= 3 for tensors of >= 64 elements; N1 1x1 and 5x7 are pooled only)\n')
    cont = CONTENT + ['same']
    for title, pick in (('d_a', lambda t: ra.get((t, 'd_a'))), ('d_b', lambda t: ra.get((t + ' d_b', 'd_b')))):
        print(f'`{title}`:\n\n| H x W, N | ' + ' | '.join(cont) + ' |\n|---|' + '---|' * len(cont))
        for (H, W) in GEOMETRY:
            for N in (1, 3):
                print(f'| {H}x{W} N{N} | ' + ' | '.join(cell(pick(f'ssim {H}x{W} N{N} {c}')) for c in cont) + ' |')
        print()
    print('Distance of the kernel to the float64 run with the exactly normalised window, `|value - exact|  relative L2 of d_a` (no bar):\n')
    print('| H x W, N | ' + ' | '.join(cont) + ' |\n|---|' + '---|' * len(cont))
    for (H, W) in GEOMETRY:
        for N in (1, 3):
            print(f'| {H}x{W} N{N} | ' + ' | '.join(' '.join(rx.get(f'ssim {H}x{W} N{N} {c}', ('', ''))) for c in cont) + ' |')
    print('\n## Rule (a), the other kernels: per run and tensor (asserted: ratio <= 3 for tensors of >= 64 elements)\n')
    print('| run | tensor | e_k | e_32 | ratio | |\n|---|---|---|---|---|---|')
    for (run, tensor), r in ra.items():
        if not run.startswith('ssim '):
            print(f'| {run} | {tensor} | {r[0]:.3e} | {r[1]:.3e} | {r[2]:.2f} | {r[3]} |')


if __name__ == '__main__':
    import sys
    import conftest
    from d3h import _lib as L
    device = sys.argv[1] if len(sys.argv) > 1 else 'cpu'
    if device == 'cpu':
        L._use_emulator_for_tests(conftest.EMUL_SO)
    main(device)
