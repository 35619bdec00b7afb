"""Host side of csrc/image_ops.hip: mesh normals, shading normal, image loss, SSIM, SDF edge regulariser (autograd)."""
import ctypes
import os

import torch
from .devconst import const as _const

from . import _lib as L


# ---- mesh normals --------------------------------------------------------------------------------------
class _AutoNormalsFn(torch.autograd.Function):
    """v: [P,3] or [B,P,3] (B vertex sets sharing the face list)"""

    @staticmethod
    def forward(ctx, v, f32):
        v = v.contiguous().float()
        nb = 1 if v.dim() == 2 else v.shape[0]
        nv, nf = v.shape[-2], f32.shape[0]
        raw = torch.empty_like(v)
        vn = torch.empty_like(v)
        L.call('auto_normals_fwd', v, nb, nv, f32, nf, raw, vn)
        ctx.save_for_backward(v, f32, raw)
        return vn

    @staticmethod
    def backward(ctx, g):
        v, f32, raw = ctx.saved_tensors
        nb = 1 if v.dim() == 2 else v.shape[0]
        d_v = L.zeros_like(v)
        g_raw = torch.empty_like(v)
        L.call('auto_normals_bwd', v, nb, v.shape[-2], f32, f32.shape[0], raw, g.contiguous(), g_raw, d_v)
        return d_v, None


def auto_normals(v_pos, faces32):
    """render/mesh.py:418-446: area-weighted, normalised vertex normals; zero-length -> (0,0,1).  v_pos [P,3] or [B,P,3]."""
    return _AutoNormalsFn.apply(v_pos, faces32.contiguous())


class _FaceNormalsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, f32):
        v = v.contiguous().float()
        nb = 1 if v.dim() == 2 else v.shape[0]
        nf = f32.shape[0]
        fn = torch.empty(*v.shape[:-2], nf, 3, dtype=torch.float32, device=v.device)
        L.call('face_normals_fwd', v, nb, v.shape[-2], f32, nf, fn)
        ctx.save_for_backward(v, f32)
        ctx.zeros = L.zeros_like(v) if ctx.needs_input_grad[0] else None      # d_v, filled ahead of the backward (d3h/mtets.py)
        return fn

    @staticmethod
    def backward(ctx, g):
        v, f32 = ctx.saved_tensors
        nb = 1 if v.dim() == 2 else v.shape[0]
        d_v, ctx.zeros = getattr(ctx, 'zeros', None), None
        if d_v is None:
            d_v = L.zeros_like(v)
        L.call('face_normals_bwd', v, nb, v.shape[-2], f32, f32.shape[0], g.contiguous(), d_v)
        return d_v, None


def face_normals(v_pos, faces32):
    """render/render.py:261-264: safe_normalize(cross(v1 - v0, v2 - v0)) per face.  v_pos [P,3] or [B,P,3]."""
    return _FaceNormalsFn.apply(v_pos, faces32.contiguous())


# ---- prepare_shading_normal ---------------------------------------------------------------------------
def _bc_strides(ts, shape, what='prepare_shading_normal'):
    """ts: tensors [B,H,W,C] or broadcast along any of B / H / W (fewer than four dims: leading ones are added) -> (float32 contiguous copies,
    int64[len(ts)][3] of their (b, h, w) element strides with 0 for a broadcast dim): the `Bc` convention of csrc/d3h_bcast.h"""
    B, H, W = shape
    out = []
    keep = []
    for t in ts:
        t = t.float()
        while t.dim() < 4:
            t = t[None]
        t = t.contiguous()
        keep.append(t)
        st = [t.stride(k) if t.shape[k] != 1 else 0 for k in range(3)]
        for k, full in enumerate((B, H, W)):
            if t.shape[k] not in (1, full):
                raise RuntimeError(f'{what}: shapes are not broadcastable')
        out += st
    arr = (ctypes.c_int64 * len(out))(*out)
    return keep, arr


class _ShadingNormalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, view_pos, pert, snrm, stng, gnrm, two_sided, opengl):
        ins = [pos, view_pos, pert, snrm, stng, gnrm]
        shp = [max(t.shape[k] if t.dim() == 4 else 1 for t in ins) for k in range(3)]
        keep, strides = _bc_strides(ins, shp)
        B, H, W = shp
        out = torch.empty(B, H, W, 3, dtype=torch.float32, device=pos.device)
        L.call('shading_normal_fwd', *keep, strides, B, H, W, int(two_sided), int(opengl), out)
        ctx.save_for_backward(*keep)
        ctx.meta = (shp, bool(two_sided), bool(opengl), [tuple(t.shape) for t in ins])
        return out

    @staticmethod
    def backward(ctx, g):
        keep = list(ctx.saved_tensors)
        shp, two_sided, opengl, in_shapes = ctx.meta
        B, H, W = shp
        _, strides = _bc_strides(keep, shp)
        grads = [torch.empty(B, H, W, 3, dtype=torch.float32, device=g.device) for _ in range(6)]
        L.call('shading_normal_bwd', *keep, strides, B, H, W, int(two_sided), int(opengl), g.contiguous(), *grads)
        outs = []
        for gr, shape in zip(grads, in_shapes):
            full = (1,) * (4 - len(shape)) + tuple(shape)
            red = [k for k in range(3) if full[k] == 1 and shp[k] != 1]
            if red:
                gr = gr.sum(dim=red, keepdim=True)
            outs.append(gr.reshape(shape))
        return (*outs, None, None)


def prepare_shading_normal(pos, view_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm, two_sided_shading=True, opengl=True):
    if perturbed_nrm is None:   # renderutils/ops.py:220-221
        perturbed_nrm = _const((0.0, 0.0, 1.0), pos.device)[None, None, None, :]
    return _ShadingNormalFn.apply(pos, view_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm, two_sided_shading, opengl)


# ---- image loss -------------------------------------------------------------------------------------------
_LOSS = {'l1': 0, 'mse': 1, 'smape': 2, 'relmse': 3}
_TONE = {'none': 0, 'log_srgb': 1}


class _ImageLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, target, loss, tonemapper):
        img_c = img.float().expand(torch.broadcast_shapes(img.shape, target.shape)).contiguous()
        tgt_c = target.float().expand(img_c.shape).contiguous()
        npix = img_c.numel() // 3
        out = torch.empty(1, dtype=torch.float32, device=img.device)
        L.call('image_loss_fwd', img_c, tgt_c, npix, _LOSS[loss], _TONE[tonemapper], out)
        ctx.save_for_backward(img_c, tgt_c)
        ctx.meta = (loss, tonemapper, npix, img.shape, target.shape)
        return out[0] / npix

    @staticmethod
    def backward(ctx, g):
        img_c, tgt_c = ctx.saved_tensors
        loss, tonemapper, npix, ishape, tshape = ctx.meta
        d_img = torch.empty_like(img_c) if ctx.needs_input_grad[0] else None
        d_tgt = torch.empty_like(tgt_c) if ctx.needs_input_grad[1] else None
        gs = g.reshape(1).contiguous().float()
        L.call('image_loss_bwd', img_c, tgt_c, npix, _LOSS[loss], _TONE[tonemapper], gs, 1.0 / npix, d_img, d_tgt)
        red = lambda t, s: None if t is None else t.sum_to_size(s)
        return red(d_img, ishape), red(d_tgt, tshape), None, None


def image_loss(img, target, loss='l1', tonemapper='none'):
    """renderutils/ops.py:479-501 (the live CUDA path, loss.cu:95): scalar mean over pixels of the channel-mean loss"""
    return _ImageLossFn.apply(img, target, loss, tonemapper)


# ---- SSIM ----------------------------------------------------------------------------------------------------
class _SSIMFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a_c, b_c = a.contiguous().float(), b.contiguous().float()
        H, W = a_c.shape[-2:]
        N = a_c.numel() // (H * W)
        need = a.requires_grad or b.requires_grad
        tmp = None
        gmom = torch.empty(5 * N * H * W, dtype=torch.float32, device=a.device) if need else None
        out = torch.empty(1, dtype=torch.float32, device=a.device)
        need_b = bool(b.requires_grad)          # a constant second image (the target of a loss): three moment-gradient planes instead of five
        L.call('ssim_fwd', a_c, b_c, N, H, W, tmp, gmom, need_b, out, None, 1)
        if need:
            ctx.save_for_backward(a_c, b_c, gmom)
        ctx.dims = (N, H, W)
        ctx.need_b = need_b
        return out[0] / (N * H * W)

    @staticmethod
    def backward(ctx, g):
        a_c, b_c, gmom = ctx.saved_tensors
        N, H, W = ctx.dims
        tmp = None
        d_a = torch.empty_like(a_c) if ctx.needs_input_grad[0] else None
        d_b = torch.empty_like(b_c) if (ctx.needs_input_grad[1] and ctx.need_b) else None
        gs = g.reshape(1).contiguous().float()
        L.call('ssim_bwd', a_c, b_c, N, H, W, gmom, ctx.need_b, tmp, gs, 1.0 / (N * H * W), d_a, d_b, None, 1)
        return d_a, d_b


def ssim(img1, img2, window_size=11, size_average=True):
    """ssim_loss.py:33-63 for [B,C,H,W] (or [C,H,W]) images: mean SSIM with an 11x11 Gaussian window (sigma 1.5)"""
    if window_size != 11 or not size_average:
        raise NotImplementedError('d3h.ssim: window_size=11, size_average=True only')
    return _SSIMFn.apply(img1, img2)


# ---- the first k channels of a pixel-major tensor, with a one-pass backward ----------------------------------------------------------------
class _FirstChannelsFn(torch.autograd.Function):
    """x[..., :k] as a VIEW (no copy), whose gradient (g, zeros) is written by one kernel (csrc/image_ops.hip: channels_pad_kernel) -- autograd's own
    slice node fills a zero tensor of x's size and copies g into it: two passes, 59 us at 4 x 1024^2 x 6"""

    @staticmethod
    def forward(ctx, x, k):
        ctx.cout = int(x.shape[-1])
        return x[..., :k]

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous().float()
        cin, cout = int(g.shape[-1]), ctx.cout
        out = torch.empty(*g.shape[:-1], cout, dtype=torch.float32, device=g.device)
        L.call('channels_pad', g, g.numel() // cin, cin, cout, out)
        return out, None


def first_channels(x, k):
    """x[..., :k] (a view); use where x is large and only these channels take a gradient"""
    if not (torch.is_grad_enabled() and x.requires_grad) or x.dtype != torch.float32 or k >= x.shape[-1]:
        return x[..., :k]
    return _FirstChannelsFn.apply(x, int(k))


# ---- composite of the layer buffers against their backgrounds -----------------------------------------------------------------
COMP_ZERO, COMP_IMAGE, COMP_CONST20, COMP_ALPHA = 0, 1, 2, 3


def _pix_view(t):
    """(tensor kept alive, pointer, floats between pixels) of a [..., c] slice of a pixel-major tensor, without copying"""
    t = t.float()
    c = t.shape[-1]
    st = t.stride()
    ok = st[-1] == 1 or c == 1
    ps = st[-2]
    n = 1
    for d in range(t.dim() - 2, -1, -1):       # every leading dim must continue the same pixel pitch
        ok = ok and (t.shape[d] == 1 or st[d] == ps * n)
        n *= t.shape[d]
    if not ok:
        t = t.contiguous()
        ps = c
    return t, ps


class _CompositeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rast, kinds, bgs, *srcs):
        import ctypes
        B, H, W = rast.shape[:3]
        dev = rast.device
        n = len(srcs)
        views = [_pix_view(s) for s in srcs]
        nch = [int(s.shape[-1]) for s in srcs]
        C = sum(1 if k == COMP_ALPHA else c + 1 for k, c in zip(kinds, nch))
        out = torch.empty(B, H, W, C, dtype=torch.float32, device=dev)
        bg_t = [None if b is None else b.float().contiguous() for b in bgs]
        I = ctypes.c_int * n
        rc = rast.contiguous()
        L.call('composite_fwd', n, L.ptr_array([v[0] for v in views], strided=True), I(*[int(v[1]) for v in views]), I(*nch), I(*kinds), L.ptr_array(bg_t),
               I(*[0 if b is None or b.shape[0] == 1 else 1 for b in bg_t]), rc, B, H, W, out)
        ctx.save_for_backward(rc)
        ctx.meta = (kinds, nch, [s.shape for s in srcs])
        return out

    @staticmethod
    def backward(ctx, g):
        import ctypes
        rc, = ctx.saved_tensors
        kinds, nch, shapes = ctx.meta
        B, H, W = rc.shape[:3]
        n = len(nch)
        g = g.contiguous().float()
        ds = [torch.empty(B, H, W, c, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[3 + k] else None for k, c in enumerate(nch)]
        I = ctypes.c_int * n
        L.call('composite_bwd', n, L.ptr_array(ds), I(*nch), I(*kinds), rc, B, H, W, g)
        red = lambda d, shp: None if d is None else d.sum_to_size(shp)
        return (None, None, None) + tuple(red(d, shp) for d, shp in zip(ds, shapes))


def composite(rast, sources):
    """render/render.py:375-382,430-449 for all buffers at once.  sources: list of (values [B,H,W,c] (a strided slice is fine), kind,
    background) with kind COMP_ZERO / COMP_IMAGE (background [1|B,H,W,3], alpha 0) / COMP_CONST20 / COMP_ALPHA (c = 1: the value is
    the alpha, output one channel).  Returns [B,H,W,sum(c+1)] = lerp(background, [values, 1], coverage) per buffer, concatenated."""
    B, H, W = rast.shape[:3]
    srcs = [s.expand(B, H, W, s.shape[-1]) for s, _, _ in sources]
    return _CompositeFn.apply(rast, [k for _, k, _ in sources], [b for _, _, b in sources], *srcs)


def composite_antialias(rast, sources, pos, tri):
    """antialias(composite(rast, sources), rast, pos, tri) in ONE forward pass (csrc/raster.hip:aa_composite_fwd_kernel), for renders
    nobody differentiates: the dead buffers of a tick in its 'all' mode, the watertight validation render.  Bit-identical to the two
    separate ops; no autograd (call it under torch.no_grad())."""
    assert not torch.is_grad_enabled() or not any(s.requires_grad for s, _, _ in sources), 'composite_antialias is forward-only'
    B, H, W = rast.shape[:3]
    srcs = [s.expand(B, H, W, s.shape[-1]) for s, _, _ in sources]
    return _composite_antialias_fwd(rast, pos, tri, [k for _, k, _ in sources], [b for _, _, b in sources], [_pix_view(s) for s in srcs])[0]


def _composite_antialias_fwd(rast, pos, tri, kinds, bgs, views):
    """the one call of composite_antialias_fwd; views: _pix_view of every source -> (out, what the backward needs of the prepared arguments:
    rast, pos, tri, flags, backgrounds, channels per source)"""
    import ctypes
    from . import raster as _R
    B, H, W = rast.shape[:3]
    n = len(views)
    nch = [int(v[0].shape[-1]) for v in views]
    C = sum(1 if k == COMP_ALPHA else c + 1 for k, c in zip(kinds, nch))
    out = torch.empty(B, H, W, C, dtype=torch.float32, device=rast.device)
    bg_t = [None if b is None else b.float().contiguous() for b in bgs]
    rc, pos_c, tri_c = rast.contiguous(), pos.contiguous().float(), tri.contiguous()
    flags = _R._edge_flags(pos_c, tri_c, B, H, W)
    I = ctypes.c_int * n
    L.call('composite_antialias_fwd', n, L.ptr_array([v[0] for v in views], strided=True), I(*[int(v[1]) for v in views]), I(*nch), I(*kinds),
           L.ptr_array(bg_t), I(*[0 if b is None or b.shape[0] == 1 else 1 for b in bg_t]), rc, pos_c, _R._bstride(pos_c), tri_c,
           tri_c.shape[0], flags, B, H, W, out)
    return out, (rc, pos_c, tri_c, flags, bg_t, nch)


class _CompositeAntialiasFn(torch.autograd.Function):
    """antialias(composite(rast, sources), rast, pos, tri) with its gradient, one kernel each way (csrc/raster.hip:aa_composite_fwd_kernel /
    aa_composite_bwd_kernel): the composited, pre-antialias image is never stored -- the backward re-evaluates it at the pair pixels.
    `use[k]`: source k is the first use[k] channels of the tensor passed in (0 = all of it); its gradient comes back at the tensor's full
    width, the unused channels zero-filled by the same kernel (the slice node + its pad pass of the separate path)."""

    @staticmethod
    def forward(ctx, rast, pos, tri, kinds, bgs, use, *srcs):
        views = [_pix_view(s if not u else s[..., :u]) for s, u in zip(srcs, use)]
        out, (rc, pos_c, tri_c, flags, bg_t, nch) = _composite_antialias_fwd(rast, pos, tri, kinds, bgs, views)
        ctx.save_for_backward(rc, pos_c, tri_c, flags, *[v[0] for v in views], *[b for b in bg_t if b is not None])
        ctx.meta = (kinds, nch, [s.shape for s in srcs], [int(v[1]) for v in views], [b is not None for b in bg_t])
        return out

    @staticmethod
    def backward(ctx, g):
        import ctypes
        from . import raster as _R
        kinds, nch, shapes, strides, has_bg = ctx.meta
        n = len(nch)
        saved = ctx.saved_tensors
        rc, pos_c, tri_c, flags = saved[:4]
        views = saved[4:4 + n]
        bgs_it = iter(saved[4 + n:])
        bg_t = [next(bgs_it) if h else None for h in has_bg]
        B, H, W = rc.shape[:3]
        g = g.contiguous().float()
        dch = [int(shp[-1]) for shp in shapes]                      # the gradient comes back at the width of the tensor passed in
        ds = [torch.empty(B, H, W, c, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[6 + k] else None for k, c in enumerate(dch)]
        d_pos = L.zeros_like(pos_c) if ctx.needs_input_grad[1] else None
        I = ctypes.c_int * n
        L.call('composite_antialias_bwd', n, L.ptr_array(views, strided=True), L.ptr_array(ds), I(*dch), I(*strides), I(*nch), I(*kinds),
               L.ptr_array(bg_t), I(*[0 if b is None or b.shape[0] == 1 else 1 for b in bg_t]), rc, pos_c, _R._bstride(pos_c), tri_c,
               tri_c.shape[0], flags, B, H, W, g, d_pos)
        red = lambda d, shp: None if d is None else d.sum_to_size(shp)
        return (None, d_pos, None, None, None, None) + tuple(red(d, shp) for d, shp in zip(ds, shapes))


def composite_antialias_grad(rast, sources, pos, tri):
    """antialias(composite(rast, sources), rast, pos, tri), differentiable in the sources and in `pos`, as one kernel forward and one
    backward.  Values bit-identical to the two separate ops, source gradients too; d(pos) up to the order of its float atomics.
    A source may be given as (tensor, kind, background, k): the buffer is tensor[..., :k] (see _CompositeAntialiasFn)."""
    B, H, W = rast.shape[:3]
    srcs = [s[0].expand(B, H, W, s[0].shape[-1]) for s in sources]
    use = [int(s[3]) if len(s) > 3 and s[3] and s[3] < s[0].shape[-1] else 0 for s in sources]
    return _CompositeAntialiasFn.apply(rast, pos, tri, [s[1] for s in sources], [s[2] for s in sources], use, *srcs)


# ---- one step of layered compositing (depth peeling) ------------------------------------------------------------------------------------------
LAYER_MAX_CHANNELS = 64          # csrc/raster.hip: the rows of a 256-pixel tile in 64 KB of LDS (forward C, backward C + the widest source gradient)


class _LayerCompositeAntialiasFn(torch.autograd.Function):
    """csrc/raster.hip: layer_composite_fwd_kernel / layer_composite_bwd_kernel, one launch each way; the blended, pre-antialias image is never
    stored.  Only the gradients somebody asks for are allocated and written."""

    @staticmethod
    def forward(ctx, rast, pos, tri, kinds, flags, alpha, under, *srcs):
        from . import raster as _R
        B, H, W = rast.shape[:3]
        n = len(srcs)
        views = [_pix_view(s) for s in srcs]
        nch = [int(v[0].shape[-1]) for v in views]
        C = sum(1 if k == COMP_ALPHA else c + 1 for k, c in zip(kinds, nch))
        rc, pos_c, tri_c = rast.contiguous(), pos.contiguous().float(), tri.contiguous()
        under_c = under.contiguous().float()
        if tuple(under_c.shape) != (B, H, W, C):
            raise ValueError(f'layer_composite_antialias: under must be [{B}, {H}, {W}, {C}], not {tuple(under.shape)}')
        widest = max([c for k, c in enumerate(nch) if ctx.needs_input_grad[7 + k]], default=0)
        if C > LAYER_MAX_CHANNELS or (widest and C + widest > LAYER_MAX_CHANNELS):
            raise ValueError(f'layer_composite_antialias: {C} channels' + (f' + a source gradient of {widest}' if widest else '') +
                             f' exceed the {LAYER_MAX_CHANNELS} a tile has room for; composite fewer buffers per call')
        alpha_c = None if alpha is None else alpha.float().expand(B, H, W, 1).contiguous()
        if flags is None:
            flags = _R._edge_flags(pos_c, tri_c, B, H, W)
        out = torch.empty(B, H, W, C, dtype=torch.float32, device=rast.device)
        I = ctypes.c_int * n
        L.call('layer_composite_antialias_fwd', n, L.ptr_array([v[0] for v in views], strided=True), I(*[int(v[1]) for v in views]), I(*nch), I(*kinds),
               alpha_c, under_c, rc, pos_c, _R._bstride(pos_c), tri_c, tri_c.shape[0], flags, B, H, W, out)
        ctx.save_for_backward(rc, pos_c, tri_c, flags, alpha_c, under_c, *[v[0] for v in views])
        ctx.meta = (kinds, nch, [s.shape for s in srcs], [int(v[1]) for v in views], None if alpha is None else alpha.shape, under.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import raster as _R
        kinds, nch, shapes, strides, ashape, ushape = ctx.meta
        n = len(nch)
        rc, pos_c, tri_c, flags, alpha_c, under_c = ctx.saved_tensors[:6]
        views = ctx.saved_tensors[6:]
        B, H, W = rc.shape[:3]
        g = g.contiguous().float()
        new = lambda c: torch.empty(B, H, W, c, dtype=torch.float32, device=g.device)
        ds = [new(c) if ctx.needs_input_grad[7 + k] else None for k, c in enumerate(nch)]
        d_alpha = new(1) if (alpha_c is not None and ctx.needs_input_grad[5]) else None
        d_under = torch.empty_like(under_c) if ctx.needs_input_grad[6] else None
        d_pos = L.zeros_like(pos_c) if ctx.needs_input_grad[1] else None
        I = ctypes.c_int * n
        L.call('layer_composite_antialias_bwd', n, L.ptr_array(views, strided=True), L.ptr_array(ds), I(*nch), I(*strides), I(*nch), I(*kinds),
               alpha_c, under_c, rc, pos_c, _R._bstride(pos_c), tri_c, tri_c.shape[0], flags, B, H, W, g, d_alpha, d_under, d_pos)
        red = lambda d, shp: None if d is None else d.sum_to_size(shp)
        return (None, d_pos, None, None, None, red(d_alpha, ashape), red(d_under, ushape)) + tuple(red(d, shp) for d, shp in zip(ds, shapes))


def layer_composite_antialias(rast, sources, alpha, under, pos, tri, flags=None):
    """One step of layered compositing, back to front (render/render.py's docstring states the whole contract): layer `rast` laid over `under`
    and antialiased along its own silhouettes,
        out = antialias(lerp(under, [values_k, 1], w) for every source k, rast, pos, tri),   w = (rast[..., 3] > 0) * alpha.
    sources: list of (values [B,H,W,c] (a strided slice is fine), kind[, ...]) as for composite(); kinds COMP_ZERO / COMP_IMAGE / COMP_CONST20 are
    one case here (c + 1 channels, the last the layer's opacity; their backgrounds are what the caller put into the deepest `under`), COMP_ALPHA
    (c = 1) is lerp(under, 1, coverage * values) in one channel, which `alpha` does not enter.  alpha: [B,H,W,1] or None (= 1); under:
    [B,H,W,sum of the widths], not modified.  The lerp is torch.lerp's two-branch form: exact at w = 0 (under) and w = 1 (the source), so a
    layer that covers nothing returns `under` bit for bit.  Differentiable in every source, alpha, under and pos (d_pos by float atomics, everything
    else gathered); under torch.no_grad() only the forward kernel runs.  flags: d3h.raster._edge_flags(pos, tri, ...), which depend on (pos, tri)
    only -- a caller that composites several layers passes the same ones to every step.  At most LAYER_MAX_CHANNELS channels."""
    B, H, W = rast.shape[:3]
    srcs = [s[0].expand(B, H, W, s[0].shape[-1]) for s in sources]
    return _LayerCompositeAntialiasFn.apply(rast, pos, tri, [int(s[1]) for s in sources], flags, alpha, under, *srcs)


# ---- fused per-pixel loss stack of tick_init / tick_split -------------------------------------------------------------------
SSIM_OCC = os.environ.get('D3H_SSIM_OCC', '1') != '0'
PIXEL_LOSS_KEYS = ('mask_mse', 'img', 'msdf_pos_l1', 'msdf_neg_l1', 'normal_mse', 'normal_cos', 'kd_grad', 'ks_grad', 'normal_grad', 'ssim')


class _PixelLossesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, stacked, cref, nref, cs, cg, cm, ckg, csg, cng, loss, tonemap, want_ssim, masked_prep):
        st = stacked.contiguous().float()
        B, H, W, C = st.shape
        cr = cref.float().expand(B, H, W, 4).contiguous()
        nr = None
        if nref is not None:
            nr = nref.float().expand(B, H, W, nref.shape[-1])
            nr = nr if nr.is_contiguous() else nr.contiguous()
        dev = st.device
        sums = torch.empty(10, dtype=torch.float32, device=dev)
        npix = B * H * W
        sa = sb = None
        if want_ssim:
            sa = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
            sb = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        # masked_prep: None = no extra output; () = the masked colour image shaded.rgb * ref.a; (shift[3], scale[3]) = that image mapped
        # to the LPIPS trunk input ((2 x - 1) - shift) / scale -- a second, differentiable output [B,H,W,3]
        masked = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev) if masked_prep is not None else None
        # the occupancy cells of the two SSIM operands (csrc/image_ops.hip: SsimOcc): both are zero wherever the target's alpha is, and the
        # SSIM passes skip the bands that see nothing else -- same results; D3H_SSIM_OCC=0: every band is computed
        occ = L.zeros((B, -(-H // 32), -(-W // 64)), torch.int32, dev) if (want_ssim and SSIM_OCC) else None
        prep = (ctypes.c_float * 6)(*[float(v) for v in (list(masked_prep[0]) + list(masked_prep[1]))]) if masked_prep else None
        L.call('pixel_losses_fwd', st, C, cs, cg, cm, ckg, csg, cng, cr, nr, 0 if nr is None else nr.shape[-1], B, H, W, loss, tonemap, sums, sa, sb,
               masked, prep, occ)
        gmom = None
        need = stacked.requires_grad
        if want_ssim:
            N = 3 * B
            tmp = None
            gmom = torch.empty(5 * N * H * W, dtype=torch.float32, device=dev) if need else None
            L.call('ssim_fwd', sa, sb, N, H, W, tmp, gmom, 0, sums[9:], occ, 3)          # (0: the masked target is a constant)
        else:
            sums[9:].zero_()
        scale = _const([1.0 / npix] * 4 + [1.0 / (3 * npix), 1.0 / npix, 1.0 / npix, 1.0 / (3 * npix), 1.0 / (3 * npix), 1.0 / (3 * npix)], dev) \
            if npix else torch.zeros(10, device=dev)
        ctx.cfg = (B, H, W, C, cs, cg, cm, ckg, csg, cng, loss, tonemap, want_ssim, prep)
        ctx.save_for_backward(st, cr, nr, sa, sb, gmom, scale, occ)
        if masked is None:
            return sums * scale
        return sums * scale, masked

    @staticmethod
    def backward(ctx, g, g_masked=None):
        st, cr, nr, sa, sb, gmom, scale, occ = ctx.saved_tensors
        B, H, W, C, cs, cg, cm, ckg, csg, cng, loss, tonemap, want_ssim, prep = ctx.cfg
        gs = (g.float() * scale).contiguous() if g is not None else torch.zeros(10, dtype=torch.float32, device=st.device)
        gm = g_masked.contiguous().float() if g_masked is not None else None
        d_a = None
        if want_ssim:
            N = 3 * B
            tmp = None
            d_a = torch.empty_like(sa)
            L.call('ssim_bwd', sa, sb, N, H, W, gmom, 0, tmp, gs[9:], 1.0, d_a, None, occ, 3)
        d_st = torch.empty_like(st)
        L.call('pixel_losses_bwd', st, C, cs, cg, cm, ckg, csg, cng, cr, nr, 0 if nr is None else nr.shape[-1], B, H, W, loss, tonemap, gs, d_a, gm,
               prep if gm is not None else None, d_st)
        return (d_st,) + (None,) * 12


def pixel_losses(stacked, layout, color_ref, normal_ref=None, image_loss_spec=None, want_ssim=False, masked_prep=None):
    """The per-pixel losses both tick_init and tick_split evaluate (hmsdf.py:835-839,895-898 / 969-975,1064-1068) in one pass over
    render_mesh's channel-concatenated output.  stacked: [B,H,W,C]; layout: {buffer: (first channel, channels)}; returns a dict of
    MEANS: mask_mse = mse(shaded.a, ref.a); img = image_loss(shaded.rgb*ref.a, ref.rgb*ref.a) for image_loss_spec = (loss,
    tonemapper) (0 if None); msdf_pos_l1 / msdf_neg_l1 = the two L1 terms on msdf_image; normal_mse / normal_cos = mse and mean
    cosine between normalize(geometric_normal)*(1,-1,-1) and normalize(normal_ref); kd_grad / ks_grad / normal_grad = the three means of
    regularizer.material_smoothness_grad (before their lambdas; 0 for absent buffers); ssim = ssim_loss.ssim of the masked images."""
    ch = lambda k: layout[k][0] if k in layout else -1
    loss, tone = (-1, 0) if image_loss_spec is None else (_LOSS[image_loss_spec[0]], _TONE[image_loss_spec[1]])
    v = _PixelLossesFn.apply(stacked, color_ref, normal_ref, ch('shaded'), ch('geometric_normal') if normal_ref is not None else -1,
                             ch('msdf_image'), ch('kd_grad'), ch('ks_grad'), ch('normal_grad'), loss, tone, bool(want_ssim), masked_prep)
    masked = None
    if masked_prep is not None:          # `masked` [B,H,W,3]: shaded.rgb * ref.a (optionally as the LPIPS trunk input), differentiable
        v, masked = v
    d = dict(zip(PIXEL_LOSS_KEYS, v.unbind(0)))
    d['vec'] = v
    d['masked'] = masked
    return d


# ---- mask and image terms of tick_seq ------------------------------------------------------------------------------------------
SEQ_LOSS_KEYS = ('all_msk', 'cloth_msk', 'body_msk', 'all_img', 'cloth_img', 'body_img')


class _SeqLossesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, stacked, label, gt_all, gt_cloth, gt_body, cs, ca, loss, tonemap):
        st = stacked.contiguous().float()
        B, H, W, C = st.shape
        npix = B * H * W
        c4 = lambda t: t.float().expand(B, H, W, 4).contiguous()
        lab = label.float().expand(B, H, W).contiguous()
        ga, gc, gb = c4(gt_all), c4(gt_cloth), c4(gt_body)
        sums = torch.empty(6, dtype=torch.float32, device=st.device)
        L.call('seq_losses_fwd', st, C, cs, ca, lab, ga, gc, gb, npix, loss, tonemap, sums)
        ctx.save_for_backward(st, lab, ga, gc, gb)
        ctx.cfg = (C, cs, ca, loss, tonemap, npix)
        return sums * (1.0 / max(npix, 1))

    @staticmethod
    def backward(ctx, g):
        st, lab, ga, gc, gb = ctx.saved_tensors
        C, cs, ca, loss, tonemap, npix = ctx.cfg
        gs = (g.float() * (1.0 / max(npix, 1))).contiguous()
        d_st = torch.empty_like(st)
        L.call('seq_losses_bwd', st, C, cs, ca, lab, ga, gc, gb, npix, loss, tonemap, gs, d_st)
        return (d_st,) + (None,) * 8


def seq_losses(stacked, layout, label, gt_all, gt_cloth, gt_body, image_loss_spec):
    """The three mask MSEs and the three image losses of tick_seq (hmsdf.py:787-797,1110-1123) as MEANS, in SEQ_LOSS_KEYS order: masks
    alpha, label * alpha, (1 - label) * alpha from the coverage channel of `geometric_normal`; image losses ru.image_loss(shaded.rgb * mask,
    gt.rgb) for image_loss_spec = (loss, tonemapper).  stacked / layout: render_mesh's '_stacked' / '_layout'; label [B,H,W] (no gradient)."""
    cs = layout['shaded'][0]
    ca = layout['geometric_normal'][0] + layout['geometric_normal'][1] - 1
    return _SeqLossesFn.apply(stacked, label, gt_all, gt_cloth, gt_body, cs, ca, _LOSS[image_loss_spec[0]], _TONE[image_loss_spec[1]])


# ---- SDF edge regulariser ----------------------------------------------------------------------------------
class _SdfRegFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sdf, edges32, marks):
        s = sdf.reshape(-1).contiguous().float()
        sums = torch.empty(2, dtype=torch.float32, device=s.device)
        L.call('sdf_reg_fwd', s, edges32, edges32.shape[0], sums, marks)
        ctx.save_for_backward(s, edges32, sums)
        ctx.shape = sdf.shape
        return sums[0] / sums[1]

    @staticmethod
    def backward(ctx, g):
        s, edges32, sums = ctx.saved_tensors
        d = L.zeros_like(s)
        gs = g.reshape(1).contiguous().float()
        L.call('sdf_reg_bwd', s, edges32, edges32.shape[0], sums, gs, d)
        return d.reshape(ctx.shape), None, None


def sdf_reg_loss(sdf, edges32, marks=None):
    """geometry/hmsdf.py:162-170 compute_sdf_reg_loss (edges32: int32 [N_e,2] == all_edges).  marks (optional): float32 [sdf.numel()], zero on
    entry; receives 1 at both ends of every sign-changing edge (what d3h.sdf_mlp.prepare_backward wants)"""
    return _SdfRegFn.apply(sdf, edges32.contiguous(), marks)


# ---- xfm_points -------------------------------------------------------------------------------------------
class _XfmPointsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts, mtx, w):
        p = pts.contiguous().float()
        M = mtx.detach().contiguous().float()
        nb, n = M.shape[0], p.shape[1]
        out = torch.empty(nb, n, 4, dtype=torch.float32, device=p.device)
        L.call('xfm_points_fwd', p, p.shape[0], M, nb, n, w, out)
        ctx.save_for_backward(M)
        ctx.pshape = p.shape
        return out

    @staticmethod
    def backward(ctx, g):
        M, = ctx.saved_tensors
        nbp, n, _ = ctx.pshape
        d = torch.empty(ctx.pshape, dtype=torch.float32, device=g.device)
        L.call('xfm_points_bwd', g.contiguous().float(), nbp, M, M.shape[0], n, d)
        return d, None, None


def xfm_points(points, matrix, w=1.0):
    """[B or 1,V,3] x [B,4,4] -> [B,V,4]: M [p; w] per point (render/renderutils/ops.py:518-537).  The matrix is treated as a constant
    (callers with a trainable matrix use the matmul formulation)."""
    return _XfmPointsFn.apply(points, matrix, float(w))


class _LpipsHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f0, n1, w):
        B, C, H, W = f0.shape
        # the feature maps of a convolution stack fed with an NHWC-strided image are channels-last: read them as they are (a
        # .contiguous() here would be a transposing copy of 16-66 MB per layer, and another one for the gradient on the way back)
        cl = C % 64 == 0 and f0.is_contiguous(memory_format=torch.channels_last) and not f0.is_contiguous()
        fmt = torch.channels_last if cl else torch.contiguous_format
        f0c, n1c = f0.contiguous(memory_format=fmt).float(), n1.contiguous(memory_format=fmt).float()
        out = torch.empty(B, dtype=torch.float32, device=f0c.device)
        L.call('lpips_head_fwd', L.ptr_any(f0c), L.ptr_any(n1c), w, B, C, H * W, int(cl), out)
        ctx.save_for_backward(f0c, n1c, w)
        ctx.cl = cl
        return out

    @staticmethod
    def backward(ctx, g):
        f0c, n1c, w = ctx.saved_tensors
        B, C, H, W = f0c.shape
        d = torch.empty_like(f0c)                       # preserves the memory format
        L.call('lpips_head_bwd', L.ptr_any(f0c), L.ptr_any(n1c), w, B, C, H * W, int(ctx.cl), g.contiguous().float(), L.ptr_any(d))
        return d, None, None


def lpips_head(f0, n1, w):
    """one LPIPS layer: f0 [B,C,H,W] features of the prediction, n1 the unit-normalised features of the reference (constant), w [C] the
    layer's linear weights (constant) -> [B] = spatial mean of sum_c w_c (f0 / (|f0| + 1e-10) - n1)^2   (csrc/lpips_head.hip)"""
    return _LpipsHeadFn.apply(f0, n1.detach(), w.detach().reshape(-1).contiguous().float())


# ---- smoothness buffers of shade() (kd, kd_grad, ks_grad, normal_grad) in one pass --------------------------------------------
class _MaterialGradsFn(torch.autograd.Function):
    """render.py:72-74,88-91,104-105; csrc/material_grads.hip.  Outputs are separate contiguous tensors (their gradients arrive as such: no
    slice nodes); every input gradient is written completely by one backward launch."""

    @staticmethod
    def forward(ctx, tex, texj, nrm, nrmj, mask, mask_tap, want_kd=True):
        shp = tex.shape[:-1]
        c = lambda t: None if t is None else t.contiguous().float()
        tex, texj, nrm, nrmj, mask, mask_tap = c(tex), c(texj), c(nrm), c(nrmj), c(mask), c(mask_tap)
        n = tex.numel() // 6
        new = lambda: torch.empty(*shp, 3, dtype=torch.float32, device=tex.device)
        kd = new() if want_kd else None
        kdg, ksg = (new(), new()) if texj is not None else (None, None)
        ng = new() if nrm is not None else None
        L.call('material_grads_fwd', tex, texj, nrm, nrmj, mask, mask_tap, n, kd, kdg, ksg, ng)
        ctx.save_for_backward(tex, texj, nrm, nrmj, mask, mask_tap)
        ctx.shp = shp
        return kd, kdg, ksg, ng

    @staticmethod
    def backward(ctx, g_kd, g_kdg, g_ksg, g_ng):
        tex, texj, nrm, nrmj, mask, mask_tap = ctx.saved_tensors
        shp = ctx.shp
        n = tex.numel() // 6
        c = lambda t: None if t is None else t.contiguous().float()
        g_kd, g_kdg, g_ksg, g_ng = c(g_kd), c(g_kdg), c(g_ksg), c(g_ng)
        need_tex = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        need_nrm = nrm is not None and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3])
        d_tex = torch.empty(*shp, 6, dtype=torch.float32, device=tex.device) if need_tex else None
        d_texj = torch.empty_like(d_tex) if (need_tex and texj is not None) else None
        d_nrm = torch.empty(*shp, 3, dtype=torch.float32, device=tex.device) if need_nrm else None
        d_nrmj = torch.empty_like(d_nrm) if need_nrm else None
        if need_tex or need_nrm:
            L.call('material_grads_bwd', tex, texj, nrm, nrmj, mask, mask_tap, n, g_kd, g_kdg, g_ksg, g_ng, d_tex, d_texj, d_nrm, d_nrmj)
        return d_tex, d_texj, d_nrm, d_nrmj, None, None, None


def material_grads(all_tex, all_tex_jitter=None, gb_normal=None, nrm_jitter=None, mask=None, mask_tap=None, want_kd=True):
    """-> (kd, kd_grad, ks_grad, normal_grad); kd_grad / ks_grad are None without all_tex_jitter, normal_grad without the normal inputs, kd
    without want_kd"""
    return _MaterialGradsFn.apply(all_tex, all_tex_jitter, gb_normal, nrm_jitter, mask, mask_tap, want_kd)
