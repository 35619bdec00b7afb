"""Host side of csrc/raster.hip: rasterize / interpolate / antialias / texture with autograd.

Signatures follow nvdiffrast.torch as the reference calls it (render/render.py:37,72,102,381,400-403); the shim module
`nvdiffrast/torch.py` re-exports these.  Tensors: pos [B or 1, V, 4] clip space, tri [F,3] int32, images NHWC float32.

Pixel derivatives (nvdiffrast is not vendored; this paragraph is the pin of what is differentiated):
  - rasterize(grad_db=True): rast_db = (du/dX, du/dY, dv/dX, dv/dY) in pixel units is differentiable in pos.  Per covered pixel it is the
    closed form of csrc/raster.hip:resolve_pixel at the pixel's winning triangle, a function of that triangle's X_k = x_k/w_k, Y_k = y_k/w_k,
    q_k = 1/w_k and the pixel centre; its exact adjoint is added to the barycentric one.  The winner itself (the visibility decision) and
    empty pixels carry no gradient, as for rast.  grad_db=False (this module's default): rast_db is returned but is not differentiable.
  - interpolate(rast_db=..., diff_attrs='all' | [indices]): out_da [.., 2 len(diff_attrs)] = per listed channel c, in list order,
    (dA_c/dX, dA_c/dY) = (db.x e0 + db.z e1, db.y e0 + db.w e1), e0 = a0 - a2, e1 = a1 - a2.  It is differentiable in attr and rast_db,
    never in rast: out_da does not depend on (u, v).  Zero where nothing is covered, and so is its gradient.

Depth peeling (rasterize(prev_rast=...); nvdiffrast.torch.DepthPeeler):
  - The key of a fragment is the rasteriser's 64-bit (order_key(z/w) << 32) | (id + 1) (csrc/raster.hip: raster_key / raster_key_cross).
    Layer k reports, at each pixel, the covering fragment whose key is the SMALLEST KEY STRICTLY GREATER than the key layer k-1 reported
    there; a fragment covers under the same coverage, near-plane and depth-range tests as rasterize.  A pixel with no such fragment is
    empty (all four channels zero) and stays empty in every later layer.  So every fragment layer 0 competes over appears in exactly one
    layer, in increasing (depth, id) order.
  - Ties (this build's rule): fragments with equal z/w -- a duplicated or coplanar triangle -- are ALL reported, one per layer, in id order.
  - Layer 0 is rasterize bit for bit (DepthPeeler's first call is a plain rasterize: the same entry point and cost).  Every layer's rast
    and db are differentiable exactly as layer 0's, under the same grad_db / want_db rules: through that layer's winning triangle; the
    visibility decision carries no gradient.
  - How: a previous-key pass recomputes, per pixel, the key the previous layer's winner (rast.w) had there with the same device functions,
    so bit-identical to the key that won (no z-buffer is kept between layers), then the wave-per-triangle rasteriser admits a fragment to
    its atomic-min only above that key.  Peeled layers always take the wave path, never the tile-binned one (BIN_MIN_TRIS).
  - DepthPeeler keeps the previous layer's rast and refuses (RuntimeError) to peel from it once it was modified in place; after the last
    non-empty layer it returns empty layers, as nvdiffrast's fixed-count loop expects.

Range mode (rasterize(pos [V,4], ranges=...), nvdiffrast's):
  - ranges: an int32 CPU tensor [B,2] of (start, count) into tri; frame b rasterises triangles start_b .. start_b + count_b - 1 and rast is
    [B,H,W,4].  Ids in rast are ABSOLUTE indices into tri, plus one, so interpolate (2-D attr) and antialias (2-D pos) take the whole tri.
    Each frame equals the instanced rasterize(pos[None], tri[start:start + count]) with its ids offset by start, bit for bit (rast and db);
    d_pos comes back [V,4], summed over the frames.  Peeling works in range mode too.  Range mode takes the wave path only.
  - A 2-D pos without ranges, ranges that are not an int32 CPU [B,2] tensor (B >= 1), a negative start or count, or a range past F raise
    ValueError.  With a 3-D pos, ranges is ignored (instanced mode), as in nvdiffrast.

Antialias options:
  - pos may be 2-D [V,4] (range mode: shared by every frame); silhouettes come from the topology of the whole tri, as nvdiffrast's hash.
  - pos_gradient_boost: d_pos is multiplied by it; the colour gradient is unchanged.
  - topology_hash = antialias_construct_topology_hash(tri): the edge hash built once in buffers of its own and reused; results are
    bit-identical to calling without it.  A hash built for another triangle count raises ValueError.
  - Not covered: OpenGL-only options of nvdiffrast.  Peeled layers are shaded and blended by render/render.py:render_mesh(num_layers=...), one
    d3h.imgops.layer_composite_antialias step per layer (csrc/raster.hip: layer_composite_*_kernel).
"""
import os
import torch

from . import _lib as L


# The tile-binned rasteriser (csrc/raster.hip: raster_tile_kernel; north_star: "tile-binned differentiable rasterizer") is BUILT, bit-identical to
# the wave-per-triangle kernels and NOT selected by default: measured on four 1024^2 frames (profiles/r5_raster_vs_triangles.txt) it is slower at
# every mesh size tried -- 9 k / 37 k / 148 k / 593 k triangles: 181 / 313 / 677 / 2 333 us against 70 / 87 / 181 / 524 us.  Three passes over the
# triangles (count, fill, per-tile) with gathered vertex loads cost more than the one wave-uniform pass they replace, and the covered 11 % of the
# tiles carry all the work.  D3H_RASTER_BIN_MIN=<triangles> selects it from that mesh size on (tests force it with BIN_MIN_TRIS = 1).
BIN_MIN_TRIS = int(os.environ.get('D3H_RASTER_BIN_MIN', str(1 << 30)))
BIN_PAIRS_PER_TRI = 4


def _bstride(t):
    """batch stride in elements, 0 for a broadcast batch of 1"""
    return 0 if t.shape[0] == 1 else t.shape[1] * t.shape[2]


class _Scratch:
    """per-device reusable scratch buffers (z-buffer, big-triangle list, edge hash)"""
    bufs = {}

    @classmethod
    def get(cls, name, n, dev, dtype=torch.uint8):
        """at least `n` elements of `dtype` (one dtype per name: the type of the C parameter the buffer is passed for)"""
        key = (name, str(dev))
        b = cls.bufs.get(key)
        if b is None or b.numel() < n:
            b = torch.empty(int(n), dtype=dtype, device=dev)
            cls.bufs[key] = b
        return b


class _RasterizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, tri, H, W, nb, want_db=True, grad_db=False, prev=None, ranges=None):
        pos_c = pos.contiguous().float()
        dev = pos.device
        nv, nf = pos_c.shape[1], tri.shape[0]
        rast = torch.empty(nb, H, W, 4, dtype=torch.float32, device=dev)
        # (want_db False: the caller reads no pixel derivatives -- 16 bytes per pixel the resolve pass does not write; an empty tensor comes back)
        db = torch.empty((nb, H, W, 4) if want_db else (0,), dtype=torch.float32, device=dev)
        zbuf = _Scratch.get('zbuf', nb * H * W, dev, torch.int64)
        big, big_cap = None, 0
        if prev is not None or ranges is not None:
            # a peeled layer (prev: the previous layer's rast) and / or range mode (ranges: (device [nb, 2] int32, largest count)): the
            # wave-per-triangle path of d3h_rasterize_peel_fwd; the previous keys go to a scratch of their own, next to the shared z-buffer
            pk = _Scratch.get('peel_keys', nb * H * W, dev, torch.int64) if prev is not None else None
            rg, max_count = ranges if ranges is not None else (None, 0)
            L.call('rasterize_peel_fwd', pos_c, _bstride(pos_c), tri, nf, nb, H, W, rg, max_count, prev, pk, zbuf, rast, db if want_db else None)
        else:
            if nf >= BIN_MIN_TRIS:
                # tile-binned rasteriser (csrc/raster.hip: raster_tile_kernel): header + room for BIN_PAIRS_PER_TRI (triangle, tile) pairs per
                # triangle and frame; a render that needs more falls back on the device to the wave-per-triangle kernels -- no host read-back
                nt = nb * (-(-W // 32)) * (-(-H // 32))
                big_cap = min(3 * nt + 8 + BIN_PAIRS_PER_TRI * nf * nb + nf, (1 << 31) - 1)
                big = _Scratch.get('bins', big_cap, dev, torch.int32)
            L.call('rasterize_fwd', pos_c, nv, _bstride(pos_c), tri, nf, nb, H, W, zbuf, big, big_cap, rast, db if want_db else None)
        ctx.save_for_backward(pos_c, tri, rast)
        ctx.dims = (H, W, nb)
        if not (grad_db and want_db):
            ctx.mark_non_differentiable(db)
        # (without this the engine hands the backward a zero-filled [nb, H, W, 4] tensor for `db` on every step: a 67 MB fill nobody reads)
        ctx.set_materialize_grads(False)
        ctx.zeros = L.zeros_like(pos) if ctx.needs_input_grad[0] else None      # d_pos, filled ahead of the backward (d3h/mtets.py)
        return rast, db

    @staticmethod
    def backward(ctx, g_rast, g_db):
        pos, tri, rast = ctx.saved_tensors
        H, W, nb = ctx.dims
        d_pos, ctx.zeros = getattr(ctx, 'zeros', None), None
        if d_pos is None:
            d_pos = L.zeros_like(pos)
        if g_db is not None:                   # the pixel derivatives were differentiated: one pass for both gradients
            L.call('rasterize_bwd_db', pos, _bstride(pos), tri, nb, H, W, rast, g_rast.contiguous() if g_rast is not None else None,
                   g_db.contiguous(), d_pos)
            return (d_pos,) + (None,) * 8
        if g_rast is None:                     # nothing flowed into the barycentrics: the position gradient through them is zero
            return (d_pos,) + (None,) * 8
        L.call('rasterize_bwd', pos, _bstride(pos), tri, nb, H, W, rast, g_rast.contiguous(), d_pos)
        return (d_pos,) + (None,) * 8


def _check_ranges(ranges, nf):
    """refuses anything but an int32 CPU tensor [B, 2] of (start, count) rows inside [0, nf]; -> the largest count (it sizes the grid)"""
    if not (isinstance(ranges, torch.Tensor) and ranges.device.type == 'cpu' and ranges.dtype == torch.int32 and ranges.dim() == 2
            and ranges.shape[1] == 2 and ranges.shape[0] > 0):
        got = (ranges.dtype, ranges.device.type, tuple(ranges.shape)) if isinstance(ranges, torch.Tensor) else type(ranges).__name__
        raise ValueError(f'rasterize: ranges must be an int32 CPU tensor [B, 2] with B >= 1, not {got}')
    r = ranges.long()
    if bool((r < 0).any()):
        raise ValueError('rasterize: ranges holds a negative start or count')
    if bool((r[:, 0] + r[:, 1] > nf).any()):
        raise ValueError(f'rasterize: a range reaches past the {nf} triangles of tri')
    return int(r[:, 1].max())


def rasterize(pos, tri, resolution, nb=None, want_db=True, grad_db=False, prev_rast=None, ranges=None):
    """-> (rast [B,H,W,4] = (u, v, z/w, tri_id+1), rast_db [B,H,W,4] = (du/dX, du/dY, dv/dX, dv/dY); want_db False (extension): rast_db is None).
    grad_db True: rast_db is differentiable in pos (module docstring); False: it is returned without a gradient.
    prev_rast: the previous depth-peeling layer (a rast of these pos / tri / ranges) -> the next one.  ranges (with a 2-D pos [V,4]): range
    mode, an int32 CPU tensor [B,2] of (start, count) into tri; ignored with a 3-D pos, as in nvdiffrast (module docstring)."""
    H, W = int(resolution[0]), int(resolution[1])
    tri = tri.contiguous()
    rg = None
    if pos.dim() == 2:
        if ranges is None:
            raise ValueError('rasterize: a 2-D pos [V, 4] needs ranges (range mode); instanced mode takes pos [B, V, 4]')
        if pos.shape[1] != 4:
            raise ValueError(f'rasterize: pos must be [V, 4] in range mode, not {tuple(pos.shape)}')
        max_count = _check_ranges(ranges, tri.shape[0])
        nb = ranges.shape[0]
        rg = ranges.contiguous()
        if pos.is_cuda:                        # (a pageable copy would stall the host until the device drained its queue)
            rg = rg.pin_memory().to(pos.device, non_blocking=True)
        rg = (rg, max_count)
        pos = pos[None]
    nb = pos.shape[0] if nb is None else nb
    prev = None
    if prev_rast is not None:
        if tuple(prev_rast.shape) != (nb, H, W, 4) or prev_rast.dtype != torch.float32 or prev_rast.device != pos.device:
            raise ValueError(f'rasterize: prev_rast must be a float32 [{nb}, {H}, {W}, 4] raster on {pos.device}')
        prev = prev_rast.detach().contiguous()
    rast, db = _RasterizeFn.apply(pos, tri, H, W, nb, bool(want_db), bool(grad_db), prev, rg)
    return rast, (db if want_db else None)


class _InterpolateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, rast, tri, rast_db, diff_idx):
        attr_c = attr.contiguous().float()
        rast_c = rast.contiguous()
        nb, H, W = rast_c.shape[:3]
        na = attr_c.shape[2]
        db_c = rast_db.contiguous().float() if rast_db is not None else None
        out = torch.empty(nb, H, W, na, dtype=torch.float32, device=attr.device)
        if diff_idx is None:                   # no derivatives, or every channel in order
            out_da = torch.empty(nb, H, W, 2 * na, dtype=torch.float32, device=attr.device) if rast_db is not None else None
            L.call('interpolate_fwd', attr_c, _bstride(attr_c), na, rast_c, tri, db_c, nb, H, W, out, out_da)
        else:
            out_da = torch.empty(nb, H, W, 2 * diff_idx.numel(), dtype=torch.float32, device=attr.device)
            L.call('interpolate_fwd_da', attr_c, _bstride(attr_c), na, rast_c, tri, db_c, diff_idx, diff_idx.numel(), nb, H, W, out, out_da)
        ctx.save_for_backward(attr_c, rast_c, tri, db_c, diff_idx)
        if out_da is None:
            out_da = out.new_empty(0)
            ctx.mark_non_differentiable(out_da)
        ctx.set_materialize_grads(False)
        return out, out_da

    @staticmethod
    def backward(ctx, g_out, g_da):
        attr, rast, tri, db, diff_idx = ctx.saved_tensors
        nb, H, W = rast.shape[:3]
        na = attr.shape[2]
        need_attr, need_rast, need_db = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[3]
        if g_da is None and g_out is None:
            return None, None, None, None, None
        d_attr = L.zeros_like(attr) if need_attr else None
        d_rast = torch.empty_like(rast) if need_rast else None
        if g_da is None:
            L.call('interpolate_bwd', attr, _bstride(attr), na, rast, tri, g_out.contiguous(), nb, H, W, d_attr, d_rast)
            return d_attr, d_rast, None, None, None
        d_db = torch.empty_like(db) if need_db else None
        nidx = na if diff_idx is None else diff_idx.numel()
        L.call('interpolate_bwd_da', attr, _bstride(attr), na, rast, tri, db, diff_idx, nidx, g_out.contiguous() if g_out is not None else None,
               g_da.contiguous(), nb, H, W, d_attr, d_rast, d_db)
        return d_attr, d_rast, None, d_db, None


def interpolate(attr, rast, tri, rast_db=None, diff_attrs=None):
    """nvdiffrast.interpolate: (out [B,H,W,A], out_da [B,H,W,2 len(diff_attrs)] or None).  diff_attrs: None, 'all' or a list of channel
    indices (their derivatives in list order); out_da is produced only with rast_db and is differentiable in attr and rast_db (module
    docstring)."""
    if attr.dim() == 2:
        attr = attr[None]
    idx = None
    if diff_attrs is not None and rast_db is not None and not (isinstance(diff_attrs, str) and diff_attrs == 'all'):
        if isinstance(diff_attrs, str):
            raise ValueError(f"interpolate: diff_attrs must be None, 'all' or a list of channel indices, not {diff_attrs!r}")
        lst = [int(c) for c in diff_attrs]
        na = attr.shape[-1]
        if any(not 0 <= c < na for c in lst):
            raise ValueError(f'interpolate: diff_attrs {lst} out of range for {na} attribute channels')
        idx = torch.tensor(lst, dtype=torch.int32).to(attr.device)
    out, da = _InterpolateFn.apply(attr, rast, tri.contiguous(), rast_db if diff_attrs is not None else None, idx)
    return out, (da if da.numel() else None)


class _GBufferFn(torch.autograd.Function):
    """every interpolation of one render layer in one pass (csrc/raster.hip: gbuffer_*): the vertex-attribute groups of a packed
    attribute array, a per-face attribute gathered by triangle id, and the coverage mask"""

    @staticmethod
    def forward(ctx, attr, face_attr, rast, tri, widths, need, want_mask, pos):
        attr_c = attr.contiguous().float()
        rast_c = rast.contiguous()
        nb, H, W = rast_c.shape[:3]
        na = attr_c.shape[2]
        dev = attr.device
        w4 = list(widths) + [0] * (4 - len(widths))
        outs = [torch.empty(nb, H, W, w, dtype=torch.float32, device=dev) if (k < len(widths) and need[k]) else None for k, w in enumerate(w4)]
        fa = face_attr.contiguous().float() if face_attr is not None else None
        fw = fa.shape[2] if fa is not None else 0
        face_out = torch.empty(nb, H, W, fw, dtype=torch.float32, device=dev) if fa is not None else None
        if fa is not None and fa.shape[1] == 0:            # a mesh without faces covers nothing: zeros, and no pointer to gather from
            face_out.zero_()
        mask = torch.empty(nb, H, W, 1, dtype=torch.float32, device=dev) if want_mask else None
        L.call('gbuffer_fwd', attr_c, _bstride(attr_c), na, fa, _bstride(fa) if fa is not None else 0, fw, rast_c, tri, nb, H, W, outs[0], w4[0],
               outs[1], w4[1], outs[2], w4[2], outs[3], w4[3], face_out if (fa is not None and fa.shape[1] > 0) else None, mask)
        # `pos` (the clip positions `rast` was rasterised from; rast itself then arrives detached): the rasteriser's backward runs inside this
        # node's backward pass -- d(barycentrics) never leaves the kernel (csrc/raster.hip: gbuffer_bwd_kernel<true>)
        pos_c = pos.contiguous().float() if pos is not None else None
        ctx.save_for_backward(attr_c, rast_c, tri, pos_c)
        ctx.meta = (w4, fa.shape if fa is not None else None)
        ctx.set_materialize_grads(False)       # outputs nobody differentiates arrive as None (the backward skips them), not as zero-filled images
        empty = attr_c.new_empty(0)
        ret = [o if o is not None else empty for o in outs[:len(widths)]]
        ret.append(face_out if face_out is not None else empty)
        ret.append(mask if mask is not None else empty)
        ctx.mark_non_differentiable(ret[-1])
        return tuple(ret)

    @staticmethod
    def backward(ctx, *gs):
        attr, rast, tri, pos = ctx.saved_tensors
        w4, fshape = ctx.meta
        nb, H, W = rast.shape[:3]
        na = attr.shape[2]
        ng = len(gs) - 2
        g4 = [None] * 4
        for k in range(ng):
            if gs[k] is not None and gs[k].numel():
                g4[k] = gs[k].contiguous().float()
        g_face = gs[ng].contiguous().float() if (gs[ng] is not None and gs[ng].numel() and fshape is not None and fshape[1] > 0) else None
        d_attr = L.zeros_like(attr) if ctx.needs_input_grad[0] else None
        d_face = L.zeros(fshape, torch.float32, attr.device) if (fshape is not None and ctx.needs_input_grad[1] and g_face is not None) else None
        fb = (fshape[1] * fshape[2] if fshape[0] > 1 else 0) if fshape is not None else 0
        if pos is not None and ctx.needs_input_grad[7]:
            d_pos = L.zeros_like(pos)
            L.call('gbuffer_raster_bwd', attr, _bstride(attr), na, fb, fshape[2] if fshape is not None else 0, rast, tri, nb, H, W, g4[0], w4[0],
                   g4[1], w4[1], g4[2], w4[2], g4[3], w4[3], g_face, d_attr, d_face, pos, _bstride(pos), d_pos)
            return d_attr, d_face, None, None, None, None, None, d_pos
        d_rast = torch.empty_like(rast) if ctx.needs_input_grad[2] else None
        L.call('gbuffer_bwd', attr, _bstride(attr), na, fb, fshape[2] if fshape is not None else 0, rast, tri, nb, H, W, g4[0], w4[0], g4[1], w4[1],
               g4[2], w4[2], g4[3], w4[3], g_face, d_attr, d_face, d_rast)
        return d_attr, d_face, d_rast, None, None, None, None, None


def gbuffer(attr, widths, rast, tri, need=None, face_attr=None, want_mask=True, raster_pos=None):
    """attr [B or 1, V, sum(widths)] -> (list of [B,H,W,w_k] (None where need[k] is False), face image [B,H,W,fw] or None,
    mask [B,H,W,1] or None).  Replaces one dr.interpolate per attribute + the (f, f, f)-indexed face-normal interpolation +
    `rast[..., -1:] > 0` of render/render.py:257-267,283,328,66."""
    if attr.dim() == 2:
        attr = attr[None]
    if face_attr is not None and face_attr.dim() == 2:
        face_attr = face_attr[None]
    widths = tuple(int(w) for w in widths)
    assert 1 <= len(widths) <= 4 and sum(widths) == attr.shape[-1]
    need = tuple(bool(n) for n in (need if need is not None else [True] * len(widths)))
    # raster_pos: the clip positions `rast` = rasterize(raster_pos, tri) came from, for a raster with NO other differentiable consumer: the
    # rasteriser's backward then runs inside this op's backward pass (d(barycentrics) is never written out) and `rast` is cut from the graph
    if raster_pos is not None and torch.is_grad_enabled() and raster_pos.requires_grad and rast.requires_grad:
        r = _GBufferFn.apply(attr, face_attr, rast.detach(), tri.contiguous(), widths, need, bool(want_mask), raster_pos)
    else:
        r = _GBufferFn.apply(attr, face_attr, rast, tri.contiguous(), widths, need, bool(want_mask), None)
    groups = [r[k] if need[k] else None for k in range(len(widths))]
    return groups, (r[len(widths)] if face_attr is not None else None), (r[len(widths) + 1] if want_mask else None)


def aux_buffers(clip, rast, db, tri, gb_pos, view_pos, want_z=True, want_depth=True, want_invdepth=True):
    """forward-only z_grad [B,H,W,3] (render.py:291-299), depth / invdepth [B,H,W,1] (render.py:197-199) in one pass -- the buffers of a
    render layer that carry no gradient.  clip [B,V,4]; rast, db [B,H,W,4]; gb_pos [B,H,W,3]; view_pos [B or 1, 1, 1, 3] (or [B,3])"""
    nb, H, W = rast.shape[:3]
    dev = rast.device
    with torch.no_grad():
        clip_c = clip.detach().contiguous().float() if want_z else None
        z = torch.empty(nb, H, W, 3, dtype=torch.float32, device=dev) if want_z else None
        dep = torch.empty(nb, H, W, 1, dtype=torch.float32, device=dev) if want_depth else None
        inv = torch.empty(nb, H, W, 1, dtype=torch.float32, device=dev) if want_invdepth else None
        gp = vp = None
        vstride = 0
        if want_depth or want_invdepth:
            gp = gb_pos.detach().contiguous().float()
            vp = view_pos.detach().reshape(-1, 3).contiguous().float()
            vstride = 3 if vp.shape[0] > 1 else 0
            assert vp.shape[0] in (1, nb)
        L.call('aux_buffers_fwd', clip_c, _bstride(clip_c) if want_z else 0, rast.contiguous(), db.contiguous() if want_z else None,
               tri.contiguous() if want_z else None, gp, vp, vstride, nb, H, W, z, dep, inv)
    return z, dep, inv


def _hash_cap(nf):
    cap = 1024
    while cap < 12 * max(nf, 1):
        cap *= 2
    return cap


def _hash_for(tri):
    nf = tri.shape[0]
    cap = _hash_cap(nf)
    dev = tri.device
    kv = _Scratch.get('aa_keys_vals', cap * 2, dev, torch.int64)          # keys [cap] uint64 | vals [2 cap] int32, contiguous: the library fills both at once
    keys, vals = kv[:cap], kv[cap:cap * 2].view(torch.int32)
    L.call('antialias_hash', tri, nf, keys, vals, cap)
    return keys, vals, cap


class TopologyHash:
    """antialias_construct_topology_hash(tri): the edge hash of d3h_antialias_hash built once, in buffers of its own (not the shared
    scratch), for antialias(..., topology_hash=...) to reuse instead of rebuilding it on every call.  Valid for this triangle count
    (antialias refuses another one) and meant for this very `tri`: the hash is a function of its contents."""

    def __init__(self, tri):
        tri = tri.contiguous()
        nf = tri.shape[0]
        cap = _hash_cap(nf)
        kv = torch.empty(cap * 2, dtype=torch.int64, device=tri.device)          # one allocation: keys | vals, as _hash_for's
        self.keys, self.vals, self.cap, self.nf = kv[:cap], kv[cap:].view(torch.int32), cap, nf
        L.call('antialias_hash', tri, nf, self.keys, self.vals, cap)


def antialias_construct_topology_hash(tri):
    """nvdiffrast.antialias_construct_topology_hash: -> a TopologyHash for antialias(..., topology_hash=...)"""
    return TopologyHash(tri)


def _edge_flags(pos_c, tri, nb, H, W, topology_hash=None):
    """[nb, nf] uint8: the silhouette-edge bits of every triangle in every frame (csrc/raster.hip:aa_edge_flags_kernel)"""
    nf = tri.shape[0]
    if topology_hash is None:
        keys, vals, cap = _hash_for(tri)
    else:
        keys, vals, cap = topology_hash.keys, topology_hash.vals, topology_hash.cap
    flags = torch.empty(nb, max(nf, 1), dtype=torch.uint8, device=pos_c.device)
    L.call('antialias_flags', pos_c, _bstride(pos_c), tri, nf, nb, keys, vals, cap, H, W, flags)
    return flags


class _AntialiasFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, rast, pos, tri, topology_hash=None, pos_gradient_boost=1.0):
        color_c, rast_c, pos_c = color.contiguous().float(), rast.contiguous(), pos.contiguous().float()
        nb, H, W, C = color_c.shape
        flags = _edge_flags(pos_c, tri, nb, H, W, topology_hash)        # per render; the backward reuses them (nb x nf bytes)
        out = torch.empty_like(color_c)
        L.call('antialias_fwd', color_c, rast_c, pos_c, _bstride(pos_c), tri, tri.shape[0], flags, nb, H, W, C, out)
        ctx.save_for_backward(color_c, rast_c, pos_c, tri, flags)
        ctx.boost = float(pos_gradient_boost)
        return out

    @staticmethod
    def backward(ctx, g_out):
        color, rast, pos, tri, flags = ctx.saved_tensors
        nb, H, W, C = color.shape
        g_color = torch.empty_like(color)
        d_pos = L.zeros_like(pos) if ctx.needs_input_grad[2] else None
        L.call('antialias_bwd', color, rast, pos, _bstride(pos), tri, tri.shape[0], flags, nb, H, W, C, g_out.contiguous(), g_color, d_pos)
        if d_pos is not None and ctx.boost != 1.0:
            d_pos.mul_(ctx.boost)
        return g_color, None, d_pos, None, None, None


def antialias(color, rast, pos, tri, topology_hash=None, pos_gradient_boost=1.0):
    """nvdiffrast.antialias.  pos [B or 1, V, 4], or [V, 4] (range mode: shared by every frame, d_pos summed over them); silhouettes come
    from the topology of the whole tri.  topology_hash: antialias_construct_topology_hash(tri), reused instead of rebuilt (bit-identical
    results).  pos_gradient_boost: d_pos is multiplied by it; the colour gradient is not."""
    tri = tri.contiguous()
    if topology_hash is not None:
        if not isinstance(topology_hash, TopologyHash):
            raise TypeError(f'antialias: topology_hash must come from antialias_construct_topology_hash, not {type(topology_hash).__name__}')
        if topology_hash.nf != tri.shape[0]:
            raise ValueError(f'antialias: topology_hash was built for {topology_hash.nf} triangles, tri has {tri.shape[0]}')
    if pos.dim() == 2:
        pos = pos[None]
    return _AntialiasFn.apply(color, rast, pos, tri, topology_hash, float(pos_gradient_boost))


class _TextureFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uv):
        tex_c, uv_c = tex.contiguous().float(), uv.contiguous().float()
        nb, H, W = uv_c.shape[:3]
        TH, TW, C = tex_c.shape[1:]
        out = torch.empty(nb, H, W, C, dtype=torch.float32, device=tex.device)
        bs = 0 if tex_c.shape[0] == 1 else TH * TW * C
        L.call('texture_fwd', tex_c, bs, TH, TW, C, uv_c, nb, H, W, out)
        ctx.save_for_backward(uv_c)
        ctx.tshape = tuple(tex_c.shape)
        return out

    @staticmethod
    def backward(ctx, g_out):
        (uv,) = ctx.saved_tensors
        nb, H, W = uv.shape[:3]
        B, TH, TW, C = ctx.tshape
        d_tex = L.zeros(ctx.tshape, torch.float32, uv.device)
        bs = 0 if B == 1 else TH * TW * C
        L.call('texture_bwd', bs, TH, TW, C, uv, nb, H, W, g_out.contiguous(), d_tex)
        return d_tex, None


def texture(tex, uv, filter_mode='linear', boundary_mode='clamp', **kw):
    """nvdiffrast.texture for the one mode the reference uses (render/render.py:72,102): bilinear, clamp; no uv gradient
    (the jittered lookup coordinates are constants)."""
    if filter_mode != 'linear' or boundary_mode != 'clamp':
        raise NotImplementedError('d3h.texture: only filter_mode="linear", boundary_mode="clamp"')
    return _TextureFn.apply(tex, uv)
