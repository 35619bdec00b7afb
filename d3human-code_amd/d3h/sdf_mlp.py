"""Host side of the fused SDF-query kernels (csrc/sdf_mlp.hip): weight packing + forward (+ backward).

The network shape is the reference's fixed working point (train.py:1618-1621): MLP(n_freq=6, d_hidden=256,
n_hidden=6, skip_in=[3]) from geometry/mlp.py:10-32; any other shape raises (no silent fallback).
"""
import os

import torch
from d3h._lib import cur_stream as _cur_stream

from . import _lib as L
from . import gradarena as _GA

HIDDEN_KEYS = (2, 4, 6, 10, 12)
SPARSE_BACKWARD = True      # skip 16-point tiles whose upstream gradient is identically zero (exact)
# The training sweep runs WITHOUT the activation save and the backward recomputes the activations of the tiles it visits (the active ~15 % of a
# grid sweep) with the same kernel -- bit-identical values -- instead of storing 1.88 GB per 262 144 points of which ~15 % was read back.
# Only with the split-operand kernels (the recompute pass is one); D3H_SDF_RECOMPUTE=0 restores the store.
RECOMPUTE = os.environ.get('D3H_SDF_RECOMPUTE', '1') != '0' 
# Every sweep runs its GEMMs on the low-precision matrix pipe with each fp32 operand split into planes (csrc/sdf_mlp_x3.h: fp32-level accuracy):
# three bf16 planes and six products per block ("bf16x3"), or two fp16 planes and three products ("fp16x2", gradient-valued operands scaled by
# a power of two per launch).  D3H_SDF_X3=0 selects the exact-f32 MFMA kernels for everything.  sweep_plan() below is the whole rule.
X3 = os.environ.get('D3H_SDF_X3', '1') != '0'
H2 = os.environ.get('D3H_SDF_H2', '1') != '0'              # '0': every sweep stays on bf16 x 3
H2_BWD = os.environ.get('D3H_SDF_H2_BWD', '1') != '0'      # '0': the data-backward sweeps stay on bf16 x 3 (A/B)
H2_JVP = os.environ.get('D3H_SDF_H2_JVP', '1') != '0'      # '0': the tangent sweep of the eikonal term stays on bf16 x 3 (A/B)
TIMING = None      # bench.py sets this to a list: (start_event, end_event, n_points) per forward launch, on the launch stream


def sweep_plan(x3, h2, h2_jvp, h2_bwd):
    """the arithmetic of (the forward-type sweeps: grid sweep, eikonal forward, recompute of the sparse backward; the tangent sweep of the
    eikonal term; the data-backward sweeps) for one setting of the four switches"""
    if not x3:
        return 'f32', 'f32', 'f32'
    if not h2:
        return 'bf16x3', 'bf16x3', 'bf16x3'
    return 'fp16x2', 'fp16x2' if h2_jvp else 'bf16x3', 'fp16x2' if h2_bwd else 'bf16x3'


def check_shape(sd, prefix='net.'):
    want = {0: (256, 39), 2: (256, 256), 4: (256, 256), 6: (256, 256), 8: (256, 295), 10: (256, 256), 12: (256, 256),
            14: (1, 256)}
    for i, shp in want.items():
        w = sd.get(f'{prefix}{i}.weight')
        if w is None or tuple(w.shape) != shp:
            raise RuntimeError(f'd3h.sdf_mlp: unsupported MLP shape at {prefix}{i} '
                               f'({None if w is None else tuple(w.shape)}; kernel is built for n_freq=6,d_hidden=256,'
                               f'n_hidden=6,skip_in=[3])')


class Pack:
    """one fragment-order copy of the network's weights (csrc/sdf_mlp_layout.h, csrc/sdf_mlp_x3.h): the buffer `t` together with what the
    kernels need to know to read it -- its arithmetic and whether it is the transposed (data-backward) form.  The kind travels with the
    object: wrap a copy of the buffer as Pack(t.clone(), p.arith, p.transposed)."""
    __slots__ = ('t', 'arith', 'transposed')
    _PLANES = {'f32': 0, 'bf16x3': 3, 'fp16x2': 2}

    def __init__(self, t, arith, transposed=False):
        if arith not in self._PLANES:
            raise ValueError(f'd3h.sdf_mlp: unknown pack arithmetic {arith!r}')
        self.t, self.arith, self.transposed = t, arith, bool(transposed)

    @property
    def planes(self):
        """the `int planes` of the C ABI: operand planes per fp32 value, 0 for the exact-f32 pack"""
        return self._PLANES[self.arith]


# (arith, transposed) -> (size query, pack entry, fwd entry); the forward packs carry the biases and the head, the transposed ones three weights
_PACK_KINDS = {('f32', False): ('sdf_mlp_wpack_floats', 'sdf_mlp_pack', 'sdf_mlp_fwd'),
               ('bf16x3', False): ('sdf_mlp_wpack3_dwords', 'sdf_mlp_pack3', 'sdf_mlp_fwd_x3'),
               ('fp16x2', False): ('sdf_mlp_wpackh2_dwords', 'sdf_mlp_pack_h2', 'sdf_mlp_fwd_h2'),
               ('f32', True): ('sdf_mlp_wpackt_floats', 'sdf_mlp_pack_t', None),
               ('bf16x3', True): ('sdf_mlp_wpackt3_dwords', 'sdf_mlp_pack_t3', None),
               ('fp16x2', True): ('sdf_mlp_wpackth2_dwords', 'sdf_mlp_pack_t_h2', None)}


def _pack(views, arith, transposed, out=None):
    """(W0, b0, Wh[5,256,256], bh[5,256], W8, b8, W14, b14) contiguous fp32 -> Pack"""
    size, entry, _ = _PACK_KINDS[(arith, transposed)]
    w0, b0, wh, bh, w8, b8, w14, b14 = views
    if out is None:
        out = torch.empty(L.query(size), dtype=torch.float32 if arith == 'f32' else torch.int32, device=w0.device)
    if transposed:
        L.call(entry, w0, wh, w8, out)
    else:
        L.call(entry, w0, b0, wh, bh, w8, b8, w14, b14, out)
    return Pack(out, arith, transposed)


def pack_weights(sd, arith='f32', transposed=False, prefix='net.', out=None):
    """state_dict-like {net.i.weight, net.i.bias} -> the Pack of that arithmetic ('f32', 'bf16x3', 'fp16x2'), forward or transposed form"""
    check_shape(sd, prefix)
    g = lambda k: sd[prefix + k].detach().contiguous().float()
    wh = torch.stack([g(f'{i}.weight') for i in HIDDEN_KEYS]).contiguous()
    bh = torch.stack([g(f'{i}.bias') for i in HIDDEN_KEYS]).contiguous()
    return _pack((g('0.weight'), g('0.bias'), wh, bh, g('8.weight'), g('8.bias'), g('14.weight'), g('14.bias')), arith, transposed, out)


def forward(x, pack, deform=None, disp=0.0, save=False, want_xdef=False, max_cus=0):
    """sdf[n] (and optionally the saved activations / deformed points) for points x[n,3] on the arithmetic of `pack` (a forward Pack).
    max_cus: a launch of fewer than 1024 point tiles uses at most this many CUs (0 = the chip), so that another stream's kernels find
    free ones next to it."""
    if not isinstance(pack, Pack) or pack.transposed:
        raise TypeError('d3h.sdf_mlp.forward: `pack` must be a forward Pack (pack_weights / PackedWeights), got '
                        + ('a transposed Pack' if isinstance(pack, Pack) else type(pack).__name__))
    x = x.contiguous().float()
    n = x.shape[0]
    sdf = torch.empty(n, dtype=torch.float32, device=x.device)
    act = torch.empty(L.query('sdf_mlp_act_floats', n), dtype=torch.float32, device=x.device) if save else None
    xdef = torch.empty(n, 3, dtype=torch.float32, device=x.device) if want_xdef else None
    d = deform.contiguous().float() if deform is not None else None
    ev = None
    if TIMING is not None and x.is_cuda:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    L.call(_PACK_KINDS[(pack.arith, False)][2], x, d, disp, pack.t, sdf, xdef, act, n, max_cus)
    if ev is not None:
        ev[1].record()
        TIMING.append((ev[0], ev[1], n))
    if save or want_xdef:
        return sdf, act, xdef
    return sdf


# ---- one flat parameter vector --------------------------------------------------------------------------------------------------
# The 16 parameter tensors of the network are concatenated ONCE per iteration into a flat vector in "arena order" (the order the
# gradient kernels write: W0, b0, the five 256x256 hidden weights stacked, their biases stacked, W8 (the 295-wide skip layer), b8, W14,
# b14).  The sweep and the eikonal term both consume that vector, so the autograd engine sums their two gradients with ONE 1.66 MB add
# (it used to be 16 small adds, 5 us apart, on the launch-bound tail of the backward), the weight packs read views of it (no
# torch.stack), and the backward hands the 16 parameter gradients back as views of one arena (no copies).
ARENA_SIZES = [256 * 39, 256, 5 * 65536, 5 * 256, 256 * 295, 256, 256, 1]
ARENA_FLOATS = sum(ARENA_SIZES)
_ARENA_PERM = [0, 1, 2, 4, 6, 10, 12, 3, 5, 7, 11, 13, 8, 9, 14, 15]          # positions in _PARAM_ORDER, in arena order
_ARENA_SHAPES = [(256, 39), (256,)] + [(256, 256)] * 5 + [(256,)] * 5 + [(256, 295), (256,), (1, 256), (1,)]


class _FlatParams(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *params):
        for k, shp in zip(_ARENA_PERM, _ARENA_SHAPES):
            if tuple(params[k].shape) != shp:
                raise RuntimeError(f'd3h.sdf_mlp: unsupported MLP shape {tuple(params[k].shape)} for net.{_PARAM_ORDER[k]} (kernel is built for '
                                   f'n_freq=6, d_hidden=256, n_hidden=6, skip_in=[3])')
        ctx.leaves = [params[k] for k in _ARENA_PERM]
        return torch.cat([params[k].detach().reshape(-1).float() for k in _ARENA_PERM])

    @staticmethod
    def backward(ctx, g):
        # frame-parallel step: the 16 gradients live in the step's all-reduce arena (d3h.gradarena) -- one 1.66 MB copy of the summed
        # vector into its block, the views below are then slices of the bucket the collective runs on
        blk = _GA.block_for(ctx.leaves)
        ctx.leaves = None
        if blk is not None:
            blk.copy_(g)
            g = blk
        out = [None] * 16
        o = 0
        for k, shp in zip(_ARENA_PERM, _ARENA_SHAPES):
            n = 1
            for d in shp:
                n *= d
            out[k] = g[o:o + n].view(shp)
            o += n
        return tuple(out)


def arena_views(flat):
    """(W0, b0, Wh[5,256,256], bh[5,256], W8, b8, W14, b14) views of a flat arena-order vector"""
    a = torch.split(flat, ARENA_SIZES)
    return a[0].view(256, 39), a[1], a[2].view(5, 256, 256), a[3].view(5, 256), a[4].view(256, 295), a[5], a[6].view(1, 256), a[7]


class PackedWeights:
    """the flat parameter vector of one parameter state plus the fragment-order Packs of it that sweep_plan() asks for (the switches are read
    here, at construction), built once per sweep and shared by the sweep, its backward and the eikonal term of the same iteration.
    `packs` holds them by (arith, transposed); `wp` / `wpt` / `wpf` / `wpj` / `wpb` name them by role, None where a role has no pack of
    that kind -- a call site passes `p.t if p else None` and `p.planes if p else 0`.  `valid_for` compares the autograd version counters:
    any optimiser step invalidates it."""

    def __init__(self, params):
        self.key = tuple((p.data_ptr(), p._version) for p in params)
        self.flat = _FlatParams.apply(*params)                  # differentiable: both consumers' gradients meet here
        views = arena_views(self.flat.detach())
        self.plan = fwd, tan, bwd = sweep_plan(X3, H2, H2_JVP, H2_BWD)
        # one pack per distinct (arithmetic, form) of the plan; a split-plane pack carries everything its sweeps need (biases and head
        # included), so with X3 the f32 packs are not built
        self.packs = {k: _pack(views, *k) for k in dict.fromkeys([(fwd, False), (tan, False), (bwd, True)])}
        pick = lambda arith, tr, split: self.packs[(arith, tr)] if (arith != 'f32') == split else None
        self.wp, self.wpt = pick(fwd, False, False), pick(bwd, True, False)          # the exact-f32 pair (D3H_SDF_X3=0), else None
        # the split-plane packs by role (None with D3H_SDF_X3=0): forward-type sweeps, tangent sweep, data-backward sweeps
        self.wpf, self.wpj, self.wpb = pick(fwd, False, True), pick(tan, False, True), pick(bwd, True, True)
        self.w14 = views[6]

    def valid_for(self, params):
        return self.key == tuple((p.data_ptr(), p._version) for p in params)


def _packs(pack, params):
    if pack is not None and pack.valid_for(params):
        return pack
    return PackedWeights(params)


_PARAM_ORDER = ['0.weight', '0.bias', '2.weight', '2.bias', '4.weight', '4.bias', '6.weight', '6.bias', '8.weight', '8.bias',
                '10.weight', '10.bias', '12.weight', '12.bias', '14.weight', '14.bias']


# ---- the first half of the sweep's compact backward, ahead of time ---------------------------------------------------------------------------
# d3h_sdf_mlp_bwd_prepare (csrc/sdf_mlp_bwd.hip): once the caller knows which points CAN receive a gradient (hmsdf.tick_init: the vertices on
# sign-changing edges, marked by the regulariser's forward) the point list, the gather and the recompute of their activations do not have to
# wait for the gradient: they run on a stream of their own beside the loss / image-space backward instead of in the serial tail of the step
# (three launches, ~100 us at 9 k points).  D3H_SDF_PREPARE=0: everything inside the backward, as before.
PREPARE = os.environ.get('D3H_SDF_PREPARE', '1') != '0'
_PREP_STREAM = {}


def prepare_backward(sdf, edges32):
    """queue the first half of the compact backward of the sweep that produced `sdf` (the tensor sdf_query returned: the state lives on its
    autograd node and dies with the graph) on the prepare stream: mark the vertices on sign-changing edges (the edge visit of the SDF
    regulariser, csrc/image_ops.hip:sdf_reg_fwd_kernel, run for its marks only), list them, gather them, recompute their activations.
    A no-op when that sweep cannot use it (sharded, activations stored, already prepared) or `sdf` is not such a sweep's output."""
    node = sdf.grad_fn
    state = getattr(node, 'prep', None) if isinstance(node, _SDFMLPFn._backward_cls) else None
    if not PREPARE or state is None or state.get('done') or edges32 is None:
        return
    n, dev = state['n'], sdf.device
    if sdf.numel() != n:
        return
    x, deform, disp, rec = state['x'], state['deform'], state['disp'], state['rec']
    main = _cur_stream() if (sdf.is_cuda and not L.emulated()) else None
    side = None
    if main is not None:
        side = _PREP_STREAM.get(dev)
        if side is None:
            side = _PREP_STREAM[dev] = torch.cuda.Stream(device=dev)
        side.wait_stream(main)
    import contextlib
    sd = sdf.detach().reshape(-1)
    e32 = edges32.contiguous()
    with (L.use_stream(side) if side is not None else contextlib.nullcontext()):
        marks = torch.zeros(n, dtype=torch.float32, device=dev)
        sums = torch.empty(2, dtype=torch.float32, device=dev)
        act = torch.empty(L.query('sdf_mlp_act_floats', n), dtype=torch.float32, device=dev)
        tiles = torch.empty(L.query('sdf_mlp_bwd_scratch_ints', n), dtype=torch.int32, device=dev)
        L.call('sdf_reg_fwd', sd, e32, e32.shape[0], sums, marks)
        L.call('sdf_mlp_bwd_prepare', x, deform, disp, marks, n, tiles, rec.t, rec.planes, act)
        ev = None
        if side is not None:
            ev = torch.cuda.Event()
            ev.record()
            for t in (x, deform, sd, e32, rec.t):
                if t is not None:
                    t.record_stream(side)
    state.update(done=True, act=act, tiles=tiles, event=ev)


class _SDFMLPFn(torch.autograd.Function):
    """sdf = MLP(x + disp*deform); first-order autograd only (the eikonal term's double backward uses the second-order ops below).
    `flat` is PackedWeights.flat (the arena-order parameter vector); the gradient w.r.t. it is the arena the kernels wrote."""

    @staticmethod
    def forward(ctx, x, deform, disp, pk, flat, rows):
        need = any(t is not None and t.requires_grad for t in (x, deform, flat))
        # rows = (lo, hi): evaluate x[lo:hi] only (a rank's shard of the grid sweep, d3h.dist_ops).  The FULL tensors are the inputs of
        # the node, so the gradient of `deform` is written into its full-size buffer directly -- no slice node with its zero-filled copy
        xs, ds = (x, deform) if rows is None else (x[rows[0]:rows[1]], deform[rows[0]:rows[1]] if deform is not None else None)
        fwd = pk.wpf or pk.wp
        if need:
            ctx.rec = pk.wpf if RECOMPUTE else None          # the pack the backward recomputes the activations with (split-plane kernels only)
            if ctx.rec is not None:
                sdf = forward(xs, fwd, deform=ds, disp=disp)
                act = xs.new_empty(0)
            else:
                sdf, act, _ = forward(xs, fwd, deform=ds, disp=disp, save=True)
            ctx.wpt, ctx.w14, ctx.wpb = pk.wpt, pk.w14, pk.wpb
            ctx.save_for_backward(x, deform if deform is not None else x.new_empty(0), act)
            ctx.disp = float(disp)
            ctx.has_deform = deform is not None
            ctx.rows = rows
            ctx.deform_leaf = deform if (deform is not None and deform.is_leaf) else None
            ctx.prep = None
            if PREPARE and SPARSE_BACKWARD and ctx.rec is not None and rows is None:
                # (the whole-grid sweep of a single rank, without the activation save: its backward is the compact form and can be prepared --
                # prepare_backward finds this state on the output's grad_fn)
                xc = x.contiguous().float()
                ctx.prep = {'n': int(xc.shape[0]), 'x': xc, 'deform': deform.contiguous().float() if deform is not None else None,
                            'disp': float(disp), 'rec': ctx.rec}
        else:
            sdf = forward(xs, fwd, deform=ds, disp=disp)
        return sdf.unsqueeze(-1)

    @staticmethod
    def backward(ctx, gout):
        x, deform, act = ctx.saved_tensors
        if not ctx.has_deform:
            deform = None
        wpt, w7, wpb, rec = ctx.wpt, ctx.w14, ctx.wpb, ctx.rec
        ctx.wpt = ctx.w14 = ctx.wpb = ctx.rec = None
        rows, leaf = ctx.rows, ctx.deform_leaf
        ctx.deform_leaf = None
        x_full, deform_full = x, deform
        if rows is not None:
            x, deform = x[rows[0]:rows[1]], (deform[rows[0]:rows[1]] if deform is not None else None)
        n = x.shape[0]
        dev = x.device
        xc = x.contiguous().float()
        g = gout.reshape(-1).contiguous().float()
        prep, ctx.prep = ctx.prep, None
        prepared = bool(prep and prep.get('done'))
        tiles = None
        if prepared:                        # list, gathered points and recomputed activations are in place (prepare_backward): join its stream
            act, tiles = prep['act'], prep['tiles']
            if prep['event'] is not None:
                _cur_stream().wait_event(prep['event'])
                for t in (act, tiles):
                    t.record_stream(_cur_stream())
        elif rec is not None:                 # scratch for the recomputed activations (written at the visited tiles' own positions only)
            act = torch.empty(L.query('sdf_mlp_act_floats', n), dtype=torch.float32, device=dev)
        dz = torch.empty_like(act)
        dx = torch.empty(n, 3, dtype=torch.float32, device=dev)
        arena = L.zeros(ARENA_FLOATS, torch.float32, dev)          # (carved from the zero slab: no fill launch); returned as d(flat)
        dw0, db0, dwh, dbh, dw4, db4, dw7, db7 = arena_views(arena)
        dfm = deform.contiguous().float() if deform is not None else None
        # active-tile list: the backward only visits 16-point tiles with a non-zero upstream gradient (csrc/sdf_mlp_bwd.hip, section 0)
        # scratch of the sparse backward: the position-tile list, or -- compact form, when the activations are recomputed -- the gathered problem
        if tiles is None:
            tiles = torch.empty(L.query('sdf_mlp_bwd_scratch_ints', n), dtype=torch.int32, device=dev) if SPARSE_BACKWARD else None
        L.call('sdf_mlp_bwd', xc, dfm, ctx.disp, g, w7, wpt.t if wpt else None, wpb.t if wpb else None, act, dz, n, dx, dw0, db0, dwh, dbh, dw4,
               db4, dw7, db7, tiles, rec.t if rec else None, rec.planes if rec else 0, wpb.planes if wpb else 0, 1 if prepared else 0)
        d_deform = None
        if deform is not None and ctx.needs_input_grad[1]:
            # frame-parallel step: into the gradient's slice of the all-reduce arena (first contribution: written; later: added in place)
            d_deform = _GA.deliver(leaf if leaf is not None else deform_full, dx, ctx.disp, rows=rows)
        if rows is not None and ctx.needs_input_grad[0]:
            dxf = L.zeros_like(x_full, dtype=torch.float32)
            dxf[rows[0]:rows[1]] = dx
            dx = dxf
        return (dx if ctx.needs_input_grad[0] else None, d_deform, None, None, arena, None)


def sdf_query(x, params, deform=None, disp=0.0, pack=None, rows=None):
    """x[n,3] (+ disp*deform) -> sdf[n,1]; params: the 16 tensors of MLP.net in state_dict order; pack: a PackedWeights of them;
    rows = (lo, hi): only x[lo:hi] (-> sdf[hi-lo,1]), with the gradients landing in the full-size buffers"""
    pk = _packs(pack, params)
    return _SDFMLPFn.apply(x, deform, disp, pk, pk.flat, None if rows is None else (int(rows[0]), int(rows[1])))


class _SDFGradFn(torch.autograd.Function):
    """g = d(sdf)/d(x) at constant points x[n,3], differentiable w.r.t. the MLP parameters (the eikonal term of
    geometry/hmsdf.py:856-876: autograd.grad(..., create_graph=True) followed by a backward through the gradient graph).
    forward = fused forward with activation save + the first-order data backward with d(sdf) = 1; backward = the hand-derived
    second-order pass d3h_sdf_mlp_eik_bwd (tangent sweep, reverse sweep with the softplus'' injection, weight-gradient GEMMs)."""

    @staticmethod
    def forward(ctx, x, *params):
        sd = {k: p for k, p in zip(_PARAM_ORDER, params)}
        # its own arithmetic, not sweep_plan's: the forward on the forward-type split, grad_x / tangent / reverse on bf16 x 3 whenever X3 is on
        a = 'bf16x3' if X3 else 'f32'
        tan = pack_weights(sd, a, prefix='')
        bwd = pack_weights(sd, a, transposed=True, prefix='')
        xc = x.detach().contiguous().float()
        n = xc.shape[0]
        _, act, _ = forward(xc, pack_weights(sd, 'fp16x2', prefix='') if (X3 and H2) else tan, save=True)
        dz = torch.empty_like(act)
        g = torch.empty(n, 3, dtype=torch.float32, device=xc.device)
        w7 = sd['14.weight'].detach().contiguous().float()
        L.call('sdf_mlp_grad_x', xc, w7, None if X3 else bwd.t, bwd.t if X3 else None, bwd.planes, act, dz, n, g, 0)
        ctx.bufs = (xc, tan, bwd, act, dz)
        return g

    @staticmethod
    def backward(ctx, u):
        xc, tan, bwd, act, dz = ctx.bufs
        f32 = tan.planes == 0
        ctx.bufs = None
        n = xc.shape[0]
        dev = xc.device
        u = u.contiguous().float()
        tb, eb = torch.empty_like(act), torch.empty_like(act)
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        dw0, db0, dwh, dbh, dw4, db4, dw7 = z(256, 39), z(256), z(5, 256, 256), z(5, 256), z(256, 295), z(256), z(1, 256)
        L.call('sdf_mlp_eik_bwd', xc, u, tan.t if f32 else None, bwd.t if f32 else None, None if f32 else tan.t, tan.planes,
               None if f32 else bwd.t, bwd.planes, 0.0, act, dz, tb, eb, n, dw0, db0, dwh, dbh, dw4, db4, dw7, 0)
        grads = [dw0, db0, dwh[0], dbh[0], dwh[1], dbh[1], dwh[2], dbh[2], dw4, db4, dwh[3], dbh[3], dwh[4], dbh[4], dw7, None]
        return (None, *grads)


def sdf_gradient(x, params):
    """x[n,3] (treated as constants) -> d(sdf)/d(x) [n,3], differentiable w.r.t. `params` (the 16 tensors of MLP.net)."""
    return _SDFGradFn.apply(x, *params)


class _EikonalLossFn(torch.autograd.Function):
    """coeff * mean((|grad_x sdf(x)| - 1)^2) at constant points (hmsdf.py:856-876) with the parameter gradients computed EAGERLY in the
    forward: the term is linear in its upstream gradient, so backward only scales the stored gradients.  This moves the second-order
    sweeps (tangent, injected reverse, weight-gradient GEMMs: ~3 ms at 50 000 points) out of the GPU-saturated backward phase of the
    iteration into the forward phase, where they fill the host-bound gaps of the render / loss bookkeeping on the side stream."""

    @staticmethod
    def forward(ctx, x, coeff, pk, flat, begun, max_cus, ready):
        wp, wpt, wpj, wpb = pk.wp, pk.wpt, pk.wpj, pk.wpb
        if begun is not None:               # eikonal_begin() already queued the forward sweep on these points with these weights
            xc, act = begun
        else:
            xc = x.detach().contiguous().float()
            _, act, _ = forward(xc, pk.wpf or wp, save=True, max_cus=max_cus)
        n = xc.shape[0]
        dev = xc.device
        dz = torch.empty_like(act)
        g = torch.empty(n, 3, dtype=torch.float32, device=dev)
        w7 = pk.w14
        L.call('sdf_mlp_grad_x', xc, w7, wpt.t if wpt else None, wpb.t if wpb else None, wpb.planes if wpb else 0, act, dz, n, g, max_cus)
        need = flat.requires_grad
        s = torch.empty(1, dtype=torch.float32, device=dev)
        u = torch.empty_like(g) if need else None
        L.call('eikonal_loss', g, n, float(coeff) / max(n, 1), s, u)
        ret = s[0] * (float(coeff) / max(n, 1))
        # The loss value exists now; the eager second-order sweeps below only produce parameter gradients.  A caller that runs this op
        # on a side stream can wait for that event (`ready[0]`, handed back by eikonal_loss as `.d3h_ready`) instead of the whole stream: the sweeps (MFMA-bound, ~2.3 ms at 5 10^4 points) then
        # keep running under the HBM-bound loss / render backward of the main stream.  The backward of this node is replayed on the
        # stream it was recorded on, i.e. after them.
        if xc.is_cuda and not L.emulated():
            ready[0] = torch.cuda.Event()
            ready[0].record()
            # inputs that were allocated on another stream and are read by the sweeps below: without this the caching allocator may
            # hand their memory out again as soon as the caller drops them (e.g. the next SDF sweep of the iteration re-packs the
            # weights) while this stream is still reading -- the caller no longer waits for the whole stream
            cur = _cur_stream()
            for t in (xc, w7, *(p.t for p in pk.packs.values())):
                t.record_stream(cur)
        if need:
            tb, eb = torch.empty_like(act), torch.empty_like(act)
            # all parameter gradients live in ONE arena-order buffer (the output bias has none: its slot stays zero): backward scales it
            # with a single elementwise kernel and returns it as d(flat)
            arena = L.zeros(ARENA_FLOATS, torch.float32, dev)
            dw0, db0, dwh, dbh, dw4, db4, dw7, _ = arena_views(arena)
            L.call('sdf_mlp_eik_bwd', xc, u, wp.t if wp else None, wpt.t if wpt else None, wpj.t if wpj else None, wpj.planes if wpj else 0,
                   wpb.t if wpb else None, wpb.planes if wpb else 0, 2.0 * float(coeff) / max(n, 1), act, dz, tb, eb, n, dw0, db0, dwh, dbh, dw4,
                   db4, dw7, max_cus)
            ctx.arena = arena
        return ret

    @staticmethod
    def backward(ctx, gout):
        g = ctx.arena * gout
        ctx.arena = None
        return (None, None, None, g, None, None, None)


def eikonal_begin(x, params, pack=None, max_cus=0):
    """First kernel of eikonal_loss (the forward sweep with the activation save) on its own, so that a caller can queue it, issue other
    work while it runs (it is the longest single launch of the chain), and come back with eikonal_loss(..., begun=<this>)."""
    pk = _packs(pack, params)
    xc = x.detach().contiguous().float()
    _, act, _ = forward(xc, pk.wpf or pk.wp, save=True, max_cus=max_cus)
    return (xc, act)


def eikonal_loss(x, params, coeff, pack=None, begun=None, max_cus=0):
    """coeff * mean((|d sdf / d x| - 1)^2) over the points x[n,3] (constants); differentiable w.r.t. `params`.
    On the GPU the result carries `.d3h_ready`: an event recorded when the loss VALUE is complete (the eager second-order sweeps that
    follow it on the same stream only produce parameter gradients) -- one event per call, so two launches in flight cannot be confused."""
    pk = _packs(pack, params)
    ready = [None]          # _EikonalLossFn.forward records the event into this call's own holder
    out = _EikonalLossFn.apply(x, float(coeff), pk, pk.flat, begun, int(max_cus), ready)
    out.d3h_ready = ready[0]
    return out
