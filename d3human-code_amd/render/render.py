"""Deferred renderer with the reference's entry point `render_mesh(...)` (render/render.py:347-451) on the MI355X kernels.

What the reference does per call (render.py:213-345,42-205,375-449): clip transform -> first-layer rasterize -> six separate
dr.interpolate calls -> shade (two texture-MLP sweeps over every pixel incl. background, prepare_shading_normal, bsdf forced to
'kd') -> for each of 12 buffers a lerp against its background and its own dr.antialias pass.  Same outputs here, regrouped for
HBM: attributes sharing an index buffer are interpolated in ONE pass, the texture MLP runs only on covered pixels, and all
buffers are composited and antialiased in ONE pass over a channel-concatenated image (antialias is per-channel linear, so this is
exact).  `buffers=` (an extension; default = all, as the reference) lets a caller name the outputs it will read.

FLAGS.lit_shading (an extension, off by default) makes the branch of render.py:121-163 real, which the reference's hard-wired `bsdf = 'kd'`
(render.py:120) leaves dead: the environment light sampled with shadow rays against the posed mesh (render.optixutils), the denoiser, the
PBR / diffuse / white combine -- `shade_lit`.  Without the flag nothing of it is touched: `lgt`, `optix_ctx`, `bsdf`, `denoiser` and
`shadow_scale` are accepted and ignored, as before.

2-D materials (the exported mesh of d3h.export.textured_mesh, or any material with 'kd' / 'ks' / 'normal' as Texture2D and no 'kd_ks'): the texel
coordinate is interpolated from mesh.v_tex by mesh.t_tex_idx and the maps are read with material['filter_mode'] (default 'linear-mipmap-linear', the
reference's Texture2D.sample; 'linear' / 'nearest' are level-0 lookups, boundary 'wrap', what the triangle-pair atlas is baked for).  Normals and
tangents go by t_nrm_idx / t_tng_idx.  With use_uv, finetune_normal, a 'normal' map (and no true 'no_perturbed_nrm') and mesh.v_tng the normal map
perturbs the shading normal in the interpolated tangent frame and 'perturbed_nrm' / 'perturbed_nrm_grad' (render.py:106-109,202-204) join the
outputs.  'kd_grad' / 'ks_grad' are SCREEN-SPACE there, built like normal_grad: |tap(kd, jitter) - kd| * grad_weight (ks times (0, 1, 1)), tap the
bilinear / clamp lookup of the image at the jittered pixel grid -- the reference has no 2-D rule (its jitter is a 3-D position offset into the MLP),
and a jitter in uv space would leave the triangle's cell of the atlas.  The lookups are one fused pass (d3h.texmat) when the mode is 'linear', the
raster and v_tex need no gradient and shading runs at the visibility resolution; else interpolate + texture, which gives the same values.
D3H_TEXMAT_FUSED=0 / 1 forces the composed / fused route where both apply (default: profiles/texmat_probe.md).

Layers and transparency (FLAGS.layers, FLAGS.transparency of the reference: train.py:449,1578,233; render.py:91-92,179-204,375-382).  The contract:
let L = num_layers >= 1, peeled front to back as rast_0 .. rast_{L-1}.  Layer l is shaded exactly as the single layer is: its own G-buffer pass, its
own material lookup and its own shade(); with spp > 1 or msaa its own scaling.  Its opacity A_l [B,H,W,1] is the fourth channel of the looked-up kd
(which the Texture2D has clamped); everything that read kd reads kd[..., :3].  A material without that channel, and any MLP material, has A_l = 1.
For every output buffer k with n_k value channels
    acc = background_k               # n_k + 1 channels: 'shaded' = [background rgb, 0]; 'depth' = 20 in all n_k + 1 channels; others 0
    for l = L-1 .. 0:                # back to front
        w   = (rast_l[..., 3] > 0) * A_l
        acc = lerp(acc, [value_{k,l}, 1], w)
        acc = antialias(acc, rast_l, v_pos_clip, tri)
    out_k = avg_pool(acc, spp) if spp > 1 else acc
'msdf_image' keeps its rule: one channel, w = coverage_l * msdf_l, end value 1 (A_l does not enter).  'visible_triangles', '_seen_faces' and '_rast'
come from layer 0.  The lerp is torch.lerp's two-branch form, exact at w = 0 (returns acc) and w = 1 (returns the source): a layer that covers
nothing is the identity, bit for bit.  Gates: the opacity is read only when getattr(FLAGS, 'transparency', False) is true -- without the flag a
4-channel kd raises NotImplementedError, as before; every call with num_layers == 1 and no opacity channel runs the single-layer code unchanged;
num_layers > 1 needs no flag (opaque layers are valid); num_layers < 1 raises ValueError; FLAGS.lit_shading with num_layers > 1 raises
NotImplementedError (shadow rays per layer are not built).  One blend step is d3h.imgops.layer_composite_antialias (one kernel each way, under
torch.no_grad() the forward one only) or, with D3H_LAYER_FUSED=0, torch.lerp + dr.antialias on the channel-concatenated image (default:
profiles/layers_probe.md).

`mesh.v_pos` may be [P,3] (the reference) or [B,P,3] (one posed mesh per frame of the batch: the build's N-frame extension,
SURVEY F5).  spp > 1 is not part of the hot path (FLAGS.spp = 1) and raises.
"""
import os

import torch
from d3h.devconst import const as _const
import nvdiffrast.torch as dr

from . import util
from . import renderutils as ru
from . import optixutils as ou
from d3h import imgops as _I
from d3h import raster as _R
from d3h import texmat as _TM
from .texture import Texture2D as _Texture2D

ALL_BUFFERS = ('shaded', 'z_grad', 'normal', 'geometric_normal', 'kd', 'ks', 'kd_grad', 'ks_grad', 'normal_grad', 'depth', 'invdepth')
LIT_BUFFERS = ('diffuse_light', 'specular_light')          # render.py:197-200: present only when the lit branch ran
LIT_BSDFS = ('pbr', 'diffuse', 'white')
BSDFS = ('kd', 'ks', 'normal', 'tangent') + LIT_BSDFS
PERTURBED_BUFFERS = ('perturbed_nrm', 'perturbed_nrm_grad')   # render.py:202-204: present only when a normal map perturbs the shading normal
TEXMAT_FUSED_DEFAULT = True                                # profiles/texmat_probe.md
LAYER_FUSED_DEFAULT = True                                 # profiles/layers_probe.md
rnd_seed = 0                                               # render.py:128-132: the sampler's seed, one step per lit shade


class LazyVisibleTriangles(torch.Tensor):
    """The sorted ids of the triangles that own at least one pixel (render.py:404-407) as a DEFERRED tensor: the compaction
    `nonzero(bitmap)` has a data-dependent size, i.e. a host synchronisation in the middle of the iteration.  Internal to tick_seq, which
    hands `visible_triangles` back to a loop that reads it once, after the last iteration (train.py:1515); `render_mesh` itself returns a
    plain tensor whenever `visible_triangles` is asked for.
    A real torch.Tensor subclass: isinstance / torch.is_tensor hold, and EVERY use -- a method or property, an argument of a torch
    function at any nesting depth (`torch.cat([v, t])`), an index (`faces[v]`), copy / deepcopy / pickle -- goes through
    __torch_function__ (or __reduce_ex__), which swaps in the materialised int64 tensor first."""

    @staticmethod
    def __new__(cls, seen):
        return torch.Tensor._make_subclass(cls, torch.empty(0, dtype=torch.long, device=seen.device))

    def __init__(self, seen):
        self._d3h_seen, self._d3h_value = seen, None

    def materialize(self):
        if self._d3h_value is None:
            with torch._C.DisableTorchFunctionSubclass():
                self._d3h_value = torch.nonzero(self._d3h_seen).reshape(-1)
        return self._d3h_value

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        from torch.utils._pytree import tree_map
        un = lambda a: a.materialize() if isinstance(a, LazyVisibleTriangles) else a
        with torch._C.DisableTorchFunctionSubclass():
            return func(*tree_map(un, tuple(args)), **tree_map(un, dict(kwargs or {})))

    def __reduce_ex__(self, proto):
        return self.materialize().__reduce_ex__(proto)

    def __repr__(self):
        return 'LazyVisibleTriangles(%s)' % ('<deferred>' if self._d3h_value is None else repr(self._d3h_value))


def interpolate(attr, rast, attr_idx, rast_db=None):
    return dr.interpolate(attr.contiguous(), rast, attr_idx, rast_db=rast_db, diff_attrs=None if rast_db is None else 'all')


def _batched(v):
    return v if v.dim() == 3 else v[None]


def shade_lit(FLAGS, cover, ro, gb_pos, gb_normal, zdz, view_pos, kd, ks, lgt, optix_ctx, bsdf, denoiser, shadow_scale=1.0):
    """render.py:121-163: the lit colour of bsdf 'pbr' / 'diffuse' / 'white' -> {'shaded', 'diffuse_light', 'specular_light'}, each [B,H,W,3].

    cover [B,H,W] or [B,H,W,1] (> 0: shade this pixel); ro = gb_pos + 0.001 n, the shadow rays' origin; gb_normal the prepared shading normal;
    zdz [B,H,W,2] = (z, |dz|), the denoiser's depth guide (read only when a denoiser is given); view_pos broadcastable to gb_pos.  `optix_ctx` is
    one OptiXContext for the whole batch or a list of B, one per frame: then frame b is traced against context b alone (B launches on [1,H,W]
    slices, all with the call's seed).  The seed is the module's `rnd_seed`, which advances by one per call; FLAGS.decorrelated passes None (a fresh
    seed each way).  With FLAGS.denoiser_demodulate the two light images are denoised (under one set of guides: one launch each way when the
    denoiser has `forward_many`) before the combine, else the combined colour is.  The reference's debug image writes are not reproduced."""
    global rnd_seed
    from . import light
    if bsdf not in LIT_BSDFS:
        raise RuntimeError(f"shade_lit: bsdf must be one of {LIT_BSDFS}, got {bsdf!r}")
    if not isinstance(lgt, light.EnvironmentLight) or optix_ctx is None:
        raise RuntimeError('shade_lit: lit shading needs an EnvironmentLight and an OptiXContext')
    if bsdf == 'white':
        kd = torch.ones_like(kd)
    seed = None if getattr(FLAGS, 'decorrelated', False) else rnd_seed
    rnd_seed += 1
    view = view_pos.expand(gb_pos.shape)
    tables = (lgt.base, lgt._pdf, lgt.rows[:, 0], lgt.cols)
    kw = dict(BSDF=bsdf, n_samples_x=getattr(FLAGS, 'n_samples', 4), rnd_seed=seed, shadow_scale=shadow_scale)
    ctxs = list(optix_ctx) if isinstance(optix_ctx, (list, tuple)) else [optix_ctx]
    if len(ctxs) == 1:
        diffuse, specular = ou.optix_env_shade(ctxs[0], cover, ro, gb_pos, gb_normal, view, kd, ks, *tables, **kw)
    else:
        if len(ctxs) != gb_pos.shape[0]:
            raise RuntimeError(f'shade_lit: {len(ctxs)} contexts for {gb_pos.shape[0]} frames')
        f = lambda t, b: t[b:b + 1]
        per = [ou.optix_env_shade(c, f(cover, b), f(ro, b), f(gb_pos, b), f(gb_normal, b), f(view, b), f(kd, b), f(ks, b), *tables, **kw)
               for b, c in enumerate(ctxs)]
        diffuse, specular = torch.cat([d for d, _ in per], dim=0), torch.cat([s_ for _, s_ in per], dim=0)
    demodulate = getattr(FLAGS, 'denoiser_demodulate', True)
    if denoiser is not None and demodulate:
        if hasattr(denoiser, 'forward_many'):
            diffuse, specular = denoiser.forward_many([diffuse, specular], gb_normal, zdz)
        else:
            diffuse = denoiser.forward(torch.cat((diffuse, gb_normal, zdz), dim=-1))
            specular = denoiser.forward(torch.cat((specular, gb_normal, zdz), dim=-1))
    if bsdf == 'pbr':
        shaded = diffuse * (kd * (1.0 - ks[..., 2:3])) + specular          # kd (1 - metalness)
    else:
        shaded = diffuse * kd
    if denoiser is not None and not demodulate:
        shaded = denoiser.forward(torch.cat((shaded, gb_normal, zdz), dim=-1))
    return {'shaded': shaded, 'diffuse_light': diffuse, 'specular_light': specular}


def _frame_contexts(optix_ctx, B):
    """The contexts a batch of B frames is traced against.  optix_build_bvh recorded the posed mesh; with one posed mesh per frame (vertices
    [B,P,3]) every frame gets a context of its own over ITS vertices -- built lazily, like any other -- where OptiXContext.build() would flatten
    the batch into one soup and test every frame against all of them at frame 0's indices.  The B contexts are kept on `optix_ctx.frames` beside the
    record they were made from: a second render_mesh against the same record (the watertight twin of geometry.hmsdf._render) reuses their BVHs, as a
    single context reuses its own; the next optix_build_bvh replaces the record and with it the contexts."""
    pend = None if optix_ctx is None else optix_ctx.pending
    if B == 1 or pend is None or pend[0].dim() != 3 or pend[0].shape[0] != B:
        return optix_ctx
    if optix_ctx.frames is not None and optix_ctx.frames[0] is pend:
        return optix_ctx.frames[1]
    verts, tris = pend
    ctxs = []
    for b in range(B):
        c = ou.OptiXContext()
        ou.optix_build_bvh(c, verts[b], tris if tris.dim() == 2 else tris[b], rebuild=1)
        ctxs.append(c)
    optix_ctx.frames = (pend, ctxs)
    return ctxs


def is_texture_material(material):
    """a 2-D material: no 'kd_ks', and 'kd' and 'ks' as Texture2D"""
    return isinstance(material, dict) and ('kd_ks' not in material) and isinstance(material.get('kd'), _Texture2D) and isinstance(material.get('ks'), _Texture2D)


def _texmat_fused():
    env = os.environ.get('D3H_TEXMAT_FUSED')
    return TEXMAT_FUSED_DEFAULT if env is None else env != '0'


def _layer_fused():
    env = os.environ.get('D3H_LAYER_FUSED')
    return LAYER_FUSED_DEFAULT if env is None else env != '0'


def _material_lookups(mesh, rast, db, names, same_res, mask):
    """{name: [B,H,W,C]} of the material's maps `names` at the pixels' texel coordinates (module docstring), zero at uncovered pixels on either
    route (the composed lookups read texel (0, 0) there: masked, so that the screen-space taps next to the silhouette see the same image)"""
    material = mesh.material
    mode = material.get('filter_mode', 'linear-mipmap-linear')
    mip = mode.startswith('linear-mipmap')
    texs = [material[k] for k in names]
    if not names:
        return {}
    level0 = [t.getMips()[0] for t in texs]
    fused_ok = (mode == 'linear' and same_res and not mip and all(l.shape[0] == 1 and l.shape[-1] <= _TM.MAX_CHANNELS for l in level0)
                and not (torch.is_grad_enabled() and (rast.requires_grad or mesh.v_tex.requires_grad)))
    if fused_ok and _texmat_fused():
        return dict(zip(names, _TM.lookup(rast.detach(), mesh.v_tex.detach(), mesh.t_tex_idx.int(), level0, boundary='wrap')))
    if mip:
        texc, texc_deriv = interpolate(mesh.v_tex[None, ...], rast, mesh.t_tex_idx.int(), rast_db=db)
        return {k: t.sample(texc, texc_deriv, filter_mode=mode) * mask for k, t in zip(names, texs)}
    texc, _ = interpolate(mesh.v_tex[None, ...], rast, mesh.t_tex_idx.int())
    return {k: dr.texture(l, texc, filter_mode=mode, boundary_mode='wrap') * mask for k, l in zip(names, level0)}


def shade(FLAGS, idx, rast, aux, gb_pos, gb_pos_original, gb_geometric_normal, gb_normal, gb_tangent, view_pos, material, want,
          finetune_normal=True, mask=None, rng_draws=None, live=None, skip_uncovered=True, lit=None, tex2d=None):
    """render.py:42-205 with perturbed_nrm None.  `lit` None: the branch the reference's hard-wired bsdf = 'kd' leaves live, exactly; else
    (bsdf, lgt, contexts, denoiser, shadow_scale) of FLAGS.lit_shading: 'shaded' follows the bsdf (render.py:121-176).  `aux` = (z_grad values, depth, invdepth) from
    the fused forward-only pass (d3h.raster.aux_buffers; entries None where not produced); `live`: the buffers that need a gradient
    (None = all) -- the producers of the others run under torch.no_grad().
    `tex2d` (a 2-D material, module docstring): {'lookup': names -> {name: image}, 'perturb': bool}; then 'kd_ks' is not read, `pos_noise` neither drawn
    nor read, and kd_grad / ks_grad are the screen-space rule."""
    B, H, W = rast.shape[:3]
    dev = rast.device
    grad_on = torch.is_grad_enabled()
    on = lambda *ks: torch.set_grad_enabled(grad_on and (live is None or any(k in live for k in ks)))
    if mask is None:
        mask = (rast[..., -1:] > 0).float()                                       # render.py:66
    need_jitter = bool(want & {'normal_grad', 'kd_grad', 'ks_grad', 'perturbed_nrm_grad'})
    # RNG call order follows the reference (offset, then the position jitter) so a seeded CPU run reproduces it
    if rng_draws is not None:            # pre-drawn jitter (tests: the same draws on every device)
        offset, pos_noise = rng_draws['offset'].to(dev), (rng_draws['pos_noise'].to(dev) if tex2d is None else None)
    else:
        offset = torch.normal(mean=0, std=0.005, size=(B, H, W, 2), device=dev) if need_jitter else None
        pos_noise = torch.normal(mean=0, std=0.01, size=gb_pos_original.shape, device=dev) if need_jitter and tex2d is None else None

    kd_ks = material['kd_ks'] if tex2d is None else None
    perturbed_nrm = None
    # the texture MLP skips uncovered pixels (their value never reaches an output: alpha = 0) -- except under supersampling, where a
    # covered sub-pixel can inherit the value of an uncovered shading pixel (render.py:241-245,334-336): then every pixel is evaluated
    tex_mask = mask if skip_uncovered else None
    out = {}
    tex_users = ('shaded', 'kd', 'ks', 'kd_grad', 'ks_grad')
    is_live = lambda k: live is None or k in live
    # kd and the three smoothness buffers in ONE pass each way (d3h.imgops.material_grads) when every one of them that is wanted takes a
    # gradient (a tick of the split / seq stage) or none does; in the mixed case (the 'all' mode of a tick) the dead ones stay separate
    # torch ops under no_grad so that the backward does not pay for them
    smooth = want & {'kd_grad', 'ks_grad', 'normal_grad'}
    fused = tex2d is None and ({'kd_grad', 'ks_grad'} <= want) and (not grad_on or all(is_live(k) for k in smooth | (want & {'shaded', 'kd'})))
    # ... and when NONE of the smoothness buffers is live (tick_init in its 'all' mode) they come out of the same pass under no_grad, kd staying
    # the plain slice that carries the gradient
    fused_dead = tex2d is None and (not fused) and ({'kd_grad', 'ks_grad'} <= want) and grad_on and not any(is_live(k) for k in smooth)
    if tex2d is not None:
        # ---- 2-D material: the maps at the texel coordinate; the smoothness terms in screen space (module docstring)
        names = [k for k, users in (('kd', {'shaded', 'kd', 'kd_grad'}), ('ks', {'ks', 'ks_grad'})) if want & users or (k == 'kd' and tex2d.get('alpha'))]
        nrm_users = {'normal', 'perturbed_nrm', 'perturbed_nrm_grad'}
        if tex2d['perturb'] and want & nrm_users:
            names.append('normal')
        # (the opacity weighs EVERY buffer of the layer: with it the lookup is differentiable whenever any buffer is live)
        with (torch.set_grad_enabled(grad_on and (live is None or bool(live))) if tex2d.get('alpha') else on(*tex_users, *nrm_users)):
            vals = tex2d['lookup'](names)
        kd, ks, perturbed_nrm = vals.get('kd'), vals.get('ks'), vals.get('normal')
        if tex2d.get('alpha'):                       # FLAGS.transparency (render.py:91-92): kd = (colour, the layer's opacity)
            out['_alpha'], kd = kd[..., 3:4], kd[..., 0:3]
        ks = ks[..., 0:3] if ks is not None else None
        if want & {'kd_grad', 'ks_grad', 'perturbed_nrm_grad'}:
            jitter = (util.pixel_grid(W, H, device=dev)[None, ...] + offset).contiguous()
            tap = lambda img: dr.texture(img.contiguous(), jitter, filter_mode='linear', boundary_mode='clamp')
            grad_weight = mask * tap(mask)                                     # render.py:72-73
            if 'kd_grad' in want:
                with on('kd_grad'):
                    out['kd_grad'] = torch.abs(tap(kd) - kd) * grad_weight
            if 'ks_grad' in want:
                with on('ks_grad'):
                    out['ks_grad'] = torch.abs(tap(ks) - ks) * grad_weight * _const((0.0, 1.0, 1.0), dev)
            if 'perturbed_nrm_grad' in want and perturbed_nrm is not None:
                with on('perturbed_nrm_grad'):                                  # render.py:106-109
                    both = util.safe_normalize(util.safe_normalize(tap(perturbed_nrm)) + util.safe_normalize(perturbed_nrm))
                    out['perturbed_nrm_grad'] = (1.0 - both[..., 2:3]).repeat(1, 1, 1, 3) * grad_weight
        if 'perturbed_nrm' in want and perturbed_nrm is not None:
            out['perturbed_nrm'] = perturbed_nrm
    elif want & set(tex_users):
        with on(*tex_users):
            all_tex = kd_ks.sample(gb_pos_original, idx, mask=tex_mask)
        kd = _I.first_channels(all_tex, 3)           # (the channels the shaded colour carries: a one-pass gradient instead of the slice node's fill + copy)
        ks = all_tex[..., 3:6]
    # Every buffer of the layer is [values, alpha = 1] in the reference (torch.cat((..., alpha), dim=-1) throughout render.py:99-199);
    # the alpha channel is appended by the composite pass, so only the value channels are collected here.
    if fused:
        all_tex_jitter = kd_ks.sample(gb_pos_original + pos_noise, idx, mask=tex_mask)
        nrm_in = (None, None, None, None)
        if 'normal_grad' in want:
            jitter = (util.pixel_grid(W, H, device=dev)[None, ...] + offset).contiguous()
            mask_tap = dr.texture(mask.contiguous(), jitter, filter_mode='linear', boundary_mode='clamp')
            nrm_jitter = dr.texture(gb_normal.contiguous(), jitter, filter_mode='linear', boundary_mode='clamp')
            nrm_in = (gb_normal, nrm_jitter, mask, mask_tap)
        kd, out['kd_grad'], out['ks_grad'], ng = _I.material_grads(all_tex, all_tex_jitter, *nrm_in)
        if ng is not None:
            out['normal_grad'] = ng
    elif fused_dead:
        with torch.no_grad():
            all_tex_jitter = kd_ks.sample(gb_pos_original + pos_noise, idx, mask=tex_mask)
            nrm_in = (None, None, None, None)
            if 'normal_grad' in want:
                jitter = (util.pixel_grid(W, H, device=dev)[None, ...] + offset).contiguous()
                mask_tap = dr.texture(mask.contiguous(), jitter, filter_mode='linear', boundary_mode='clamp')
                nrm_jitter = dr.texture(gb_normal.contiguous(), jitter, filter_mode='linear', boundary_mode='clamp')
                nrm_in = (gb_normal, nrm_jitter, mask, mask_tap)
            _, out['kd_grad'], out['ks_grad'], ng = _I.material_grads(all_tex, all_tex_jitter, *nrm_in, want_kd=False)
            if ng is not None:
                out['normal_grad'] = ng
    elif tex2d is None and want & {'kd_grad', 'ks_grad'}:
        with on('kd_grad', 'ks_grad'):
            all_tex_jitter = kd_ks.sample(gb_pos_original + pos_noise, idx, mask=tex_mask)
            out['kd_grad'] = torch.abs(all_tex_jitter[..., 0:3] - kd)
            ks_w = _const((0.0, 1.0, 1.0), dev)
            out['ks_grad'] = torch.abs(all_tex_jitter[..., 3:6] - ks) * ks_w
    if 'normal_grad' in want and not fused and not fused_dead:
        with on('normal_grad'):
            jitter = (util.pixel_grid(W, H, device=dev)[None, ...] + offset).contiguous()
            mask_tap = dr.texture(mask.contiguous(), jitter, filter_mode='linear', boundary_mode='clamp')
            nrm_jitter = dr.texture(gb_normal.contiguous(), jitter, filter_mode='linear', boundary_mode='clamp')
            out['normal_grad'] = torch.abs(nrm_jitter - gb_normal) * (mask * mask_tap)
    if 'normal' in want:
        with on('normal'):
            out['normal'] = ru.prepare_shading_normal(gb_pos, view_pos, perturbed_nrm, gb_normal, gb_tangent, gb_geometric_normal, two_sided_shading=True,
                                                      opengl=True)
    if 'shaded' in want and lit is not None:
        bsdf, lgt, ctxs, denoiser, shadow_scale = lit
        with on('shaded'):
            if bsdf in LIT_BSDFS:
                n = out['normal']
                out.update(shade_lit(FLAGS, mask, gb_pos + n * 0.001, gb_pos, n, aux[0][..., 0:2] if denoiser is not None else None, view_pos, kd, ks,
                                     lgt, ctxs, bsdf, denoiser, shadow_scale))
            elif bsdf == 'normal':
                out['shaded'] = (out['normal'] + 1.0) * 0.5        # render.py:165-174
            elif bsdf == 'tangent':
                out['shaded'] = (gb_tangent + 1.0) * 0.5
            else:
                out['shaded'] = kd if bsdf == 'kd' else ks
    elif 'shaded' in want:
        out['shaded'] = kd                                         # bsdf = 'kd' (render.py:120,169-170)
        if not fused and tex2d is None:
            out['_shaded_of'] = all_tex                            # kd IS all_tex[..., :3]: the fused composite takes the wide tensor (compose)
    if 'kd' in want:
        out['kd'] = kd
    if 'ks' in want:
        out['ks'] = ks
    z_aux, depth_aux, inv_aux = aux
    if 'z_grad' in want:
        out['z_grad'] = z_aux                                      # (z, |dz|, 0): render.py:291-299,105
    if 'geometric_normal' in want:
        out['geometric_normal'] = gb_geometric_normal
    if 'depth' in want:
        if depth_aux is not None:
            out['depth'] = depth_aux
        else:
            out['depth'] = (gb_pos - view_pos).pow(2).sum(dim=-1, keepdim=True).sqrt()
    if 'invdepth' in want:
        if inv_aux is not None:
            out['invdepth'] = inv_aux
        else:
            out['invdepth'] = 1.0 / ((gb_pos - view_pos).pow(2) + 1e-8).sum(dim=-1, keepdim=True).sqrt()
    return out


def render_mesh(FLAGS, idx, ctx, mesh, mesh_original, mtx_in, view_pos, lgt, resolution, spp=1, num_layers=1, msaa=False, background=None,
                optix_ctx=None, bsdf=None, denoiser=None, shadow_scale=1.0, use_uv=True, finetune_normal=True, extra_dict=None, xfm_lgt=None,
                shade_data=False, buffers=None, _keep_rast=False, _rng_draws=None, _grad_buffers=None):
    """`_rng_draws` (extension, tests): {'noise' [B,H,W,3], 'offset' [B,H,W,2], 'pos_noise' [B,H,W,3]} -- the three random tensors of a
    call, which the reference draws from the global generator in this order (render.py:285, :68, :84); None = draw them here.
    `_grad_buffers` (extension, tick_*): the buffers whose gradient somebody will ask for; the others are produced under
    torch.no_grad() and composited / antialiased in a pass of their own, so the backward of a tick that renders all 12 buffers costs
    what the backward of the three to seven it reads costs.  None = every buffer is differentiable, as in the reference."""
    num_layers = int(num_layers)
    if num_layers < 1:
        raise ValueError(f'render_mesh: num_layers must be at least 1, got {num_layers}')
    if num_layers > 1 and getattr(FLAGS, 'lit_shading', False):
        raise NotImplementedError('render_mesh: FLAGS.lit_shading with num_layers > 1 (shadow rays per peeled layer) is not built')
    transparency = bool(getattr(FLAGS, 'transparency', False))
    spp = int(spp)
    H, W = int(resolution[0]), int(resolution[1])
    Hf, Wf = H * spp, W * spp                     # visibility resolution (render.py:239); == (H, W) in every configuration of train.py (spp = 1)
    want = set(ALL_BUFFERS) if buffers is None else set(buffers)
    want.discard('msdf_image')
    _keep_rast = _keep_rast or (buffers is not None and '_rast' in buffers)
    for k in ('_rast', 'visible_triangles', '_seen_faces'):
        want.discard(k)
    if extra_dict is not None and extra_dict.get('msdf') is not None and (buffers is None or 'msdf_image' in buffers):
        want.add('msdf_image')
    grad_on = torch.is_grad_enabled()
    # ---- a 2-D material (module docstring): what it needs of the mesh, and whether its normal map perturbs the shading normal
    tex2d = is_texture_material(mesh.material)
    perturb = False
    if tex2d:
        if mesh.v_tex is None or mesh.t_tex_idx is None:
            raise ValueError("render_mesh: a material with 'kd' / 'ks' texture maps needs mesh.v_tex and mesh.t_tex_idx")
        if mesh.material['kd'].getChannels() == 4 and not transparency:
            raise NotImplementedError('render_mesh: a 4-channel kd (transparency, FLAGS.transparency of the reference) is not built')
        perturb = bool(use_uv and finetune_normal and isinstance(mesh.material.get('normal'), _Texture2D)
                       and not mesh.material.get('no_perturbed_nrm', False) and mesh.v_tng is not None)
        if perturb and buffers is None:
            want |= set(PERTURBED_BUFFERS)
    if not perturb:
        want -= set(PERTURBED_BUFFERS)
    has_alpha = bool(tex2d and transparency and mesh.material['kd'].getChannels() == 4)
    live = None if (_grad_buffers is None or not grad_on) else (want & set(_grad_buffers))
    # ---- FLAGS.lit_shading: the colour follows the bsdf (render.py:117-176).  `want` grows by what the lit colour is made of, so that a caller that
    # reads only 'shaded' still gets positions, shading normal, kd / ks and the denoiser's (z, |dz|); `want_out` / `live_out` stay what was asked for
    want_out, live_out, lit = set(want), live, None
    if getattr(FLAGS, 'lit_shading', False):
        assert bsdf is not None or 'bsdf' in mesh.material, 'Material must specify a BSDF type'
        bsdf = mesh.material['bsdf'] if bsdf is None else bsdf
        if bsdf not in BSDFS:
            raise RuntimeError(f"render_mesh: invalid BSDF '{bsdf}'")
        if buffers is None and bsdf in LIT_BSDFS:
            want_out |= set(LIT_BUFFERS)
        if 'shaded' in want:
            deps = {'pbr': {'normal', 'kd', 'ks'}, 'diffuse': {'normal', 'kd', 'ks'}, 'white': {'normal', 'kd', 'ks'}, 'normal': {'normal'},
                    'tangent': {'normal'}, 'kd': {'kd'}, 'ks': {'ks'}}[bsdf]
            if bsdf in LIT_BSDFS and denoiser is not None:
                deps = deps | {'z_grad'}
            want = want | deps
            if live is not None and 'shaded' in live:
                live = live | (deps - {'z_grad'})
            lit = (bsdf, lgt, None, denoiser, shadow_scale)
    view_pos = view_pos[:, None, None, :] if view_pos.dim() == 2 else view_pos
    tri = mesh.t_pos_idx32
    dev = mesh.v_pos.device

    v_pos = _batched(mesh.v_pos)
    v_pos_clip = ru.xfm_points(v_pos, mtx_in)                                      # render.py:396
    B = v_pos_clip.shape[0]
    # the pixel derivatives of the barycentrics are read by the z-gradient pass only (render.py:291-299): not written when no buffer wants it
    no_grad_of = lambda k: k in want and (not grad_on or (live is not None and k not in live))
    need_aux = 'z_grad' in want or no_grad_of('depth') or no_grad_of('invdepth')
    # grad_db=False: db feeds the no-grad z-gradient pass only, so its (spp > 1) rescale below records no autograd node
    with dr.DepthPeeler(ctx, v_pos_clip, tri, [Hf, Wf], grad_db=False) as peeler:
        mip_uv = tex2d and mesh.material.get('filter_mode', 'linear-mipmap-linear').startswith('linear-mipmap')     # the texel footprint
        peeled = [peeler.rasterize_next_layer(want_db='z_grad' in want or mip_uv) for _ in range(num_layers)]      # front to back
    rast_full = peeled[0][0]
    if spp > 1 and not msaa:
        H, W = Hf, Wf                             # no msaa: everything at the visibility resolution, averaged at the end

    F = tri.shape[0]
    # ---- G-buffer: one interpolation pass for everything indexed by t_pos_idx (render.py:257-259,283,328) ------------------
    # one pass over the raster (d3h.raster.gbuffer): each attribute lands in its own contiguous image, attributes no requested buffer
    # reads are neither packed nor produced (nor, for lazily built normals, computed), the face normal (render.py:261-267: an
    # (f, f, f)-indexed interpolation) is a gather by triangle id and the coverage mask of shade() (render.py:66) comes out of the
    # same read
    has_msdf = 'msdf_image' in want
    need_pos, need_nrm = bool(want & {'normal', 'depth', 'invdepth'}), bool(want & {'normal', 'normal_grad'})
    srcs = []
    # (a 2-D material reads no canonical position; its normals go by t_nrm_idx, in a pass of their own when that is another index buffer)
    own_nrm_idx = tex2d and mesh.t_nrm_idx is not None and mesh.t_nrm_idx is not mesh.t_pos_idx
    if need_pos:
        srcs.append(('pos', v_pos))
    if not tex2d:
        srcs.append(('orig', _batched(mesh_original.v_pos)))
    if need_nrm and not own_nrm_idx:
        srcs.append(('nrm', _batched(mesh.v_nrm)))
    if has_msdf:
        m = extra_dict['msdf']
        assert m.dim() == 1 or (m.dim() == 2 and m.size(1) == 1)
        srcs.append(('msdf', m.reshape(1, -1, 1)))
    if not srcs:
        srcs.append(('pos', v_pos))               # (the pass also makes the coverage mask and the face normal)
    nb_attr = max(t.shape[0] for _, t in srcs)
    packed = torch.cat([t.expand(nb_attr, -1, -1) for _, t in srcs], dim=-1) if len(srcs) > 1 else srcs[0][1]
    fn = _I.face_normals(v_pos, tri) if want & {'geometric_normal', 'normal'} else None      # [B,F,3], one launch
    if lit is not None and lit[0] in LIT_BSDFS:
        lit = (lit[0], lit[1], _frame_contexts(optix_ctx, B), lit[3], lit[4])

    def shade_layer(rast_full, db_full):
        """one peeled layer, shaded exactly as the single layer of the reference: -> ({buffer: values at the visibility resolution}, the texture MLP's
        whole output when 'shaded' is its channel prefix, the layer's opacity [B,Hf,Wf,1] or None = 1)"""
        rast, db = rast_full, db_full
        if spp > 1 and msaa:                          # shade at the framebuffer resolution (render.py:241-245): nearest sample of the raster
            rast = util.scale_img_nhwc(rast_full, [H, W], mag='nearest', min='nearest')
            db = util.scale_img_nhwc(db_full, [H, W], mag='nearest', min='nearest') * spp if db_full is not None else None
        # (the raster's only differentiable consumer at the shading resolution == visibility resolution is this pass -- antialias and composite take
        # it as a constant, the z / depth pass runs under no_grad --: its backward is folded into the G-buffer's, d3h.raster.gbuffer)
        fold = (H, W) == (Hf, Wf) and os.environ.get('D3H_FUSED_GBUFFER_RASTER_BWD', '1') != '0'
        groups, gb_geometric_normal, cover = _R.gbuffer(packed, [t.shape[-1] for _, t in srcs], rast, tri, face_attr=fn, want_mask=True,
                                                        raster_pos=v_pos_clip if fold else None)
        gb = {k: g for (k, _), g in zip(srcs, groups)}
        gb_pos, gb_pos_original, gb_normal, gb_msdf = gb.get('pos'), gb.get('orig'), gb.get('nrm'), gb.get('msdf')
        if need_nrm and own_nrm_idx:
            gb_normal, _ = interpolate(_batched(mesh.v_nrm), rast, mesh.t_nrm_idx.int())                  # render.py:272

        gb_tangent = None
        if perturb and 'normal' in want:
            gb_tangent, _ = interpolate(_batched(mesh.v_tng), rast, mesh.t_tng_idx.int())                # render.py:273
        elif 'normal' in want:
            with torch.no_grad():                                                    # render.py:284-287 (use_uv == False branch)
                noise = torch.randn_like(gb_normal) if _rng_draws is None else _rng_draws['noise'].to(dev)
                noise = noise / noise.norm(dim=-1, keepdim=True)
            gb_tangent = torch.cross(noise, gb_normal, dim=-1)

        # forward-only buffers in one fused pass: z / z-gradient (torch.no_grad in the reference, render.py:291-299) and, when nobody
        # differentiates them (the reference does only under FLAGS.use_depth), depth / inverse depth (render.py:197-199)
        aux = (None, None, None)
        if need_aux:
            aux = _R.aux_buffers(v_pos_clip, rast, db, tri, gb_pos, view_pos, want_z='z_grad' in want, want_depth=no_grad_of('depth'),
                                 want_invdepth=no_grad_of('invdepth'))

        layer = shade(FLAGS, idx, rast, aux, gb_pos, gb_pos_original, gb_geometric_normal, gb_normal, gb_tangent, view_pos, mesh.material,
                      want, finetune_normal, mask=cover, rng_draws=_rng_draws, live=live, skip_uncovered=(H, W) == (Hf, Wf), lit=lit,
                      tex2d={'lookup': lambda names: _material_lookups(mesh, rast, db, names, (H, W) == (Hf, Wf), cover), 'perturb': perturb,
                             'alpha': has_alpha} if tex2d else None)
        if lit is not None:
            layer = {k: t for k, t in layer.items() if k in want_out or k == '_alpha'}      # what the lit colour was made of is not an output unless asked for
        shaded_of = layer.pop('_shaded_of', None)
        if (H, W) != (Hf, Wf):
            shaded_of = None
        if has_msdf:
            layer['msdf_image'] = gb_msdf
        if (H, W) != (Hf, Wf):                        # back up to the visibility resolution (render.py:334-336)
            layer = {k: (util.scale_img_nhwc(t, [Hf, Wf], mag='nearest', min='nearest') if t is not None else None) for k, t in layer.items()}
        return layer, shaded_of, layer.pop('_alpha', None)

    layers = [shade_layer(r, d) for r, d in peeled]
    layer, shaded_of, _ = layers[0]
    if lit is not None:
        want, live = want_out, live_out

    # ---- composite against each buffer's background (one pass), then ONE antialias pass over all channels (render.py:375-382,430-449)
    if background is None:
        background = torch.zeros(1, Hf, Wf, 3, dtype=torch.float32, device=dev)
    elif spp > 1:
        background = util.scale_img_nhwc(background, [Hf, Wf], mag='nearest', min='nearest')          # render.py:424-425

    def compose(keys):
        sources = []
        for k in keys:
            if k == 'shaded':
                sources.append((layer[k], _I.COMP_IMAGE, background))
            elif k == 'depth':
                sources.append((layer[k], _I.COMP_CONST20, None))
            elif k == 'msdf_image':                     # lerp(0, 1, coverage * msdf): the value IS the alpha (render.py:444-449)
                sources.append((layer[k], _I.COMP_ALPHA, None))
            else:
                sources.append((layer[k], _I.COMP_ZERO, None))
        widths = [1 if k == 'msdf_image' else layer[k].shape[-1] + 1 for k in keys]
        if not torch.is_grad_enabled() and os.environ.get('D3H_FUSED_COMPOSITE_AA', '1') != '0':
            # nobody differentiates this pass (dead buffers, validation renders): composite + antialias as ONE forward kernel
            img = _I.composite_antialias(rast_full, sources, v_pos_clip, tri)
        elif os.environ.get('D3H_FUSED_COMPOSITE_AA_GRAD', '1') != '0':
            # the differentiated pass: one kernel each way, the composited pre-antialias image is never stored (round 6); the shaded colour
            # goes in as the texture MLP's whole output + "first three channels", so that its gradient comes back at that width in the same pass
            if shaded_of is not None and os.environ.get('D3H_FUSED_COMPOSITE_PREFIX', '1') != '0':
                sources = [(shaded_of, kind, bg_, 3) if k == 'shaded' else (s_, kind, bg_) for k, (s_, kind, bg_) in zip(keys, sources)]
            img = _I.composite_antialias_grad(rast_full, sources, v_pos_clip, tri)
        else:
            img = dr.antialias(_I.composite(rast_full, sources), rast_full, v_pos_clip, tri)
        return (util.avg_pool_nhwc(img, spp) if spp > 1 else img), widths                              # render.py:449

    layer_flags = []

    def edge_flags():
        """the silhouette-edge bits depend on (pos, tri) only: once per call, not per layer or group of buffers"""
        if not layer_flags:
            layer_flags.append(_R._edge_flags(v_pos_clip.detach().contiguous().float(), tri.contiguous(), B, Hf, Wf))
        return layer_flags[0]

    def compose_layers(keys):
        """the module docstring's loop over the peeled layers, back to front, on the channel-concatenated image of the buffers `keys`"""
        widths = [1 if k == 'msdf_image' else layer[k].shape[-1] + 1 for k in keys]
        kind = {'shaded': _I.COMP_IMAGE, 'depth': _I.COMP_CONST20, 'msdf_image': _I.COMP_ALPHA}
        # what lies behind the deepest layer: every buffer's background, written once
        acc = torch.zeros(B, Hf, Wf, sum(widths), dtype=torch.float32, device=dev)
        c0 = 0
        for k, n in zip(keys, widths):
            if k == 'shaded':
                acc[..., c0:c0 + 3] = background
            elif k == 'depth':
                acc[..., c0:c0 + n] = 20.0
            c0 += n
        fused = _layer_fused()
        flags = edge_flags() if fused else None
        for (lay, _, a), (r, _) in reversed(list(zip(layers, peeled))):
            if fused:
                acc = _I.layer_composite_antialias(r, [(lay[k], kind.get(k, _I.COMP_ZERO)) for k in keys], a, acc, v_pos_clip, tri, flags=flags)
                continue
            cov = (r[..., 3:4] > 0).float()
            w = cov if a is None else cov * a
            one = torch.ones_like(cov)
            end = torch.cat([one if k == 'msdf_image' else torch.cat((lay[k].expand(B, Hf, Wf, -1), one), dim=-1) for k in keys], dim=-1)
            if 'msdf_image' in keys:                  # its value IS its weight (render.py:444-449)
                w = torch.cat([cov * lay[k] if k == 'msdf_image' else w.expand(-1, -1, -1, n) for k, n in zip(keys, widths)], dim=-1)
            acc = dr.antialias(torch.lerp(acc, end, w), r, v_pos_clip, tri)
        return (util.avg_pool_nhwc(acc, spp) if spp > 1 else acc), widths

    layered = num_layers > 1 or has_alpha
    all_keys = [k for k in list(ALL_BUFFERS) + ['msdf_image'] + list(LIT_BUFFERS) + list(PERTURBED_BUFFERS) if k in layer]
    live_keys = all_keys if live is None else [k for k in all_keys if k in live]
    dead_keys = [k for k in all_keys if k not in live_keys]
    # '_stacked' / '_layout': the channel-concatenated image itself, for consumers that read several buffers in one pass
    # (d3h.imgops.pixel_losses); the per-buffer entries are views of it, as the reference's separate tensors would be
    out_buffers = {'_layout': {}}
    for name, keys, no_grad in (('_stacked', live_keys, False), ('_stacked_nograd', dead_keys, True)):
        # (the composite pass takes 12 sources: the reference's 11 buffers and the msdf image fit; the two light images of the lit branch, last in the
        # order, may overflow into a pass of their own, outside '_stacked' / '_layout', which no consumer of the layout reads them from; the same holds for
        # the two perturbed-normal buffers of a 2-D material, which come after them)
        for first in range(0, len(keys), 12):
            chunk = keys[first:first + 12]
            with torch.set_grad_enabled(grad_on and not no_grad):
                stacked, widths = compose_layers(chunk) if layered else compose(chunk)
            if first == 0:
                out_buffers[name] = stacked
            c0 = 0
            for k, n in zip(chunk, widths):
                out_buffers[k] = stacked[..., c0:c0 + n]
                if not no_grad and first == 0:
                    out_buffers['_layout'][k] = (c0, n)
                c0 += n
    if '_stacked' not in out_buffers:
        out_buffers['_stacked'] = None
    if _keep_rast:
        out_buffers['_rast'] = rast_full
    if buffers is None or 'visible_triangles' in buffers or '_seen_faces' in buffers:
        # render.py:404-407 -- sorted unique triangle ids; bitmap scatter + nonzero instead of sorting a million ids.  '_seen_faces'
        # is the bitmap itself: consumers that only need "is this triangle visible" avoid nonzero's host synchronisation
        seen = torch.zeros(F + 1, dtype=torch.bool, device=dev)
        # index_fill_, not `seen[ids] = True`: the indexed assignment uploads the Python scalar as a tensor, which synchronises the stream
        seen.index_fill_(0, rast_full[..., 3].reshape(-1).long(), True)
        out_buffers['_seen_faces'] = seen[1:]
        if buffers is None or 'visible_triangles' in buffers:
            out_buffers['visible_triangles'] = torch.nonzero(seen[1:]).reshape(-1)          # a plain int64 tensor, as the reference's
    return out_buffers


def render_uv(ctx, mesh, resolution, mlp_texture):
    """Texture bake of the export step (render.py:456-472; called by train.py:218 after xatlas): the mesh rasterised in its uv chart,
    world positions interpolated per texel, kd / ks sampled from the texture MLP.  -> (coverage [1,H,W,1], kd [1,H,W,3], ks [1,H,W,3])"""
    uv = mesh.v_tex[None, ...] * 2.0 - 1.0
    clip = torch.cat((uv, torch.zeros_like(uv[..., 0:1]), torch.ones_like(uv[..., 0:1])), dim=-1).contiguous()
    rast, _ = dr.rasterize(ctx, clip, mesh.t_tex_idx.int(), resolution)
    v_pos = mesh.v_pos if mesh.v_pos.dim() == 3 else mesh.v_pos[None, ...]
    gb_pos, _ = interpolate(v_pos, rast, mesh.t_pos_idx.int())
    cover = (rast[..., -1:] > 0).float()
    tex = mlp_texture.sample(gb_pos)                    # every texel, as the reference (uncovered texels are dilated over by the caller)
    assert tex.shape[-1] == 6, "Combined kd_ks must be 6 channels"
    return cover, tex[..., 0:3], tex[..., 3:6]
