"""Textured-mesh export: a fitted mesh with its MLP material -> a mesh with uv coordinates and kd / ks / normal texture maps that
render/obj.py:write_obj writes as mesh.obj + mesh.mtl + three PNGs (the reference's xatlas_uvmap, train.py:198-246).

The chart is the closed-form triangle-pair atlas of d3h.uvatlas, the bake evaluates the material once per texel at the position of the
owning triangle's affine map (gutter texels included, so nothing is dilated), and a level-0 bilinear lookup anywhere on the surface reads
texels of its own triangle only.  The maps are for level-0 bilinear use (mip levels above 0 mix triangles); (s - 4)^2 / s^2 of the texels of
a cell carry surface: the exported material says so with 'filter_mode': 'linear', which render.render.render_mesh honours (its default,
the mip-mapped Texture2D.sample, is off by up to 0.56 on values within +-0.6 on such a bake; level-0 bilinear stays within 3.9e-7).
`load_textured_mesh` reads the files write_obj wrote back as a renderable mesh.  `render.render.render_uv` is the rasterising route of the reference and stays as a cross-check."""
import os

import torch

from render import material as _material, mesh as _mesh, obj as _obj, texture as _texture
from . import uvatlas as _U


@torch.no_grad()
def textured_mesh(mesh, material, texture_res, kd_min, kd_max, ks_min, ks_max, nrm_min, nrm_max, transparency=False, alpha_init=1.0):
    """mesh: render.mesh.Mesh (v_pos [V,3], or [B,V,3] posed frames of which the first is baked); material: dict with 'kd_ks', an MLPTexture3D
    of 6 channels; texture_res: (H, W) or one int.  -> Mesh(v_tex, t_tex_idx, base=mesh) whose material is `material` without 'kd_ks' and with
    'kd', 'ks', 'normal' as trainable Texture2D ([1,H,W,3] each) clamped to the given ranges and 'filter_mode': 'linear' (module docstring); texels no triangle owns hold the mean of the owned ones.
    transparency (FLAGS.transparency of the reference, train.py:233): 'kd' is [1,H,W,4], the fourth channel the opacity render_mesh blends peeled
    layers with under FLAGS.transparency -- alpha_init everywhere (a number), or uniform random numbers in [0, 1) for alpha_init='rand' (the
    reference's rand_like); kd_min / kd_max of three entries get the opacity's bounds 0 and 1 appended, four entries are taken as given."""
    v_pos = mesh.v_pos[0] if mesh.v_pos.dim() == 3 else mesh.v_pos
    atlas = _U.make_atlas(v_pos, mesh.t_pos_idx, texture_res)
    pos, owned, _, _ = _U.bake_positions(atlas, v_pos, mesh.t_pos_idx)
    tex = material['kd_ks'].sample(pos, mask=owned)
    assert tex.shape[-1] == 6, 'Combined kd_ks must be 6 channels'
    mean = (tex * owned).sum(dim=(0, 1, 2)) / owned.sum().clamp(min=1.0)
    tex = torch.where(owned > 0, tex, mean.expand_as(tex))
    normal = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float32, device=tex.device).expand(*tex.shape[:3], 3)
    dev = tex.device
    rng = lambda lo, hi: [torch.as_tensor(lo, dtype=torch.float32, device=dev), torch.as_tensor(hi, dtype=torch.float32, device=dev)]
    leaf = lambda t: t.clone().detach().contiguous().requires_grad_(True)
    out = _mesh.Mesh(v_tex=atlas.uvs, t_tex_idx=atlas.t_tex_idx, base=mesh)
    out.material = {k: v for k, v in material.items() if k != 'kd_ks'}
    out.material['filter_mode'] = 'linear'
    kd = tex[..., 0:3]
    if transparency:
        if isinstance(alpha_init, str):
            if alpha_init != 'rand':
                raise ValueError(f"textured_mesh: alpha_init must be a number or 'rand', not {alpha_init!r}")
            alpha = torch.rand_like(kd[..., 0:1])
        else:
            alpha = torch.full_like(kd[..., 0:1], float(alpha_init))
        kd = torch.cat((kd, alpha), dim=-1)
        kd_min, kd_max = rng(kd_min, kd_max)
        if kd_min.numel() == 3:
            kd_min, kd_max = torch.cat((kd_min, kd_min.new_zeros(1))), torch.cat((kd_max, kd_max.new_ones(1)))
    out.material.update({'kd': _texture.Texture2D(leaf(kd), min_max=rng(kd_min, kd_max)),
                         'ks': _texture.Texture2D(leaf(tex[..., 3:6]), min_max=rng(ks_min, ks_max)),
                         'normal': _texture.Texture2D(leaf(normal), min_max=rng(nrm_min, nrm_max))})
    return out


def load_textured_mesh(obj_path, filter_mode='linear', clear_ks=False, device=None):
    """mesh.obj + the first material of the .mtl next to it (the `mtllib` line's file, mesh.mtl when there is none) -> a Mesh render_mesh can draw:
    positions, uvs and faces of render.obj.load_obj, the file's normals or auto_normals when it has no `vn`, tangents from compute_tangents, and
    the material of render.material.load_mtl with 'filter_mode' set (what the maps were baked for: module docstring).  Everything on `device`
    (None: the GPU when there is one)."""
    m = _obj.load_obj(obj_path, device=device)
    if m.v_tex is None or m.t_tex_idx is None:
        raise ValueError(f'load_textured_mesh: {obj_path} has no texture coordinates')
    mtl = 'mesh.mtl'
    with open(obj_path) as fh:
        for line in fh:
            p = line.split()
            if len(p) > 1 and p[0].lower() == 'mtllib':
                mtl = p[1]
                break
    mats = _material.load_mtl(os.path.join(os.path.dirname(obj_path), mtl), clear_ks=clear_ks)
    if not mats:
        raise ValueError(f'load_textured_mesh: {mtl} defines no material')
    mat = dict(mats[0])
    dev = m.v_pos.device
    for k, v in mat.items():
        if isinstance(v, _texture.Texture2D):
            v.data = [l.to(dev) for l in v.data] if isinstance(v.data, list) else v.data.to(dev)
        elif torch.is_tensor(v):
            mat[k] = v.to(dev)
    mat['filter_mode'] = filter_mode
    m.material = mat
    if m.v_nrm is None:
        m = _mesh.auto_normals(m)
    return _mesh.compute_tangents(m)


def _per_level(texture_res, levels):
    """one value -- an int or an (H, W) pair of ints -- for every level, or a sequence of `levels` such values (a pair of ints is always (H, W))"""
    one = lambda r: isinstance(r, int) or (isinstance(r, (list, tuple)) and len(r) == 2 and all(isinstance(x, int) for x in r))
    if one(texture_res):
        return [texture_res] * levels
    if not isinstance(texture_res, (list, tuple)) or len(texture_res) != levels or not all(one(r) for r in texture_res):
        raise ValueError(f'lod_chain: texture_res must be one resolution or one per level ({levels}), got {texture_res!r}')
    return list(texture_res)


@torch.no_grad()
def lod_chain(mesh, material, face_counts, texture_res, kd_min, kd_max, ks_min, ks_max, nrm_min, nrm_max, **decimate_kw):
    """A chain of levels of detail of a fitted mesh, each a textured_mesh of its own: fewer faces give the triangle-pair atlas larger cells, so a
    coarser level uses its maps better ((s - 4)^2 / s^2 of a cell carries surface: 25 % at 131 072 faces on 2048^2, 67 % at 16 384).
    face_counts: absolute, strictly decreasing, one per level.  Level 0 is textured_mesh(mesh, ...) whatever face_counts[0] says; level i is
    d3h.meshrefine.decimate (quadric error metric, **decimate_kw passed on) of level i - 1's geometry down to face_counts[i], then auto_normals, then
    textured_mesh with the same material: the material is volumetric (an MLPTexture3D under 'kd_ks'), so a coarse level gets its colours by
    sampling it at its OWN surface -- nothing is baked from fine to coarse, and every level keeps the flat (0, 0, 1) normal map.  A count that
    decimation cannot reach is no error: the level's real count is on its mesh.  texture_res: one resolution (an int or (H, W)) or one per level.
    -> [Mesh, ...].  A material without 'kd_ks' (2-D maps) raises."""
    from . import meshrefine as _MR
    counts = [int(c) for c in face_counts]
    if not counts or counts[-1] < 0 or any(b >= a for a, b in zip(counts, counts[1:])):
        raise ValueError(f'lod_chain: face_counts must be non-negative and strictly decreasing, got {list(face_counts)!r}')
    if 'kd_ks' not in material:
        raise ValueError("lod_chain: the material must be volumetric ('kd_ks'); 2-D maps cannot be sampled at a coarser surface")
    res = _per_level(texture_res, len(counts))
    ranges = (kd_min, kd_max, ks_min, ks_max, nrm_min, nrm_max)
    chain = [textured_mesh(mesh, material, res[0], *ranges)]
    v = (mesh.v_pos[0] if mesh.v_pos.dim() == 3 else mesh.v_pos).detach().float().contiguous()
    f = mesh.t_pos_idx
    for count, r in zip(counts[1:], res[1:]):
        v, f, _, _, _ = _MR.decimate(v, f, count, **decimate_kw)
        chain.append(textured_mesh(_mesh.auto_normals(_mesh.Mesh(v, f, material=material)), material, r, *ranges))
    return chain


def write_lod_chain(folder, chain):
    """folder/lod{i}/mesh.obj + mesh.mtl + the three maps of every level, through render.obj.write_obj; load_textured_mesh reads each back.
    -> the folders written"""
    out = []
    for i, level in enumerate(chain):
        sub = os.path.join(folder, f'lod{i}')
        os.makedirs(sub, exist_ok=True)
        _obj.write_obj(sub, level)
        out.append(sub)
    return out
