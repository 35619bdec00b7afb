"""Materials as dictionaries of textures, with the interface of the reference's render/material.py (:21-169): `load_mtl`, `save_mtl`,
`create_trainable`, `get_parameters`, `merge_materials`.  Written for this build on top of render/texture.py; the .mtl dialect is the
reference's (`bsdf`, `map_Kd` stored in sRGB, `map_Ks`, `bump` stored as (n + 1) / 2)."""
import os

import numpy as np
import torch

from . import mlptexture, texture, util

_FILE_KEYS = ('bsdf', 'map_kd', 'map_ks', 'bump')


def _device():
    return 'cuda' if torch.cuda.is_available() else 'cpu'


def load_mtl(fn, clear_ks=True):
    """-> list of material dicts, one per `newmtl`.  kd / ks become Texture2D (1 x 1 for constants), kd is converted from sRGB to linear; clear_ks
    zeroes the first ks channel (the occlusion slot of an ORM map, which the shading uses for something else)."""
    folder = os.path.dirname(fn)
    materials = []
    with open(fn) as f:
        for line in f:
            words = line.split()
            if not words:
                continue
            key, args = words[0].lower(), words[1:]
            if 'newmtl' in key:
                materials.append({'name': args[0]})
            elif materials:
                if any(k in key for k in _FILE_KEYS):
                    materials[-1][key] = args[0]
                else:
                    materials[-1][key] = torch.tensor([float(a) for a in args], dtype=torch.float32, device=_device())
    for mat in materials:
        mat.setdefault('bsdf', 'pbr')
        mat['kd'] = texture.load_texture2D(os.path.join(folder, mat['map_kd'])) if 'map_kd' in mat else texture.Texture2D(mat['kd'])
        mat['ks'] = texture.load_texture2D(os.path.join(folder, mat['map_ks']), channels=3) if 'map_ks' in mat else texture.Texture2D(mat['ks'])
        if 'bump' in mat:
            mat['normal'] = texture.load_texture2D(os.path.join(folder, mat['bump']), lambda_fn=lambda x: x * 2 - 1, channels=3)
        mat['kd'] = texture.srgb_to_rgb(mat['kd'])
        if clear_ks:
            for level in mat['ks'].getMips():
                level[..., 0] = 0.0
    return materials


def save_mtl(fn, material):
    """one material `defaultMat`; its kd / ks / normal maps as texture_kd.png (sRGB), texture_ks.png, texture_n.png next to `fn`"""
    folder = os.path.dirname(fn)
    lines = ['newmtl defaultMat']
    if material is None:
        lines += ['Kd 1 1 1', 'Ks 0 0 0', 'Ka 0 0 0', 'Tf 1 1 1', 'Ni 1', 'Ns 0']
    else:
        lines.append('bsdf   %s' % material['bsdf'])
        if 'kd' in material.keys():
            lines.append('map_Kd texture_kd.png')
            texture.save_texture2D(os.path.join(folder, 'texture_kd.png'), texture.rgb_to_srgb(material['kd']))
        if 'ks' in material.keys():
            lines.append('map_Ks texture_ks.png')
            texture.save_texture2D(os.path.join(folder, 'texture_ks.png'), material['ks'])
        if 'normal' in material.keys():
            lines.append('bump texture_n.png')
            texture.save_texture2D(os.path.join(folder, 'texture_n.png'), material['normal'], lambda_fn=lambda x: (util.safe_normalize(x) + 1) * 0.5)
    with open(fn, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def create_trainable(material):
    """a copy of the material with every Texture2D replaced by a trainable one"""
    return {k: texture.create_trainable(v) if isinstance(v, texture.Texture2D) else v for k, v in material.items()}


def get_parameters(material):
    out = []
    for v in material.values():
        if isinstance(v, (texture.Texture2D, mlptexture.MLPTexture3D)):
            out += list(v.parameters())
    return out


def merge_materials(materials, texcoords, tfaces, mfaces):
    """several materials -> one: their maps side by side along x (each scaled to the largest resolution, the sheet padded to a power of two by
    edge replication), texture coordinates moved into their material's strip.  -> (material, new texcoords, tfaces re-indexed in place)"""
    assert len(materials) > 0
    first = materials[0]
    for mat in materials:
        assert mat['bsdf'] == first['bsdf'], 'All materials must have the same BSDF (uber shader)'
        assert ('normal' in mat) is ('normal' in first), 'All materials must have either normal map enabled or disabled'
    maps = ('kd', 'ks', 'normal')
    res = np.array([1, 1])
    for mat in materials:
        for k in maps:
            if k in mat:
                res = np.maximum(res, np.array(mat[k].getRes()))
    full = (2 ** np.ceil(np.log2(res * np.array([1, len(materials)])))).astype(np.int64)
    merged = {'name': 'uber_material', 'bsdf': first['bsdf']}
    for k in maps:
        if k in first:
            sheet = torch.cat([util.scale_img_nhwc(mat[k].data, tuple(int(r) for r in res)) for mat in materials], dim=2).permute(0, 3, 1, 2)
            sheet = torch.nn.functional.pad(sheet, (0, int(full[1]) - sheet.shape[3], 0, int(full[0]) - sheet.shape[2]), 'replicate')
            merged[k] = texture.Texture2D(sheet.permute(0, 2, 3, 1).contiguous())
    sy, sx = full[0] / res[0], full[1] / res[1]
    slot, new_tc = {}, []
    for fi in range(len(tfaces)):
        m = mfaces[fi]
        for c in range(3):
            key = (tfaces[fi][c], m)
            if key not in slot:
                u, v = texcoords[key[0]][0], texcoords[key[0]][1]
                new_tc.append([(m + u) / sx, v / sy])
                slot[key] = len(new_tc) - 1
            tfaces[fi][c] = slot[key]
    return merged, new_tc, tfaces
