"""script/connet_face_head.py of the reference on this build: the hand-off from the split stage to the seq stage (train.py:1792, :1843 call
process_close_hole on the split stage's body and garment meshes).  Same functions, same signatures over numpy arrays, same files written;
the component labelling and the vertex weld run on the device (d3h/meshtopo.py, csrc/meshtopo.hip) instead of Python dicts and per-face
`set.issubset` loops.

This directory has no __init__.py on purpose: `script` is a namespace package in the reference too, so with both roots on the path
`script.connet_face_head`, `script.process_body_cloth_head_msdfcut` and `script.get_tet_smpl` resolve here while any other `script` module keeps
resolving to the reference's file.

Deviations from the reference:
  * openmesh may drop faces it finds non-manifold when it loads a file; here every `f` line is kept;
  * cloth_concat.obj / body_concat.obj are written in write_pc's format (`v %f %f %f`, `f` 1-based), not in open3d's OBJ dialect;
  * open3d's remove_duplicated_vertices / remove_degenerate_triangles are restated from their documented behaviour (exact coordinates, first
    occurrence kept, order kept; triangles with two equal indices dropped) and are not pinned against open3d itself."""
import os
from collections import namedtuple

import numpy as np
import torch

from d3h import _lib as L
from d3h import meshtopo as MT

MergedMesh = namedtuple('MergedMesh', 'vertices triangles')


def _device():
    return 'cpu' if L.emulated() else 'cuda'


def write_pc(path_mesh, v, vn=None, f=None):
    v = np.asarray(v)
    assert v.ndim == 2 and v.shape[1] == 3
    with open(path_mesh, 'w') as fp:
        fp.write(''.join('v %f %f %f\n' % tuple(r) for r in v.tolist()))
        if vn is not None:
            fp.write(''.join('vn %f %f %f\n' % tuple(r) for r in np.asarray(vn).tolist()))
        if f is not None:
            fp.write(''.join('f %d %d %d\n' % tuple(r) for r in (np.asarray(f).reshape(-1, 3) + 1).tolist()))


def om_loadmesh(path):
    """-> (v float64 [n,3] as parsed, f int32 [m,3]): `v x y z` and triangle `f a b c` lines, `a/b/c` forms accepted, negative (relative) indices
    resolved; any other polygon is a ValueError"""
    v, f = [], []
    with open(path) as fp:
        for ln, line in enumerate(fp, 1):
            t = line.split()
            if not t:
                continue
            if t[0] == 'v':
                v.append((float(t[1]), float(t[2]), float(t[3])))
            elif t[0] == 'f':
                if len(t) != 4:
                    raise ValueError(f'{path}:{ln}: a face of {len(t) - 1} vertices; only triangles are read')
                idx = [int(s.split('/')[0]) for s in t[1:]]
                f.append([i - 1 if i > 0 else len(v) + i for i in idx])
    return np.asarray(v, np.float64).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)


def _labels(n_vertices, faces):
    f = torch.from_numpy(np.ascontiguousarray(np.asarray(faces).reshape(-1, 3))).to(_device())
    if f.dtype not in (torch.int32, torch.int64):
        f = f.long()
    return f, MT.connected_components(f, n_vertices)


def find_connected_components(vertices, faces):
    """-> the components as lists of vertex indices (ascending), in the order of their smallest vertex -- the reference's dict order"""
    lab = _labels(len(vertices), faces)[1].cpu().numpy()
    order = np.argsort(lab, kind='stable')
    cuts = np.flatnonzero(np.diff(lab[order])) + 1
    return [c.tolist() for c in np.split(order, cuts)] if len(lab) else []


def filter_and_sort_components(components):
    return sorted((c for c in components if len(c) > 1), key=len, reverse=True)          # stable: ties keep their order


def body_head_box(body_components, body_v):
    """the box (-/+ 0.01) of the component with the largest mean y, the first one on a tie"""
    ys = [np.mean(body_v[c], axis=0)[1] for c in body_components]
    head = body_v[body_components[ys.index(max(ys))]]
    return np.min(head, axis=0) - 0.01, np.max(head, axis=0) + 0.01


def merge_and_repair_meshes(mesh1_v, mesh1_f, mesh2_v, mesh2_f):
    dev = _device()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(dev)
    v, f = MT.merge_and_repair(t(mesh1_v, np.float64).reshape(-1, 3), t(mesh1_f, np.int64).reshape(-1, 3),
                               t(mesh2_v, np.float64).reshape(-1, 3), t(mesh2_f, np.int64).reshape(-1, 3))
    return MergedMesh(v.cpu().numpy(), f.cpu().numpy())


def _split(v, f, keep_first):
    """faces of the first `keep_first` ranked components, faces of the others (each grouped in rank order, file order inside a group)"""
    ft, lab = _labels(len(v), f)
    ranked, _ = MT.rank_components(lab)
    stay = MT.faces_by_component(ft, lab, ranked[:keep_first]).cpu().numpy()
    go = MT.faces_by_component(ft, lab, ranked[keep_first:]).cpu().numpy()
    lab = lab.cpu().numpy()
    kept = [np.flatnonzero(lab == r).tolist() for r in ranked[:keep_first].tolist()]
    return stay, go, kept


def process_close_hole(FLAGS, root, body_mesh, cloth_mesh, num=5):
    body_v, body_f = om_loadmesh(body_mesh)
    cloth_v, cloth_f = om_loadmesh(cloth_mesh)

    # body: the `num` largest components stay, the rest goes to the garment; garment: the largest stays, the rest goes to the body
    body_frombody_faces, cloth_frombody_faces, body_components_frombody = _split(body_v, body_f, num)
    cloth_fromcloth_faces, body_fromcloth_faces, _ = _split(cloth_v, cloth_f, 1)

    print("body_components_frombody:", len(body_components_frombody))
    bbox_min, bbox_max = body_head_box(body_components_frombody, body_v)
    bbox_path = os.path.join(root, "bbox.npz")
    np.savez(bbox_path, bbox_min=bbox_min, bbox_max=bbox_max)

    path_body_frombody_faces = os.path.join(root, "body_frombody_faces.obj")
    write_pc(path_body_frombody_faces, v=body_v, f=body_frombody_faces)
    write_pc(os.path.join(root, "cloth_frombody_faces.obj"), v=body_v, f=cloth_frombody_faces)
    write_pc(os.path.join(root, "body_fromcloth_faces.obj"), v=cloth_v, f=body_fromcloth_faces)
    write_pc(os.path.join(root, "cloth_fromcloth_faces.obj"), v=cloth_v, f=cloth_fromcloth_faces)

    if len(cloth_frombody_faces) != 0 and len(cloth_fromcloth_faces) != 0:
        merge_cloth = merge_and_repair_meshes(body_v, cloth_frombody_faces, cloth_v, cloth_fromcloth_faces)
        cloth_concat_path = os.path.join(root, "cloth_concat.obj")
        write_pc(cloth_concat_path, v=merge_cloth.vertices, f=merge_cloth.triangles)
    else:
        cloth_concat_path = cloth_mesh

    if len(body_frombody_faces) != 0 and len(body_fromcloth_faces) != 0:
        merge_body = merge_and_repair_meshes(body_v, body_frombody_faces, cloth_v, body_fromcloth_faces)
        body_concat_path = os.path.join(root, "body_concat.obj")
        write_pc(body_concat_path, v=merge_body.vertices, f=merge_body.triangles)
    else:
        body_concat_path = path_body_frombody_faces

    return body_concat_path, cloth_concat_path, bbox_path
