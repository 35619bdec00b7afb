"""script/process_body_cloth_head_msdfcut.py of the reference on this build: the second half of the hand-off from the split stage to the seq stage
(train.py:1858 calls process_body_msdf_distance_bodyedge on the meshes process_close_hole left; the seq stage reads merge_body_cloth.obj,
merge_body_cloth.npz and inside_body_index.npz, train.py:1865, dataset/dataset_split.py).  Same signatures over numpy arrays and paths, same three files
with the same keys and dtypes.  The reference makes five meshlabserver calls under xvfb-run and uses pysdf, open3d and openmesh; none of them is used
here.  `script` is a namespace package (see connet_face_head.py): with both roots on the path this file resolves before the reference's.

The route, step by step (reference lines :613-747), and every deviation:
  1. "remesh" (remesh.mlx: MeshLab isotropic remeshing to 0.01, three iterations) is d3h.meshrefine.refine_long_edges(4/3 target_len, iterations=3): the
     refine step alone.  There is no collapse, flip or tangential smoothing, so short edges stay and vertices are never moved.  That is the default,
     remesh='split'.  remesh='isotropic' runs d3h.meshrefine.isotropic_remesh(target_len, 3) in its place, here and in step 5: per iteration a split
     above 4/3 target_len, collapses below 4/5 target_len, valence-improving flips, one tangential smoothing pass and the reprojection of every moved
     vertex onto the input surface (one BVH per call).  What remains of the deviation: boundary and non-manifold vertices are pinned (MeshLab moves
     boundary vertices along the boundary), independent operations are chosen by a deterministic minimum instead of MeshLab's sequential sweep, and
     there is no adaptive length and no surface-distance check per operation.  process_subdivide (step 6) keeps its thresholded split either way.
  2. The garment is never made watertight and never extracted (wt.mlx: screened Poisson at depth 8, then pysdf): GarmentField answers the distance
     queries directly on the open garment, as -mesh_wsdf: distance to the nearest triangle, signed by the generalised winding number (|w| > 0.5 inside).
     field_accel='bvh' (default 'brute': the loop over every triangle) answers them, and the field of step 5, from a d3h.raytrace.Bvh: the garment's is
     built once for all push rounds.
  3. One ring of open faces is peeled off the cut SMPL, whose vertices are pushed inward along their normals (deform_body_collision: 0.005 per round
     while less than 0.002 inside, at most 100 rounds).  The reference's sweep is a Jacobi sweep too; its kd-tree query per pushed vertex has no effect
     and is left out.  The device route stops when a round moves nothing (the remaining rounds would move nothing either).
     Vertex normals are d3h.imgops.auto_normals: area weighted, where openmesh sums unit face normals.
  4. Two rings are peeled off the visible body parts, which are stacked with the pushed SMPL and welded (merge_and_repair_meshes, d3h.meshtopo).
  5. The merge is made watertight by d3h.watertight.watertight (winding-number field on a Kuhn lattice, marching tets, relaxed caps) in place of screened
     Poisson, then refined as in 1.  The surface is therefore the input surface to within a quarter cell away from the cuts, not Poisson's smoothed one.
  6. process_subdivide: the faces whose three vertices lie in the head box (+- 0.01) are refined with refine_long_edges(head_threshold,
     head_iterations, face_mask=...) (midpoint_head.mlx: "Midpoint" on edges above 0.002, three iterations).  Unmasked neighbours of a split edge are
     split too, so the result is conforming; the reference subdivides the head faces as a mesh of their own and stacks them back, which leaves
     T-junctions (cracks) along the box.
  7. The body (face_labels 0) and the refined garment (1) are stacked; find_inside_point records which body vertices the garment covers.
  Lines :631-655 of the reference (a distance map, components and valid_smpl_face that nothing reads) and the remesh of smpl_path at :621 that feeds
  only them are left out: smpl_path is checked for existence and not read.  get_tet_mesh / smpl_msdf, which the reference creates and never reads,
  and the other process_* variants of the reference file are not provided.
  Files: merge_body_cloth.obj / .npz and inside_body_index.npz as the reference; of the intermediates only those this route produces, under the
  reference's base names: deform_smpl.obj, body_edge_cut.obj, all_v_f.obj (+ inside_body_v.obj / outside_body_v.obj from find_inside_point); they are
  side outputs: the body's positions go from step 5 to the .npz without passing through a text file.  OBJ files are in
  write_pc's format; openmesh may drop faces it finds non-manifold when it loads a file, here every `f` line is kept.
  `script_root` and `local` are accepted and ignored."""
import os

import numpy as np
import torch

from d3h import imgops as IO
from d3h import meshops as MO
from d3h import meshrefine as MR
from d3h import meshtopo as MT
from d3h import raytrace as RT
from d3h import watertight as WT
from script.connet_face_head import MergedMesh, _device, om_loadmesh, write_pc


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(_device())


def _faces(f):
    return _t(np.asarray(f).reshape(-1, 3), np.int64)


def find_open_edges(faces):
    """-> (open vertices as an ascending list, the unique sorted edges [E,2]); `faces` a tensor or an array [F,3]"""
    f = faces if torch.is_tensor(faces) else torch.from_numpy(np.asarray(faces))
    f = f.reshape(-1, 3).long()
    edges = torch.sort(torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], dim=0), dim=1)[0]
    unique_edges = torch.unique(edges, dim=0)
    nv = int(f.max()) + 1 if f.numel() else 0
    return MT.open_vertices(f.to(_device()), nv).cpu().tolist(), unique_edges


def remove_faces_with_open_vertices(faces, open_vertices):
    faces = np.asarray(faces)
    return faces[~np.isin(faces, np.array(open_vertices)).any(axis=1)]


def merge_and_repair_meshes(mesh1, mesh2):
    """mesh1, mesh2: anything with .vertices and .triangles (arrays)"""
    v, f = MT.merge_and_repair(_t(mesh1.vertices, np.float64).reshape(-1, 3), _faces(mesh1.triangles), _t(mesh2.vertices, np.float64).reshape(-1, 3),
                               _faces(mesh2.triangles))
    return MergedMesh(v.cpu().numpy(), f.cpu().numpy())


def merge_meshes_with_face_labels(mesh1, mesh2):
    """-> (merged mesh, labels, vertices, triangles); unlike the reference, mesh2's triangles are not shifted in place"""
    vertices1, vertices2 = np.asarray(mesh1.vertices), np.asarray(mesh2.vertices)
    triangles1, triangles2 = np.asarray(mesh1.triangles).reshape(-1, 3), np.asarray(mesh2.triangles).reshape(-1, 3) + len(vertices1)
    vertices = np.vstack((vertices1, vertices2))
    triangles = np.vstack((triangles1, triangles2))
    labels = np.concatenate((np.zeros(len(triangles1), dtype=int), np.ones(len(triangles2), dtype=int)))
    return MergedMesh(vertices, triangles), labels, vertices, triangles


def find_inside_point(v, body_index, sdf_gt_fn, root):
    sdf_values = np.asarray(sdf_gt_fn(v[body_index]))
    inside_body_index = np.nonzero(np.isin(body_index, body_index[np.where(sdf_values > -0.002)]))[0]
    write_pc(os.path.join(root, "inside_body_v.obj"), v=v[inside_body_index])
    outside_body_index = np.nonzero(np.isin(body_index, body_index[np.where(sdf_values <= -0.002)]))[0]
    write_pc(os.path.join(root, "outside_body_v.obj"), v=v[outside_body_index])
    return inside_body_index, outside_body_index


def face_in_bbox(v_indices, f):
    f = np.asarray(f).reshape(-1, 3)
    inside = np.isin(f, np.asarray(v_indices)).all(axis=1)
    return f[inside], f[~inside]


class GarmentField:
    """the signed distance to the OPEN garment mesh with pysdf's sign (positive inside): -mesh_wsdf.  Callable on numpy [n,3] -> numpy [n], as a
    pysdf.SDF is; `device(x)` takes and returns tensors on the device.  accel='bvh': the garment does not change between the rounds that query it, so
    one d3h.raytrace.Bvh is built here and every query is answered from it (meshops.mesh_wsdf, accel)"""

    def __init__(self, v, f, accel='brute'):
        self.v, self.f = _t(v, np.float32).reshape(-1, 3), _faces(f).int().contiguous()
        if self.f.shape[0] == 0 or int(self.f.min()) < 0 or int(self.f.max()) >= self.v.shape[0]:      # once: the queries below skip the check
            raise RuntimeError('GarmentField: no faces, or a face index outside [0, V)')
        if accel not in MO.ACCELS:
            raise RuntimeError(f'GarmentField: accel must be one of {MO.ACCELS}, got {accel!r}')
        self.accel = accel
        self.bvh = RT.Bvh(self.v, self.f) if accel == 'bvh' else None

    def device(self, x):
        return -MO.mesh_wsdf(x, self.v, self.f, want_w=False, check=False, accel=self.accel, bvh=self.bvh)[0]

    def __call__(self, x):
        return self.device(_t(x, np.float32).reshape(-1, 3)).cpu().numpy()


def deform_body_collision(cloth_v, cloth_n, body_v, body_n, sdf_gt_fn, epsilon=0.005, margin=0.002, rounds=100):
    """pushes body_v inward along body_n while sdf_gt_fn (positive inside) is below `margin`.  cloth_v / cloth_n are unused (the reference builds a
    kd-tree of cloth_v whose answers it drops).  With a GarmentField the rounds stay on the device; any other callable is evaluated on the host,
    in float64 as the reference does."""
    if isinstance(sdf_gt_fn, GarmentField):
        out, _ = MO.collision_push(_t(body_v, np.float32), _t(body_n, np.float32), sdf_gt_fn.device, eps=epsilon, margin=margin, rounds=rounds)
        return out.cpu().numpy().astype(np.float64)
    deformed = np.array(body_v, dtype=np.float64)
    body_n = np.asarray(body_n, np.float64)
    unit = body_n / (np.linalg.norm(body_n, axis=1, keepdims=True) + 0.0000001)
    for _ in range(int(rounds)):
        push = np.asarray(sdf_gt_fn(np.array(deformed))) < margin
        deformed[push] -= unit[push] * epsilon
    return deformed


def _normals(v, f):
    return IO.auto_normals(_t(v, np.float32), _faces(f).int()).cpu().numpy()


def _remesh_tensors(v, f, target_len, remesh):
    """remesh='split': the refine step alone; 'isotropic': split, collapse, flip, smooth and reproject (d3h.meshrefine.isotropic_remesh)"""
    if remesh == 'isotropic':
        return MR.isotropic_remesh(v, f, target_len, 3)[:2]
    return MR.refine_long_edges(v, f, 4.0 / 3.0 * target_len, iterations=3)[:2]


def _remesh(v, f, target_len, remesh='split'):
    return _remesh_tensors(_t(v, np.float32), _faces(f), target_len, remesh)


def _head_faces(v, f, bbox_npz_path):
    box = np.load(bbox_npz_path)
    inside = np.all((v >= (box["bbox_min"] - 0.01)) & (v <= (box["bbox_max"] + 0.01)), axis=1)
    return inside[f].all(axis=1)


def _subdivide(v, f, bbox_npz_path, root, head_threshold, head_iterations):
    """tensors in, tensors out; all_v_f.obj is a side output"""
    mask = _t(_head_faces(v.cpu().numpy(), f.cpu().numpy(), bbox_npz_path), np.bool_)
    v, f, _ = MR.refine_long_edges(v, f, head_threshold, head_iterations, face_mask=mask)
    add_v_path = os.path.join(root, "all_v_f.obj")
    write_pc(add_v_path, v=v.cpu().numpy(), f=f.cpu().numpy())
    return v, f, add_v_path


def process_subdivide(body_path, bbox_npz_path, root, script_root=None, local=False, *, head_threshold=0.002, head_iterations=3):
    body_v, body_f = om_loadmesh(body_path)
    return _subdivide(_t(body_v, np.float32), _faces(body_f), bbox_npz_path, root, head_threshold, head_iterations)[2]


def process_body_msdf_distance_bodyedge(FLAGS, root, body_path, ori_cloth_path, smpl_cloth_path, smpl_path, bbox_npz_path, script_root="checkpoints/script",
                                        local=False, *, target_len=0.01, wt_res=128, relax_iters=32, head_threshold=0.002, head_iterations=3, push_eps=0.005,
                                        push_margin=0.002, push_rounds=100, field_accel='brute', remesh='split'):
    if remesh not in ('split', 'isotropic'):
        raise RuntimeError(f"process_body_msdf_distance_bodyedge: remesh must be 'split' or 'isotropic', got {remesh!r}")
    for p in (body_path, ori_cloth_path, smpl_cloth_path, smpl_path, bbox_npz_path):
        if not os.path.exists(p):
            raise FileNotFoundError(f'process_body_msdf_distance_bodyedge: {p} does not exist')
    os.makedirs(root, exist_ok=True)

    # 1. the garment and the SMPL part under it, refined
    cloth_v, cloth_f = _remesh(*om_loadmesh(ori_cloth_path), target_len, remesh)
    cut_v, cut_f = _remesh(*om_loadmesh(smpl_cloth_path), target_len, remesh)
    # 2. the garment as a distance oracle
    garment = GarmentField(cloth_v.cpu().numpy(), cloth_f.cpu().numpy(), accel=field_accel)
    # 3. one ring off the cut SMPL, pushed under the garment
    cut_f = MT.peel_open_faces(cut_f, cut_v.shape[0], rounds=1)
    cut_v, cut_f = cut_v.cpu().numpy(), cut_f.cpu().numpy()
    deformed_v = deform_body_collision(garment.v.cpu().numpy(), None, cut_v, _normals(cut_v, cut_f), garment, push_eps, push_margin, push_rounds)
    write_pc(os.path.join(root, "deform_smpl.obj"), v=deformed_v, f=cut_f)
    # 4. two rings off the visible body parts, merged with the pushed SMPL
    body_v, body_f = om_loadmesh(body_path)
    body_f = MT.peel_open_faces(_faces(body_f), len(body_v), rounds=2).cpu().numpy()
    write_pc(os.path.join(root, "body_edge_cut.obj"), v=body_v, f=body_f)
    merged = merge_and_repair_meshes(MergedMesh(deformed_v, cut_f), MergedMesh(body_v, body_f))
    # 5. watertight, refined
    wt_v, wt_f, _ = WT.watertight(_t(merged.vertices, np.float32), _faces(merged.triangles), res=wt_res, relax_iters=relax_iters, accel=field_accel)
    wt_v, wt_f = _remesh_tensors(wt_v, wt_f, target_len, remesh)
    # 6. the head box, subdivided (the positions stay on the device; all_v_f.obj is written beside)
    sub_v, sub_f, _ = _subdivide(wt_v, wt_f, bbox_npz_path, root, head_threshold, head_iterations)
    # 7. body + garment under face labels, and the body vertices the garment covers
    _, face_labels, v, f = merge_meshes_with_face_labels(MergedMesh(sub_v.cpu().numpy().astype(np.float64), sub_f.cpu().numpy().astype(np.int32)),
                                                         MergedMesh(cloth_v.cpu().numpy().astype(np.float64), cloth_f.cpu().numpy().astype(np.int32)))
    write_pc(os.path.join(root, "merge_body_cloth.obj"), v=v, f=f)
    np.savez(os.path.join(root, "merge_body_cloth.npz"), v=v, f=f, face_labels=face_labels)
    body_index = np.unique(f[face_labels == 0])
    inside_body_index, outside_body_index = find_inside_point(v, body_index, garment, root)
    np.savez(os.path.join(root, "inside_body_index.npz"), inside_body_index=inside_body_index, outside_body_index=outside_body_index)
