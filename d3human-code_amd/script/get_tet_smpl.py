"""script/get_tet_smpl.py of the reference on this build: the tetrahedral mesh of the SMPL-X template that HmSDFTetsGeometry._init_sdf builds at
start-up (geometry/hmsdf.py:239-243).  Same functions, same positional signature, same return and the same two files; the reference's tetgen
(behind pyvista) is replaced by d3h.tetfill.fill_mesh (csrc/tetfill.hip).

Deviations from the reference:
  * the result is a CLIPPED LATTICE, not a constrained Delaunay mesh: a Kuhn lattice over the cube of d3h.watertight (centred on the bounding box,
    side = scale x the longest extent, res cells per side) cut by the linear interpolant of the mesh's winding-signed distance.  Its boundary is the
    marching-tets surface of that field, within about a lattice pitch of the template and not on it;
  * no template vertex is a vertex of the result (tetgen keeps the input surface's vertices);
  * tetgen's maxvolume = 6e-3 has no counterpart: the size of the cells is the pitch side / res (inner tets have volume pitch^3 / 6); cut tets can
    be arbitrarily thin, nothing is snapped;
  * tet.make_manifold is not needed: an open, consistently wound mesh is closed by the |winding number| = 0.5 surface;
  * the OBJ is read by script.connet_face_head.om_loadmesh (triangles only);
  * get_tet_mesh_test (pytetwild, an interactive plot) is not provided."""
import numpy as np
import torch

from d3h import tetfill as _tetfill

from . import connet_face_head as _cf


def get_tet_mesh(mesh_path, save_npz_path, res=64, scale=1.1):
    """-> (vertices float32 [n,3], indices int64 [m,4]); writes save_npz_path (keys v, f) and the .obj beside it"""
    v, f = _cf.om_loadmesh(mesh_path)
    dev = _cf._device()
    tv, tt, _ = _tetfill.fill_mesh(torch.as_tensor(v, device=dev).float(), torch.as_tensor(f, device=dev), res=res, scale=scale)
    vertices, indices = tv.cpu().numpy().astype(np.float32), tt.cpu().numpy()
    save_tet_mesh_as_obj(vertices, indices, save_npz_path.replace("npz", "obj"))
    np.savez(save_npz_path, v=vertices, f=indices)
    return vertices, indices


def save_tet_mesh_as_obj(vertices, tetrahedra, filename):
    """`v x y z` lines, then 1-based `f a b c d` lines (the reference's format; repr of the float32 values, which parses back exactly)"""
    with open(filename, 'w') as f:
        f.write(''.join(f"v {p[0]} {p[1]} {p[2]}\n" for p in np.asarray(vertices)))
        if tetrahedra is not None:
            f.write(''.join("f %d %d %d %d\n" % tuple(t) for t in (np.asarray(tetrahedra) + 1).tolist()))
