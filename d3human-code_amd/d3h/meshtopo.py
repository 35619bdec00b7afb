"""Host side of csrc/meshtopo.hip: mesh topology for the hand-off between the training stages (the reference's script/connet_face_head.py and the
open-edge helpers of script/process_body_cloth_head_msdfcut.py:92-102,151-156).  Tensors live on the device the kernels run on; faces are [F,3]
int32 or int64, positions [n,3] float32 or float64 (compared in the type given).

    connected_components(faces, nv) -> labels int32 [nv]
        labels[v] = the smallest vertex index of v's component (edges (0,1) and (1,2) of every face); an isolated vertex is its own label; a face
        with repeated indices is legal; deterministic
    rank_components(labels) -> (ranked_labels int64 [c], sizes int64 [c])
        the reference's filter_and_sort_components: components of one vertex dropped, the rest by size descending, ties to the smaller label
    faces_by_component(faces, labels, ranked_labels) -> faces [k,3]
        the faces of the ranked components, grouped in rank order, file order kept inside a group (a face's vertices always share a component)
    weld(v, table_log2=0) -> (keep int64 [m], new_index int64 [n])
        rows with equal coordinates (-0 == +0; a row with a NaN equals nothing) collapse onto their first occurrence; keep = the first occurrences,
        ascending (open3d's remove_duplicated_vertices order), v[keep][new_index] == v for every row without a NaN.  table_log2 = 0: a table of the
        smallest power of two >= 2 n slots; any other value is taken if 2^table_log2 > n, else the call fails
    remove_degenerate(faces) -> faces without the rows that have two equal indices
    merge_and_repair(v1, f1, v2, f2) -> (v, f): stack, weld, remap, drop degenerates; unreferenced vertices stay, as in open3d
    open_vertices(faces, nv) -> int64 [k], ascending: the ends of the (min, max) edges that exactly one face side uses -- counted literally, so a
        face (a,a,b) gives (a,a) once and (a,b) twice; an edge of three or more faces is not open
    peel_open_faces(faces, nv, rounds=1) -> faces: `rounds` times, drop every face that touches an open vertex

Each call that launches kernels reads its error word (or a count) back once: that is its one synchronisation.  A face index outside [0, nv)
raises; so does a table that cannot be built."""
import torch

from . import _lib as L

ERR_RANGE, ERR_CAP, ERR_TABLE = 1, 2, 4


def _faces(faces, what):
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise RuntimeError(f'{what}: expected faces [F,3] int32 or int64, got {tuple(faces.shape)} {faces.dtype}')
    return faces.contiguous()


def _raise(word, what):
    if word:
        why = [t for b, t in ((ERR_RANGE, 'a face index outside [0, nv)'), (ERR_CAP, 'an iteration cap was reached'),
                              (ERR_TABLE, 'a probe went round the whole hash table')) if word & b]
        raise RuntimeError(f'{what}: ' + '; '.join(why))


def _table_log2(items, table_log2, what):
    lg = L.query('topo_table_log2', items, table_log2)
    if lg < 0:
        raise RuntimeError(f'd3h: {what} failed with code {lg} (bad argument): 2^{table_log2} slots cannot hold {items} keys')
    return lg


def connected_components(faces, nv):
    f = _faces(faces, 'connected_components')
    nv = int(nv)
    dev = f.device
    parent = torch.empty(nv, dtype=torch.int32, device=dev)
    label = torch.empty(nv, dtype=torch.int32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    L.call('cc_init', parent, nv, err)
    L.call('cc_hook', f, f.dtype == torch.int64, f.shape[0], parent, nv, err)
    L.call('cc_flatten', parent, nv, label, err)
    _raise(int(err.item()), 'connected_components')
    return label


def rank_components(labels):
    roots, sizes = torch.unique(labels.long(), return_counts=True)         # roots ascending
    many = sizes > 1
    roots, sizes = roots[many], sizes[many]
    sizes, order = torch.sort(sizes, descending=True, stable=True)
    return roots[order], sizes


def faces_by_component(faces, labels, ranked_labels):
    f = _faces(faces, 'faces_by_component')
    if f.shape[0] == 0 or ranked_labels.numel() == 0:
        return f[:0]
    rank_of = torch.full((labels.shape[0],), -1, dtype=torch.int64, device=f.device)
    rank_of[ranked_labels.long()] = torch.arange(ranked_labels.numel(), device=f.device)
    r = rank_of[labels.long()[f[:, 0].long()]]
    sel = torch.nonzero(r >= 0).reshape(-1)
    return f[sel[torch.sort(r[sel], stable=True)[1]]]


def weld_representatives(v, table_log2=0):
    """-> rep int32 [n]: the lowest index with row i's coordinates"""
    if v.dim() != 2 or v.shape[1] != 3 or v.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f'weld: expected positions [n,3] float32 or float64, got {tuple(v.shape)} {v.dtype}')
    v = v.detach().contiguous()
    n, dev = int(v.shape[0]), v.device
    lg = _table_log2(n, table_log2, 'weld_insert')
    table = torch.empty(1 << lg, dtype=torch.int32, device=dev)
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    f64 = v.dtype == torch.float64
    L.call('weld_insert', v, f64, n, table, table_log2, err)
    L.call('weld_lookup', v, f64, n, table, table_log2, rep, err)
    _raise(int(err.item()), 'weld')
    return rep


def weld(v, table_log2=0):
    rep = weld_representatives(v, table_log2).long()
    first = rep == torch.arange(rep.shape[0], device=rep.device)
    keep = torch.nonzero(first).reshape(-1)
    new_index = (torch.cumsum(first, 0) - 1)[rep]
    return keep, new_index


def remove_degenerate(faces):
    f = _faces(faces, 'remove_degenerate')
    return f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]


def merge_and_repair(v1, f1, v2, f2):
    v = torch.cat([v1, v2.to(v1.dtype)])
    f = torch.cat([_faces(f1, 'merge_and_repair').long(), _faces(f2, 'merge_and_repair').long() + v1.shape[0]])
    keep, new_index = weld(v)
    return v[keep], remove_degenerate(new_index[f])


def open_vertex_mask(faces, nv, table_log2=0):
    """-> uint8 [nv]: 1 at the ends of the edges that exactly one face side uses"""
    f = _faces(faces, 'open_vertices')
    nv, nf, dev = int(nv), int(f.shape[0]), f.device
    lg = _table_log2(3 * nf, table_log2, 'edge_count')
    keys = torch.empty(1 << lg, dtype=torch.int64, device=dev)
    counts = torch.empty(1 << lg, dtype=torch.int32, device=dev)
    mask = torch.empty(nv, dtype=torch.uint8, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call('edge_count', f, f.dtype == torch.int64, nf, nv, keys, counts, table_log2, err)
    L.call('open_vertex_mask', keys, counts, lg, nv, mask)
    _raise(int(err.item()), 'open_vertices')
    return mask


def open_vertices(faces, nv):
    return torch.nonzero(open_vertex_mask(faces, nv)).reshape(-1)


def peel_open_faces(faces, nv, rounds=1):
    f = _faces(faces, 'peel_open_faces')
    for _ in range(int(rounds)):
        mask = open_vertex_mask(f, nv).bool()
        f = f[~mask[f.long()].any(dim=1)]
    return f
