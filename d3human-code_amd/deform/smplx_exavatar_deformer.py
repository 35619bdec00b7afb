"""SMPL-X driven deformer with the reference's interface (deform/smplx_exavatar_deformer.py: SMPLX_Deformer :21,
initialize :173, interpolate_weights :363, apply_lbs_inverse :385, lbs_forward :434), running on the HIP kernels of
csrc/lbs.hip through d3h.lbs.  `lbs_forward_batch` is the build's N-frame extension (the reference poses
every frame of a batch with idx[0]).

`k` (the reference's `self.k`, :40): the number of nearest template vertices whose skin-weight rows are blended by inverse distance
(:366-381), 1..32.  It is a plain attribute read at call time (`deformer.k = 4` works as in the reference); k = 1 is the reference's
setting and takes the single-neighbour kernels."""
import numpy as np
import torch
from d3h.devconst import const as _const

from d3h import lbs as HL
from .smplx_exavatar import SMPLX


def write_pc(path_mesh, v, vn=None, f=None):
    v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    with open(path_mesh, 'w') as fp:
        for p in v.reshape(-1, 3):
            fp.write('v %f %f %f\n' % tuple(p))
        if f is not None:
            f = f.detach().cpu().numpy() if torch.is_tensor(f) else np.asarray(f)
            for t in f.reshape(-1, 3) + 1:
                fp.write('f %d %d %d\n' % tuple(t))


class SMPLX_Deformer(object):
    def __init__(self, model_path='smplx', gender='neutral', model_dict=None, device='cuda', shape_param_dim=100,
                 expr_param_dim=50, k=1):
        self.shape_param_dim = shape_param_dim
        self.expr_param_dim = expr_param_dim
        self.model_path = model_path
        self.k = k
        self.device = device
        self.layer = SMPLX(model_path=model_path, gender=gender, num_betas=shape_param_dim,
                           num_expression_coeffs=expr_param_dim, model_dict=model_dict).to(device)
        self.lbs_weights = self.layer.lbs_weights.contiguous()
        self.vertex_num = self.layer.v_template.shape[0]
        self.face = self.layer.faces
        self.joint = {'num': 55}

    # deformer.py:173-238 -- canonical ("init") pose: zero except body_pose[2] = pi/36, body_pose[5] = -pi/36 (:178-180)
    def initialize(self, betas, pose=None, save_path=None):
        dev = self.device
        B = betas.shape[0]
        z = lambda n: torch.zeros(B, n, device=dev)
        body = z(63)
        body[:, 2] = torch.pi / 36
        body[:, 5] = -torch.pi / 36
        args = dict(global_orient=z(3), body_pose=body, jaw_pose=z(3), leye_pose=z(3), reye_pose=z(3), left_hand_pose=z(45),
                    right_hand_pose=z(45), expression=z(self.expr_param_dim))
        if pose is not None:
            for k in args:
                if k in pose:
                    args[k] = pose[k].to(dev)
        with torch.no_grad():
            output, A = self.layer(betas=betas.to(dev), transl=z(3), **args)
        self.vs_template = output.vertices
        self.f = self.layer.faces_tensor
        self.vertices = self.vs_template.float()
        self.init_A = A
        if save_path is not None:
            write_pc(save_path, self.vs_template[0], f=self.f)

    def nearest(self, pts):
        """nearest template vertex of every point (K=1 knn_points of :363-383); the template is fixed between initialize() calls, so
        its search grid is built once"""
        tmpl = self.vs_template[0]
        grid = getattr(self, '_knn_grid', None)
        if grid is None or not grid.matches(tmpl):
            grid = self._knn_grid = HL.KnnGrid(tmpl)
        k = self._k()
        if k > 1:                # the K nearest: HL.KnnResult(idx [P,K], d2 [P,K]), handed on to lbs_forward_batch(nn_idx=) as it is
            return HL.knnk(pts.reshape(-1, 3), tmpl, k, grid=grid)
        return HL.knn1(pts.reshape(-1, 3), tmpl, grid=grid)

    def _k(self):
        k = self.k
        if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= HL.K_MAX:
            raise ValueError(f'SMPLX_Deformer.k must be an int in 1..{HL.K_MAX}, got {k!r}')
        return k

    def interpolate_weights(self, pts):
        """[B,P,3] -> [B,P,J]; with K=1 the inverse-distance weight is exactly 1 (:367-370).  K > 1: the inverse-distance blend of the K
        nearest rows (:367-381), differentiable in pts (neighbours from the HIP search, the few blend operations in torch: this is the
        reference-interface accessor, the skinning itself blends inside its kernels)"""
        B, P, _ = pts.shape
        if self._k() > 1:
            tmpl = self.vs_template[0]
            idx = torch.stack([self.nearest(pts[b]).idx for b in range(B)]).long()                # [B,P,K]
            dist = torch.sqrt(((pts[:, :, None, :] - tmpl[idx]) ** 2).sum(-1) + 1e-9)
            w = 1.0 / (dist + 1e-9)
            w = w / w.sum(dim=2, keepdim=True)
            return (self.lbs_weights[idx] * w[..., None]).sum(dim=2)
        idx = torch.stack([self.nearest(pts[b]) for b in range(B)]).long()
        return self.lbs_weights[idx]

    def apply_lbs_inverse(self, pts, init_A, w_pts, Inverse=True):
        M = torch.einsum('bpj,bjmn->bpmn', w_pts, init_A)
        if Inverse:
            M = torch.inverse(M)
        ph = torch.cat([pts, torch.ones_like(pts[..., :1])], -1)[..., None]
        return (M @ ph)[..., :3, 0]

    def frame_transforms(self, smplx_param, idx_list):
        """A [B,55,4,4], trans [B,3] for the frames idx_list.  A is a pure function of (shape, expr, poses, offsets): when none of them
        requires grad (init stage: only `trans` is optimised, train.py:601-609) and none changed since the last call, the cached
        transforms are reused instead of re-running ~100 tiny kernels per iteration."""
        idx_list = [int(i) for i in idx_list]
        ii = _const(idx_list, self.device, torch.int64)

        def g(k, n):
            # frames 0..B-1 of a B-row tensor: the tensor itself (advanced indexing costs a sort-based index_put of ~8 launches in the
            # backward of `trans`); otherwise index_select, whose backward is one index_add
            t = smplx_param[k]
            if idx_list == list(range(t.shape[0])):
                return t.reshape(len(idx_list), n)
            return t.index_select(0, ii).reshape(len(idx_list), n)
        deps = [smplx_param[k] for k in ('shape', 'root_pose', 'body_pose', 'jaw_pose', 'expr', 'face_offset', 'joint_offset', 'locator_offset')
                if smplx_param.get(k) is not None]
        key = None
        if not any(t.requires_grad for t in deps):
            key = (tuple(idx_list), tuple((t.data_ptr(), t._version) for t in deps))
            hit = getattr(self, '_A_cache', None)
            if hit is not None and hit[0] == key and all(a is b for a, b in zip(hit[2], deps)):
                return hit[1], g('trans', 3)
        A = self.layer.transforms(smplx_param['shape'], g('root_pose', 3), g('body_pose', 63), g('jaw_pose', 3),
                                  g('expr', self.expr_param_dim), smplx_param.get('face_offset'), smplx_param.get('joint_offset'),
                                  smplx_param.get('locator_offset'))
        if key is not None:
            self._A_cache = (key, A.detach(), deps)      # the entry holds the tensors: their addresses cannot be re-used under the key
        return A, g('trans', 3)

    def lbs_forward_batch(self, pts, smplx_param, idx_list, nn_idx=None, transforms=None, pre=None):
        """pts [P,3] -> [B,P,3] for frames idx_list (one nearest-vertex search shared by all frames).  `transforms`: the (A, trans) of
        frame_transforms for these frames when the caller already has them; `pre`: the result computed ahead by lbs_forward_counted"""
        pts = pts.reshape(-1, 3)
        if nn_idx is None:
            nn_idx = self.nearest(pts)
        A, trans = transforms if transforms is not None else self.frame_transforms(smplx_param, idx_list)
        if isinstance(nn_idx, HL.KnnResult):
            return HL.lbs_points_k(pts, nn_idx, self.lbs_weights, self.vs_template[0], self.init_A[0], A, trans, pre=pre)
        return HL.lbs_points(pts, nn_idx, self.lbs_weights, self.init_A[0], A, trans, pre=pre)

    def nearest_counted(self, pts_cap, counts):
        """nearest() over the rows of a capacity buffer that the extraction's device-side counters say are real (d3h/mtets.py)"""
        tmpl = self.vs_template[0]
        grid = getattr(self, '_knn_grid', None)
        if grid is None or not grid.matches(tmpl):
            grid = self._knn_grid = HL.KnnGrid(tmpl)
        k = self._k()
        if k > 1:
            return grid.query_k_counted(pts_cap, counts, k)
        return grid.query_counted(pts_cap, counts)

    def lbs_forward_counted(self, pts_cap, counts, nn_idx_cap, transforms):
        A, trans = transforms
        if isinstance(nn_idx_cap, HL.KnnResult):
            return HL.lbs_points_k_counted(pts_cap, counts, nn_idx_cap, self.lbs_weights, self.vs_template[0], self.init_A[0], A, trans)
        return HL.lbs_points_counted(pts_cap, counts, nn_idx_cap, self.lbs_weights, self.init_A[0], A, trans)

    def lbs_forward(self, pts, smplx_param, idx, face=None):
        return self.lbs_forward_batch(pts.reshape(-1, 3), smplx_param, [int(idx)])[0]

    def lbs_forward_inverse(self, pts):
        w = self.interpolate_weights(pts)
        return self.apply_lbs_inverse(pts, self.init_A, w)
