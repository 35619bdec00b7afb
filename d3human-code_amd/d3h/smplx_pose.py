"""SMPL-X pose -> per-joint skinning transforms A[B,55,4,4] (the only SMPL-X output the hot path consumes,
deform/smplx_exavatar_deformer.py:456,476).

Follows deform/smplx_exavatar/lbs.py (joints :216-224, batch_rodrigues :311-347, batch_rigid_transform :361-413) and the
full-pose assembly of body_models.py:1225-1257, but walks the kinematic tree level by level (all joints of one depth in
one batched matmul: 10 steps instead of the reference's 54 sequential 4x4 products) and skips the vertex skinning /
landmark code whose results the reference discards.  Differentiable through torch autograd (tiny tensors: plumbing).
"""
import torch
import torch.nn.functional as F


def rodrigues(rv):
    """axis-angle [N,3] -> rotation matrices [N,3,3] (lbs.py:311-347, incl. the +1e-8 inside the norm)"""
    angle = torch.norm(rv + 1e-8, dim=1, keepdim=True)
    axis = rv / angle
    s, c = torch.sin(angle)[..., None], torch.cos(angle)[..., None]
    x, y, z = axis[:, 0], axis[:, 1], axis[:, 2]
    o = torch.zeros_like(x)
    K = torch.stack([o, -z, y, z, o, -x, -y, x, o], 1).view(-1, 3, 3)
    return torch.eye(3, dtype=rv.dtype, device=rv.device)[None] + s * K + (1 - c) * (K @ K)


class KinematicTree:
    def __init__(self, parents):
        parents = [int(p) for p in parents]
        self.parents = parents
        depth = [0] * len(parents)
        for j in range(1, len(parents)):
            depth[j] = depth[parents[j]] + 1
        self.levels = []
        for d in range(1, max(depth) + 1):
            js = [j for j in range(len(parents)) if depth[j] == d]
            self.levels.append((js, [parents[j] for j in js]))

    def transforms(self, rot, joints):
        """rot [B,J,3,3], joints [B,J,3] -> A [B,J,4,4] = G_j with the rest joint subtracted (lbs.py:407-411)"""
        B, J = joints.shape[:2]
        par = torch.as_tensor(self.parents[1:], device=joints.device)
        rel = torch.cat([joints[:, :1], joints[:, 1:] - joints[:, par]], 1)
        T = torch.cat([torch.cat([rot, rel[..., None]], -1),
                       torch.tensor([0., 0., 0., 1.], dtype=rot.dtype, device=rot.device).expand(B, J, 1, 4)], -2)
        G = [None] * J
        G[0] = T[:, 0]
        for js, ps in self.levels:
            Gp = torch.stack([G[p] for p in ps], 1)
            Gc = Gp @ T[:, js]
            for k, j in enumerate(js):
                G[j] = Gc[:, k]
        G = torch.stack(G, 1)
        t = G[..., :3, 3] - (G[..., :3, :3] @ joints[..., None])[..., 0]
        return torch.cat([torch.cat([G[..., :3, :3], t[..., None]], -1), G[..., 3:, :]], -2)


def assemble_full_pose(root, body, jaw, leye, reye, lhand, rhand):
    B = body.reshape(-1, 63).shape[0]
    fp = torch.cat([root.reshape(B, 3), body.reshape(B, 63), jaw.reshape(B, 3)], 1)
    # body_models.py:1255 zeroes entries >= 69 (eyes + both hands): they never influence A
    return torch.cat([fp, fp.new_zeros(B, 165 - 69)], 1)


class _PoseFn(torch.autograd.Function):
    """(full pose [B,J,3], rest joints [B or 1,J,3]) -> A [B,J,4,4] on the single-launch kernels of csrc/smplx_pose.hip"""

    @staticmethod
    def forward(ctx, fp, joints, parents32):
        from . import _lib as L
        fpc, jc = fp.contiguous().float(), joints.contiguous().float()
        B, J = fpc.shape[0], fpc.shape[1]
        A = torch.empty(B, J, 4, 4, dtype=torch.float32, device=fp.device)
        G = torch.empty(B, J, 12, dtype=torch.float32, device=fp.device)
        jbs = 0 if jc.shape[0] == 1 else J * 3
        L.call('smplx_pose_fwd', fpc, jc, jbs, parents32, J, B, A, G)
        ctx.save_for_backward(fpc, jc, parents32, G)
        ctx.jshape = joints.shape
        return A

    @staticmethod
    def backward(ctx, dA):
        from . import _lib as L
        fpc, jc, parents32, G = ctx.saved_tensors
        B, J = fpc.shape[0], fpc.shape[1]
        d_fp = torch.empty_like(fpc)
        d_J = torch.empty(B, J, 3, dtype=torch.float32, device=fpc.device) if ctx.needs_input_grad[1] else None
        jbs = 0 if jc.shape[0] == 1 else J * 3
        L.call('smplx_pose_bwd', fpc, jc, jbs, parents32, J, B, G, dA.contiguous().float(), d_fp, d_J)
        if d_J is not None and tuple(d_J.shape) != tuple(ctx.jshape):
            d_J = d_J.sum_to_size(ctx.jshape)
        return d_fp, d_J, None


NJ_MAX = 64       # NJ_MAX of csrc/smplx_pose.hip


def check_tree(parents):
    """parents of a kinematic tree as host values (a list, or a tensor: read back): 0 <= parents[j] < j for every j >= 1 (parents[0] is
    ignored).  The backward folds the tree level by level from the leaves and relies on every ancestor walk ending at joint 0"""
    p = [int(v) for v in (parents.tolist() if torch.is_tensor(parents) else parents)]
    bad = [j for j in range(1, len(p)) if not 0 <= p[j] < j]
    if bad:
        raise ValueError(f'd3h pose_transforms: parents[j] must lie in 0..j-1 for every j >= 1; joint {bad[0]} has parent {p[bad[0]]}')


def pose_transforms(full_pose, joints, parents32, tree_checked=False):
    """full_pose [B,165] (or [B,55,3]) axis-angle, joints [B or 1,55,3] -> A [B,55,4,4] (lbs.py:311-413), one kernel launch.  Any tree of
    1..64 joints: full_pose [B,3 nj] or [B,nj,3], joints [B or 1,nj,3], parents32 int32 [nj] on the device with parents[j] < j.  The values
    of parents32 are read back and checked on every call (a host sync) unless `tree_checked`: the caller has run check_tree on the values
    this tensor was built from (the body model does, once, when it is constructed)"""
    if full_pose.dim() not in (2, 3) or full_pose.shape[-1] % 3 != 0 or (full_pose.dim() == 3 and full_pose.shape[2] != 3):
        raise RuntimeError(f'd3h pose_transforms: the pose must be [B,3 J] or [B,J,3], got {tuple(full_pose.shape)}')
    B = full_pose.shape[0]
    nj = full_pose.shape[1] if full_pose.dim() == 3 else full_pose.shape[1] // 3
    if not 1 <= nj <= NJ_MAX:
        raise RuntimeError(f'd3h pose_transforms: {nj} joints, the kernels hold 1..{NJ_MAX}')
    if joints.dim() != 3 or joints.shape[0] not in (1, B) or tuple(joints.shape[1:]) != (nj, 3) or joints.device != full_pose.device:
        raise RuntimeError(f'd3h pose_transforms: the rest joints must be [{B} or 1, {nj}, 3] on the device of the pose, got {tuple(joints.shape)}')
    if not torch.is_tensor(parents32) or parents32.dtype != torch.int32 or tuple(parents32.shape) != (nj,) or not parents32.is_contiguous() or \
            parents32.device != full_pose.device:
        raise RuntimeError(f'd3h pose_transforms: parents must be a contiguous int32 tensor of shape {(nj,)} on {full_pose.device}, got '
                           f'{tuple(parents32.shape) if torch.is_tensor(parents32) else type(parents32).__name__} '
                           f'{getattr(parents32, "dtype", "")} on {getattr(parents32, "device", "")}')
    if not tree_checked:
        check_tree(parents32)
    return _PoseFn.apply(full_pose.reshape(B, nj, 3), joints, parents32)
