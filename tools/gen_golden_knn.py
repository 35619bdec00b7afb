"""Generate tests/golden/lbs_knn.npz: the reference's SMPLX_Deformer with `k` in {2, 4} (K-nearest, inverse-distance blended skinning) on the
miniature body model and the inputs of tests/golden/lbs.npz (tools/gen_golden.py:gen_lbs).  Dev container only: the reference is imported at
run time through tools/refharness.py; only DATA is stored (the reference's outputs and gradients, and the neighbour ids it used).

Run: python tools/gen_golden_knn.py

The harness replaces knn_points by a float64 cdist + topk stand-in.  It and the float32 kernels pick the same neighbours as long as no
query has its K-th and (K+1)-th distances within rounding of each other: asserted here at 1e-6 relative (re-seed the points of gen_lbs if it
fires); the stored ids let the test check the neighbours exactly.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, ROOT)
import refharness                                     # noqa: E402
from gen_golden import synth, npy, GOLD               # noqa: E402  (the input generators, loaded by path: see gen_golden._load_by_path)

KS = (2, 4)


def main():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'lbs.npz'))
    m = synth.make_body_model(n_verts=512, seed=0, n_shape=10, n_expr=5)
    for k, v in m.items():                            # the very model of lbs.npz (which leaves posedirs out)
        assert k == 'posedirs' or np.array_equal(v, g['model.' + k]), k
    mt = {k: torch.from_numpy(v) for k, v in m.items()}
    T = lambda n: torch.from_numpy(g[n]).clone()
    betas, expr, jaw, hands, eyes = T('betas'), T('expr'), T('jaw'), T('hands'), T('eyes')
    pts, gw = T('pts'), T('gout')
    nfr = gw.shape[0]
    res = {}
    with refharness.ref_ctx():
        from deform.smplx_exavatar.lbs import lbs as ref_lbs
        from deform.smplx_exavatar_deformer import SMPLX_Deformer

        class Layer:
            """stands in for the licence-gated SMPL-X layer: full_pose assembled as body_models.py:1225-1257 does, then the REFERENCE lbs()"""
            lbs_weights = mt['weights']
            faces_tensor = None

            def forward(self, betas=None, global_orient=None, body_pose=None, jaw_pose=None, leye_pose=None, reye_pose=None,
                        left_hand_pose=None, right_hand_pose=None, expression=None, transl=None, face_offset=None,
                        joint_offset=None, locator_offset=None, pose2rot=True):
                fp = torch.cat([global_orient.reshape(-1, 1, 3), body_pose.reshape(-1, 21, 3), jaw_pose.reshape(-1, 1, 3),
                                leye_pose.reshape(-1, 1, 3), reye_pose.reshape(-1, 1, 3), left_hand_pose.reshape(-1, 15, 3),
                                right_hand_pose.reshape(-1, 15, 3)], dim=1).reshape(-1, 165)
                fp[:, 69:].zero_()
                comp = torch.cat([betas, expression], dim=-1)
                dirs = torch.cat([mt['shapedirs'], mt['expr_dirs']], dim=-1)
                vt = mt['v_template'] if face_offset is None else mt['v_template'] + face_offset
                verts, joints, A = ref_lbs(comp, fp, vt, dirs, mt['posedirs'], mt['J_regressor'], joint_offset, locator_offset,
                                           mt['parents'], mt['weights'], pose2rot=True)
                return SimpleNamespace(vertices=verts + transl[:, None]), A
            __call__ = forward

        d = object.__new__(SMPLX_Deformer)
        d.layer = Layer(); d.lbs_weights = mt['weights']; d.expr_param_dim = 5; d.shape_param_dim = 10
        bp0 = torch.zeros(1, 63); bp0[:, 2] = torch.pi / 36; bp0[:, 5] = -torch.pi / 36
        z = lambda n: torch.zeros(1, n)
        out0, A0 = d.layer(betas=betas, global_orient=z(3), body_pose=bp0, jaw_pose=z(3), leye_pose=z(3), reye_pose=z(3),
                           left_hand_pose=z(45), right_hand_pose=z(45), expression=z(5), transl=z(3))
        d.vs_template = out0.vertices; d.init_A = A0
        assert np.array_equal(out0.vertices[0].numpy(), g['tmpl']) and np.array_equal(A0[0].numpy(), g['A0'])
        d2 = torch.cdist(pts.double(), out0.vertices[0].double()).pow(2).sort(dim=1).values
        for K in KS:
            gap = ((d2[:, K] - d2[:, K - 1]) / d2[:, K]).min().item()
            assert gap > 1e-6, f'K={K}: the K-th and (K+1)-th neighbour of a query are {gap:.2e} (relative) apart: re-seed the points'
            d.k = K
            param = {'shape': betas, 'face_offset': T('face_offset'), 'joint_offset': T('joint_offset'), 'locator_offset': T('locator_offset'),
                     'trans': T('trans').requires_grad_(True), 'rhand_pose': hands[:, 1], 'lhand_pose': hands[:, 0], 'jaw_pose': jaw,
                     'expr': expr, 'body_pose': T('body_pose').requires_grad_(True), 'root_pose': T('root_pose').requires_grad_(True),
                     'leye_pose': eyes[:, 0], 'reye_pose': eyes[:, 1]}
            p_in = pts.clone().requires_grad_(True)
            outs, loss = [], 0
            for f in range(nfr):
                o = d.lbs_forward(p_in.reshape(1, -1, 3), param, idx=f)
                outs.append(o.detach())
                loss = loss + (o * gw[f]).sum()
            loss.backward()
            with torch.no_grad():
                w_pts = d.interpolate_weights(pts.reshape(1, -1, 3))
                can = d.apply_lbs_inverse(pts.reshape(1, -1, 3), A0, w_pts)
                idx = sys.modules['pytorch3d.ops'].knn_points(pts[None], out0.vertices, K=K).idx[0]
            res.update({f'k{K}.idx': idx.to(torch.int32), f'k{K}.w_pts': w_pts[0], f'k{K}.canonical': can[0], f'k{K}.out': torch.stack(outs),
                        f'k{K}.d_pts': p_in.grad, f'k{K}.d_trans': param['trans'].grad, f'k{K}.d_body_pose': param['body_pose'].grad,
                        f'k{K}.d_root_pose': param['root_pose'].grad})
            print(f'lbs_knn: k = {K}: smallest relative gap between the K-th and (K+1)-th distance {gap:.2e}')
    out = os.path.join(GOLD, 'lbs_knn.npz')
    np.savez_compressed(out, **npy(res))
    print('wrote', out, os.path.getsize(out), 'bytes (lbs.npz:', os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'lbs.npz')), 'bytes)')


if __name__ == '__main__':
    main()
