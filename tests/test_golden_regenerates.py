"""The oracle package and the one fixture not taken from the upstream project's outputs (tests/golden/parity_state_sdf.npz).
(Regenerating the other fixtures needs a checkout of that project: tools/gen_golden.py asserts oracle == upstream on their inputs.)"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def test_oracle_package_never_imports_the_product():
    """oracle/ is the checker: importing it (its own MobileNet-shaped trunk included) must pull in neither d3h nor any product module"""
    code = ("import sys; sys.path.insert(0, %r); import oracle.tick, oracle.parity, oracle.render, oracle.raster, oracle.texmlp, oracle.seq_ops, oracle.perceptual as m; "
            "import torch; t = m.MobileNetPerceptualLoss(use_gpu=False, seed=1); x = torch.rand(1, 3, 32, 32); t(x, torch.rand(1, 3, 32, 32)); "
            "bad = [k for k in sys.modules if k == 'd3h' or k.startswith('d3h.') or k.startswith('geometry') or k.startswith('render')]; assert not bad, bad") % (
        ROOT,)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd='/tmp',
                       env={k: v for k, v in os.environ.items() if k != 'PYTHONPATH'})
    assert r.returncode == 0, r.stderr[-2000:]


def test_parity_state_fixture_is_a_fitted_body():
    """tests/golden/parity_state_sdf.npz (tools/gen_parity_state.py): the reference's network shape, finite, and -- through the oracle's
    restatement of the network -- the analytic capsule humanoid to the rmse the generator recorded"""
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'd3human-code_amd'))
    from oracle import sdf_mlp as O
    from d3h import synth
    g = np.load(os.path.join(GOLD, 'parity_state_sdf.npz'))
    want = {0: (256, 39), 2: (256, 256), 4: (256, 256), 6: (256, 256), 8: (256, 295), 10: (256, 256), 12: (256, 256), 14: (1, 256)}
    sd = {}
    for i, shp in want.items():
        assert g[f'net.{i}.weight'].shape == shp and g[f'net.{i}.bias'].shape == (shp[0],) and g[f'net.{i}.weight'].dtype == np.float32
        assert np.isfinite(g[f'net.{i}.weight']).all()
        sd[f'net.{i}.weight'], sd[f'net.{i}.bias'] = torch.from_numpy(g[f'net.{i}.weight']), torch.from_numpy(g[f'net.{i}.bias'])
    v, _ = synth.kuhn_grid(24)
    v = torch.from_numpy(v)
    with torch.no_grad():
        err = O.mlp_forward(v, sd).reshape(-1) - synth.body_sdf(v)
    assert float(err.pow(2).mean().sqrt()) < 2.0 * float(g['fit_rmse']) + 1e-3
