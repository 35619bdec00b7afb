"""bench.py --dump-outputs: what the timed step computed in its last call (losses, updated parameters, their gradients) as .npy files,
float32 / float64 only, DUMP_LIMIT_BYTES in all (larger arrays keep a fixed, seeded sample).  On the host emulation of the kernels."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(ROOT, 'bench.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_step_outputs_of_init_and_split_steps(emul, tmp_path):
    import torch
    from d3h.scene import Scene
    B = _bench()
    ell = lambda x: (((x - torch.tensor([0.0, -0.4, 0.0])) / torch.tensor([0.55, 0.8, 0.45])).norm(dim=-1) - 1.0) * 0.4
    sc = Scene(res=24, grid_n=4, n_frames=1, device='cpu', prefit_steps=60, loss_set='full', body_verts=300, sdf_fn=ell,
               flags_hook=lambda F: (setattr(F, 'prefit_with_library_path', True), setattr(F, 'use_eikonal', False)))
    r = sc.step()
    out = B.step_outputs(sc)
    assert {f'loss.{k}' for k in r} <= set(out)
    for n in ('geometry.deform', 'geometry.sdf_net.net.0.weight', 'material.encoder.params', 'flags.trans_optim'):
        assert f'param.{n}' in out and f'grad.{n}' in out, n
    assert np.array_equal(out['param.geometry.deform'], sc.geometry.deform.detach().numpy())
    assert np.array_equal(out['grad.flags.trans_optim'], sc.FLAGS.trans_optim.grad.numpy())
    assert float(out['loss.total']) == float(r['total'])
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    B.dump_outputs(out, str(tmp_path / 'init'))
    got = _load(tmp_path / 'init')
    assert sorted(got) == sorted(out) and all(np.array_equal(got[k], out[k]) for k in out)
    # the split stage optimises msdf (and not the SDF network)
    sc._build_optimizers('split', warmup_iter=300)
    sc.step_split()
    out = B.step_outputs(sc)
    assert 'param.geometry.msdf' in out and 'grad.geometry.msdf' in out and 'loss.cloth_msk_loss' in out
    assert 'param.geometry.sdf_net.net.0.weight' not in out


def test_dump_stays_within_the_limit_with_a_seeded_sample(tmp_path, monkeypatch):
    B = _bench()
    rng = np.random.default_rng(3)
    arrays = {'param.big': rng.standard_normal((500, 300)).astype(np.float32), 'grad.big': rng.standard_normal(90000),
              'loss.total': np.float32(1.5)}
    monkeypatch.setattr(B, 'DUMP_LIMIT_BYTES', 300000)
    B.dump_outputs(arrays, str(tmp_path / 'a'))
    B.dump_outputs(arrays, str(tmp_path / 'b'))
    a, b = _load(tmp_path / 'a'), _load(tmp_path / 'b')
    assert sum(os.path.getsize(os.path.join(tmp_path, 'a', f)) - 128 for f in os.listdir(tmp_path / 'a')) <= 300000
    assert sorted(a) == sorted(arrays) and all(np.array_equal(a[k], b[k]) for k in a)
    assert a['param.big'].size == 100000 // 4 and np.isin(a['param.big'], arrays['param.big']).all()
    assert a['grad.big'].dtype == np.float64 and a['grad.big'].size == 100000 // 8
    assert float(a['loss.total']) == 1.5
    small = arrays['param.big'][:100]
    B.dump_outputs({'param.small': small}, str(tmp_path / 'c'))          # under the limit: written whole, shape kept
    assert np.array_equal(np.load(tmp_path / 'c' / 'param.small.npy'), small)
