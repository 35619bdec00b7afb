"""Shim under the third-party name so `import tinycudann as tcnn` (render/mlptexture.py:11) resolves to the project's HIP kernels.

tcnn.Encoding(n_input_dims, encoding_config) with .params / .n_input_dims / .n_output_dims / forward, and free_temporary_memory().
  * the reference's configuration (render/mlptexture.py:68-75: 3-D HashGrid, 5 levels x 2 features, base 16, its per-level scale, a table
    large enough that every level is dense) runs on csrc/texmlp.hip, as it always has (`cfg is None`);
  * every other HashGrid / DenseGrid / Grid configuration runs on the general encoding of csrc/gridenc.hip (`cfg` = its
    d3h.gridenc.GridConfig; the accepted keys, their defaults and the semantics are in the docstring of d3h/gridenc.py).
The output is float32 (tcnn's default is half precision: a documented deviation); features are initialised U(-1e-4, 1e-4) from `seed`.

tcnn.Network(n_input_dims, n_output_dims, network_config) with .params / .n_input_dims / .n_output_dims / forward: the fused bias-free MLP of
csrc/fusedmlp.hip ("FullyFusedMLP" and "CutlassMLP" run the same kernels; the accepted keys, their defaults and the semantics are in the
docstring of d3h/fusedmlp.py).  `.params` is ONE flat float32 Parameter: the matrices in layer order, each [fan_out][fan_in] with its exact
shape, Xavier-uniform per matrix from `seed` (tcnn pads the first fan-in and the last fan-out to 16 inside its vector and returns half
precision: documented deviations).
tcnn.NetworkWithInputEncoding(n_input_dims, n_output_dims, encoding_config, network_config): ONE flat `.params`, the network's first, then
the encoding's table (tcnn's order, restated from memory); with the same `seed` it equals cat(Network(...).params, Encoding(...).params).
forward is the encoding (csrc/texmlp.hip's for the reference configuration, csrc/gridenc.hip's otherwise) followed by the fused MLP, both
reading views of `.params`."""
import torch

from d3h import texmlp as _T
from d3h import gridenc as _G
from d3h import fusedmlp as _F


class Encoding(torch.nn.Module):
    def __init__(self, n_input_dims, encoding_config, dtype=None, seed=1337):
        super().__init__()
        c = encoding_config
        ref = (n_input_dims == 3 and c.get('otype') == 'HashGrid' and c.get('n_levels') == 5 and c.get('n_features_per_level') == 2
               and c.get('base_resolution') == 16 and abs(c.get('per_level_scale', 2.0) - _T.PER_LEVEL_SCALE) < 1e-9
               and c.get('log2_hashmap_size', 21) >= 19 and c.get('type', 'Hash') == 'Hash' and c.get('interpolation', 'Linear') == 'Linear')
        self.cfg = None if ref else _G.GridConfig(n_input_dims, c)
        self.n_input_dims = n_input_dims
        self.n_output_dims = _T.ENC_DIMS if ref else self.cfg.n_output_dims
        dev = 'cuda' if torch.cuda.is_available() else 'cpu'
        g = torch.Generator().manual_seed(seed)
        n = _T.grid_param_count() if ref else self.cfg.n_params
        # tcnn initialises grid features U(-1e-4, 1e-4)
        self.params = torch.nn.Parameter(((torch.rand(n, generator=g) * 2 - 1) * 1e-4).to(dev))

    def forward(self, x):
        if self.cfg is None:
            return _T.grid_encode(x, self.params)
        return _G.grid_encode(x, self.params, self.cfg)


def _xavier(cfg, seed):
    """the matrices of `cfg` in layer order, flattened: Xavier-uniform U(-b, b), b = sqrt(6 / (fan_in + fan_out)), from `seed`"""
    g = torch.Generator().manual_seed(seed)
    return torch.cat([((torch.rand(fo * fi, generator=g) * 2 - 1) * (6.0 / (fi + fo)) ** 0.5) for fo, fi in cfg.shapes])


def _matrices(cfg, flat):
    out, off = [], 0
    for fo, fi in cfg.shapes:
        out.append(flat[off:off + fo * fi].view(fo, fi))
        off += fo * fi
    return out


class Network(torch.nn.Module):
    def __init__(self, n_input_dims, n_output_dims, network_config, seed=1337):
        super().__init__()
        self.cfg = _F.MLPConfig(n_input_dims, n_output_dims, network_config)
        self.n_input_dims, self.n_output_dims = self.cfg.n_input_dims, self.cfg.n_output_dims
        dev = 'cuda' if torch.cuda.is_available() else 'cpu'
        self.params = torch.nn.Parameter(_xavier(self.cfg, seed).to(dev))

    def forward(self, x):
        return _F.fused_mlp(x, _matrices(self.cfg, self.params), self.cfg)


class NetworkWithInputEncoding(torch.nn.Module):
    def __init__(self, n_input_dims, n_output_dims, encoding_config, network_config, seed=1337):
        super().__init__()
        enc = Encoding(n_input_dims, encoding_config, seed=seed)
        self.enc_cfg, self.n_enc_dims = enc.cfg, enc.n_output_dims
        self.cfg = _F.MLPConfig(enc.n_output_dims, n_output_dims, network_config)
        self.n_input_dims, self.n_output_dims = n_input_dims, self.cfg.n_output_dims
        dev = enc.params.device
        self.params = torch.nn.Parameter(torch.cat([_xavier(self.cfg, seed).to(dev), enc.params.detach()]))

    def forward(self, x):
        table = self.params[self.cfg.n_params:]
        e = _T.grid_encode(x, table) if self.enc_cfg is None else _G.grid_encode(x, table, self.enc_cfg)
        return _F.fused_mlp(e, _matrices(self.cfg, self.params[:self.cfg.n_params]), self.cfg)


def free_temporary_memory():
    pass
