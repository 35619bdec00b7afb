"""MLPTexture3D with the reference's interface (render/mlptexture.py:51-115): `.encoder.params`, `.net.net.{0,2,4}.weight`,
`.sample(texc, frame_id)`.  For the reference's shape (its grid, 10 -> 32 -> 32 -> 6) sample() runs the fused grid-encoding + MLP kernel
(csrc/texmlp.hip, `fused`); with another `enc_cfg` or another `channels` / `internal_dims` / `hidden` it is the composed path of the
reference itself (:91-107): box normalisation + clamp, `self.encoder` (csrc/gridenc.hip through the tinycudann shim), then
  * `fused_net` (D3H_TEX_FUSED_NET=1 in the environment when the texture is constructed; not the default, see FUSED_NET_DEFAULT): ONE
    call of the general fused MLP (csrc/fusedmlp.hip through d3h.fusedmlp.fused_mlp) on the nn.Linear weights themselves,
    which does the x128 input-gradient scale of _MLP (:31), the network, the sigmoid range map and the mask, and keeps no activation for
    the backward -- every network shape the kernels are built for (d3h.fusedmlp.supported);
  * otherwise (the default; always for e.g. `internal_dims=48`; D3H_TEX_FUSED_NET=0 says so explicitly), the same steps op by op: _ScaleGrad,
    `self.net` through the library GEMMs, the sigmoid range map, the mask."""
import os

import numpy as np
import torch
import tinycudann as tcnn

from d3h import texmlp as _T
from d3h import fusedmlp as _F


# what D3H_TEX_FUSED_NET is taken to be when it is not set ('1': the general fused MLP, '0': the library GEMMs).  The fused network
# becomes the default only by measurement (tools/gpu_probe_fusedmlp.py: forward + backward faster than the library composition by more than
# the run-to-run spread, and a lower peak of allocated memory); profiles/fusedmlp_probe.md does not exist yet, so it is opt-in.
FUSED_NET_DEFAULT = '0'


class _MLP(torch.nn.Module):
    def __init__(self, cfg, loss_scale=1.0):
        super().__init__()
        self.loss_scale = loss_scale
        net = (torch.nn.Linear(cfg['n_input_dims'], cfg['n_neurons'], bias=False), torch.nn.ReLU())
        for _ in range(cfg['n_hidden_layers'] - 1):
            net = net + (torch.nn.Linear(cfg['n_neurons'], cfg['n_neurons'], bias=False), torch.nn.ReLU())
        net = net + (torch.nn.Linear(cfg['n_neurons'], cfg['n_output_dims'], bias=False),)
        self.net = torch.nn.Sequential(*net)
        for m in self.net:
            if isinstance(m, torch.nn.Linear):
                torch.nn.init.kaiming_uniform_(m.weight, nonlinearity='relu')     # mlptexture.py:36-41

    def forward(self, x):
        # library-GEMM path (only used when someone calls the sub-module directly; sample() uses the fused kernel)
        y = self.net(x.to(torch.float32))
        return y


class _ScaleGrad(torch.autograd.Function):
    """identity whose gradient is multiplied by `s`: the register_full_backward_hook of the reference's _MLP (mlptexture.py:31)"""

    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


class MLPTexture3D(torch.nn.Module):
    # mlptexture.py:94: hard-coded, sign-flipped box; AABB and frame_id are ignored by the reference -- kept literally
    BBOX = (0.6, 0.6, 0.2, -0.8, -1.2, -0.2)

    def __init__(self, AABB, channels=3, internal_dims=32, hidden=2, min_max=None, use_float16=False, enc_cfg=None):
        super().__init__()
        self.channels, self.internal_dims, self.AABB, self.min_max, self.use_float16 = channels, internal_dims, AABB, min_max, use_float16
        per_level_scale = np.exp(np.log(4096 / 16) / (16 - 1))
        if enc_cfg is None:
            enc_cfg = {"otype": "HashGrid", "n_levels": 5, "n_features_per_level": 2, "log2_hashmap_size": 21, "base_resolution": 16,
                       "per_level_scale": per_level_scale}
        self.encoder = tcnn.Encoding(3, enc_cfg)
        self.net = _MLP({"n_input_dims": self.encoder.n_output_dims, "n_output_dims": channels, "n_hidden_layers": hidden,
                         "n_neurons": internal_dims}, 128.0)
        dev = self.encoder.params.device
        self.net.to(dev)
        # the fused kernel is built for the reference's grid and the shape 10 -> 32 -> 32 -> 6; everything else is composed (see sample())
        self.fused = self.encoder.cfg is None and channels == 6 and internal_dims == 32 and hidden == 2
        # the composed path runs its network on the general fused MLP when asked to and the kernels are built for the shape
        self.fused_net = (not self.fused and os.environ.get('D3H_TEX_FUSED_NET', FUSED_NET_DEFAULT) != '0'
                          and _F.supported(self.encoder.n_output_dims, channels, internal_dims, hidden))
        self.net_cfg = _F.MLPConfig(self.encoder.n_output_dims, channels, {'otype': 'FullyFusedMLP', 'activation': 'ReLU', 'output_activation': 'Sigmoid',
                                                                            'n_neurons': internal_dims, 'n_hidden_layers': hidden}) if self.fused_net else None

    def _range_host(self):
        """host copy of the output range (HOST arguments of the C ABI).  Read back once per value: a `.cpu()` here is a stream
        synchronisation in the middle of every render otherwise, after which the rest of the forward is launch-bound."""
        mm = self.min_max
        lo, hi = mm[0], mm[1]                                           # a [2,C] tensor or a pair of tensors / lists
        key = tuple((t.data_ptr(), t._version) if torch.is_tensor(t) else None for t in (lo, hi))
        # the entry holds what owns the memory behind the key (the [2,C] tensor, or the two tensors of a pair), so that an address in the
        # key cannot be handed to another tensor while the entry lives
        own = (mm,) if torch.is_tensor(mm) else (lo, hi)
        hit = getattr(self, '_range_cache', None)
        if hit is None or hit[0] != key or None in key or len(hit[2]) != len(own) or any(a is not b for a, b in zip(hit[2], own)):
            host = lambda t: t.detach().float().cpu().tolist() if torch.is_tensor(t) else [float(v) for v in t]
            hit = self._range_cache = (key, (host(lo), host(hi)), own)
        return hit[1]

    def sample(self, texc, frame_id=None, mask=None):
        if not self.fused:
            return self._sample_composed(texc, mask)
        w = [self.net.net[i].weight for i in (0, 2, 4)]
        omin, omax = self._range_host()
        return _T.texture_mlp(texc, self.encoder.params, w[0], w[1], w[2], self.BBOX, omin, omax, mask=mask, in_grad_scale=self.net.loss_scale)

    def _sample_composed(self, texc, mask):
        """mlptexture.py:91-107: the encoding, then the network fused (`fused_net`) or op by op; rows with mask <= 0 give zeros (no gradient
        flows through them)"""
        dev = texc.device
        b0 = torch.tensor(self.BBOX[:3], dtype=torch.float32, device=dev)
        b1 = torch.tensor(self.BBOX[3:], dtype=torch.float32, device=dev)
        x = torch.clamp((texc.reshape(-1, 3) - b0[None]) / (b1 - b0)[None], min=0, max=1)
        enc = self.encoder(x.contiguous())
        if self.fused_net:
            lo, hi = (torch.as_tensor(v, dtype=torch.float32, device=dev) for v in (self.min_max[0], self.min_max[1]))
            w = [m.weight for m in self.net.net if isinstance(m, torch.nn.Linear)]
            out = _F.fused_mlp(enc, w, self.net_cfg, mask=None if mask is None else mask.reshape(-1), out_scale=hi - lo, out_bias=lo,
                               in_grad_scale=self.net.loss_scale)
            return out.reshape(*texc.shape[:-1], self.channels)
        if self.net.loss_scale != 1.0:
            enc = _ScaleGrad.apply(enc, self.net.loss_scale)
        out = self.net(enc)
        lo, hi = (torch.as_tensor(v, dtype=torch.float32, device=dev) for v in (self.min_max[0], self.min_max[1]))
        out = torch.sigmoid(out) * (hi[None, :] - lo[None, :]) + lo[None, :]
        if mask is not None:
            out = out * (mask.reshape(-1, 1) > 0).to(out.dtype)
        return out.reshape(*texc.shape[:-1], self.channels)

    def clamp_(self):
        pass

    def cleanup(self):
        tcnn.free_temporary_memory()
