"""The trainable lat-long environment light, with the public surface of the reference's render/light.py (EnvironmentLight, load_env,
save_env_map, create_trainable_env_rnd) so that train.py, which imports `render.light`, gets this module.

`update_pdf`, called once per training iteration, builds the three tables the importance sampler of render.optixutils searches -- the texel pdf,
the per-row column CDFs and the row CDF -- in two launches of csrc/envlight.hip (d3h.envlight) instead of a chain of torch ops."""
import os

import numpy as np
import torch
import nvdiffrast.torch as dr

from . import util
from d3h import envlight as _envlight


def _device():
    return 'cuda' if torch.cuda.is_available() else 'cpu'


class EnvironmentLight:
    LIGHT_MIN_RES = 16

    MIN_ROUGHNESS = 0.08
    MAX_ROUGHNESS = 0.5

    def __init__(self, base):
        self.mtx = None
        self.base = base                       # [H,W,3] radiance, lat-long; may be a leaf that requires grad
        self.pdf_scale = (base.shape[0] * base.shape[1]) / (2 * np.pi * np.pi)
        self.update_pdf()

    def xfm(self, mtx):
        self.mtx = mtx

    def parameters(self):
        return [self.base]

    def clone(self):
        return EnvironmentLight(self.base.clone().detach())

    def clamp_(self, min=None, max=None):
        self.base.clamp_(min, max)

    def update_pdf(self):
        """_pdf [H,W]: max over channels times sin(theta), normalised to sum 1; cols [H,W]: each row's CDF; rows [H,W]: the CDF of the row totals,
        repeated along W (an expanded view: callers read rows[:, 0])"""
        self._pdf, self.rows, self.cols = _envlight.tables(self.base)

    @torch.no_grad()
    def generate_image(self, res):
        """the map resampled (bilinear) to [res[0], res[1], 3]"""
        uv = util.pixel_grid(res[1], res[0], device=self.base.device)
        return dr.texture(self.base[None].contiguous(), uv[None].contiguous(), filter_mode='linear')[0]


@torch.no_grad()
def load_env(fn, scale=1.0, res=None, trainable=False):
    """An .hdr lat-long image through util.load_image, scaled; res = [H, W] resamples it (clamped to >= 1e-4)."""
    ext = os.path.splitext(fn)[1].lower()
    assert ext == '.hdr', 'Unknown envlight extension %s' % ext
    img = torch.tensor(util.load_image(fn), dtype=torch.float32, device=_device()) * scale
    if res is not None:
        uv = util.pixel_grid(res[1], res[0], device=img.device)
        img = torch.clamp(dr.texture(img[None].contiguous(), uv[None].contiguous(), filter_mode='linear')[0], min=0.0001)
    print('EnvProbe,', img.shape, ', min/max', torch.min(img).item(), torch.max(img).item())
    if trainable:
        return EnvironmentLight(img.clone().detach().requires_grad_(True))
    return EnvironmentLight(img)


@torch.no_grad()
def save_env_map(fn, light):
    assert isinstance(light, EnvironmentLight)
    util.save_image_raw(fn, light.generate_image([512, 1024]).detach().cpu().numpy())


def create_trainable_env_rnd(base_res, scale=0.5, bias=0.25):
    base = torch.rand(base_res, base_res, 3, dtype=torch.float32, device=_device()) * scale + bias
    return EnvironmentLight(base.clone().detach().requires_grad_(True))
