"""2-D texture maps with the interface of the reference's render/texture.py (:20-182): `texture2d_mip`, `Texture2D`, `create_trainable`,
`srgb_to_rgb` / `rgb_to_srgb`, `load_texture2D` / `save_texture2D`.  Written for this build: the mip op is csrc/uvatlas.hip (d3h.uvatlas), the
lookup is the build's nvdiffrast.texture (csrc/texture.hip), image files go through render/util.py (its own PNG code when no image library is
installed).  Tensors made from numpy data land on the GPU when there is one (the reference hard-codes 'cuda')."""
import os

import numpy as np
import torch
import nvdiffrast.torch as dr

from d3h import uvatlas as _U
from . import util


def _device():
    return 'cuda' if torch.cuda.is_available() else 'cpu'


class texture2d_mip(torch.autograd.Function):
    """NHWC 2 x 2 mean; its gradient is the bilinear x2 upsample of 0.25 dout (texture.py:20-30), not the adjoint.  Odd H or W: ValueError."""

    @staticmethod
    def forward(ctx, texture):
        return _U.mip2x2_fwd(texture)

    @staticmethod
    def backward(ctx, dout):
        return _U.mip2x2_bwd(dout)


class Texture2D:
    """`init`: a constant ([C]), one image ([H,W,C] or [N,H,W,C]; mips are built on the fly in sample()), or a list of NHWC levels (a custom mip
    chain, used as given).  numpy arrays are converted.  `min_max` = (low [C], high [C]) is what clamp_() enforces."""

    def __init__(self, init, min_max=None):
        if isinstance(init, np.ndarray):
            init = torch.tensor(init, dtype=torch.float32, device=_device())
        if isinstance(init, (list, tuple)) and len(init) == 1:
            init = init[0]
        if isinstance(init, (list, tuple)):
            self.data = list(init)
        elif init.dim() == 4:
            self.data = init
        elif init.dim() == 3:
            self.data = init[None]
        else:
            self.data = init.reshape(1, 1, 1, -1)
        self.min_max = min_max

    def sample(self, texc, texc_deriv, filter_mode='linear-mipmap-linear'):
        """filtered lookup at texc [N,h,w,2] with its screen-space derivatives"""
        if isinstance(self.data, list):
            return dr.texture(self.data[0], texc, texc_deriv, mip=self.data[1:], filter_mode=filter_mode)
        if min(self.data.shape[1:3]) <= 1:
            return dr.texture(self.data, texc, texc_deriv, filter_mode=filter_mode)
        chain = [self.data]
        while min(chain[-1].shape[1:3]) > 1:
            chain.append(texture2d_mip.apply(chain[-1]))
        return dr.texture(chain[0], texc, texc_deriv, mip=chain[1:], filter_mode=filter_mode)

    def getMips(self):
        return self.data if isinstance(self.data, list) else [self.data]

    def getRes(self):
        return self.getMips()[0].shape[1:3]

    def getChannels(self):
        return self.getMips()[0].shape[3]

    def parameters(self):
        return self.getMips()

    def clamp_(self):
        """per-channel clamp to min_max, in place"""
        if self.min_max is None:
            return
        lo, hi = self.min_max
        for level in self.getMips():
            for c in range(level.shape[-1]):
                level[..., c].clamp_(min=lo[c], max=hi[c])

    def normalize_(self):
        with torch.no_grad():
            for level in self.getMips():
                level.copy_(util.safe_normalize(level))


def create_trainable(init, res=None, auto_mipmaps=True, min_max=None):
    """a Texture2D whose level(s) are fresh leaf tensors that require grad, initialised from `init` (a Texture2D, numpy array or tensor; constant /
    HWC / NHWC), resampled to `res`; auto_mipmaps=False: an explicit chain down to 1 x 1, every level a parameter"""
    with torch.no_grad():
        if isinstance(init, Texture2D):
            assert torch.is_tensor(init.data), 'create_trainable: a texture with a custom mip chain cannot be the initial guess'
            min_max = init.min_max if min_max is None else min_max
            init = init.data
        elif isinstance(init, np.ndarray):
            init = torch.tensor(init, dtype=torch.float32, device=_device())
        if init.dim() == 1:
            init = init.reshape(1, 1, 1, -1)
        elif init.dim() == 3:
            init = init[None]
        if res is not None:
            init = util.scale_img_nhwc(init, res)
        leaf = lambda t: t.detach().clone().requires_grad_(True)
        if auto_mipmaps:
            return Texture2D(leaf(init), min_max=min_max)
        chain = [leaf(init)]
        while max(chain[-1].shape[1:3]) > 1:
            h, w = chain[-1].shape[1:3]
            chain.append(leaf(util.scale_img_nhwc(chain[-1], [max(h // 2, 1), max(w // 2, 1)])))
        return Texture2D(chain, min_max=min_max)


def srgb_to_rgb(texture):
    return Texture2D([util.srgb_to_rgb(level) for level in texture.getMips()])


def rgb_to_srgb(texture):
    return Texture2D([util.rgb_to_srgb(level) for level in texture.getMips()])


def _level_name(fn, i):
    base, ext = os.path.splitext(fn)
    return '%s_%d%s' % (base, i, ext)


def _load_level(fn, lambda_fn, channels):
    img = torch.tensor(util.load_image(fn), dtype=torch.float32, device=_device())
    if channels is not None:
        img = img[..., :channels]
    if lambda_fn is not None:
        img = lambda_fn(img)
    return img.detach().clone()


def load_texture2D(fn, lambda_fn=None, channels=None):
    """`name.ext`, or the custom mip chain `name_0.ext`, `name_1.ext`, ... when `name_0.ext` exists"""
    if not os.path.exists(_level_name(fn, 0)):
        return Texture2D(_load_level(fn, lambda_fn, channels))
    levels = []
    while os.path.exists(_level_name(fn, len(levels))):
        levels.append(_load_level(_level_name(fn, len(levels)), lambda_fn, channels))
    return Texture2D(levels)


def save_texture2D(fn, tex, lambda_fn=None):
    """image 0 of the texture to `fn`; a custom mip chain to `name_0.ext`, `name_1.ext`, ..."""
    chain = isinstance(tex.data, list)
    for i, level in enumerate(tex.getMips()):
        img = level[0] if lambda_fn is None else lambda_fn(level[0])
        util.save_image(_level_name(fn, i) if chain else fn, img.detach().cpu().numpy())
