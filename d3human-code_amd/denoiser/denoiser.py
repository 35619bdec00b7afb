"""The cross-bilateral denoiser module of the lit render path, with the surface of the reference's denoiser/denoiser.py (BilateralDenoiser:
set_influence, sigma, variance, N, forward) on render.optixutils' kernel (csrc/denoise.hip).

`forward_many` is an extension: the demodulated path filters diffuse and specular light under the SAME normals and depths, and it filters both in
one launch each way (d3h.denoise.bilateral_denoise_many), the guides staged and the tap weights computed once."""
import math

import torch

from render import util
from render import optixutils as ou
from d3h import denoise as _denoise


class BilateralDenoiser(torch.nn.Module):
    def __init__(self, influence=1.0):
        super().__init__()
        self.set_influence(influence)

    def set_influence(self, factor):
        self.sigma = max(factor * 2, 0.0001)
        self.variance = self.sigma ** 2.
        self.N = 2 * math.ceil(self.sigma * 2.5) + 1

    def forward(self, input):
        """input [B,H,W,8] = (colour, normal, depth, depth gradient) -> the filtered colour [B,H,W,3]"""
        nrm = util.safe_normalize(input[..., 3:6])          # bent normals can be shorter than 1
        return ou.bilateral_denoiser(input[..., 0:3], nrm, input[..., 6:8], self.sigma)

    def forward_many(self, cols, nrm, zdz):
        """cols: a list of one or two colour images [B,H,W,3] filtered under one set of guides nrm [B,H,W,3], zdz [B,H,W,2] -> the list of filtered
        images, each equal to forward(cat(col, nrm, zdz)) bit for bit"""
        nrm = util.safe_normalize(nrm)
        return [cw[..., 0:3] / cw[..., 3:4] for cw in _denoise.bilateral_denoise_many(cols, nrm, zdz, self.sigma)]
