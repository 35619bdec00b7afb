"""Shim under the third-party name so `import nvdiffrast.torch as dr` (train.py:19, render/*.py) resolves to the
MI355X kernels of csrc/raster.hip and csrc/texture.hip.  Only the entry points the reference calls are provided."""
from d3h import raster as _raster, texture as _texture
from d3h.raster import antialias, interpolate, rasterize as _rasterize  # noqa: F401
from d3h.texture import TextureMip, texture_construct_mip  # noqa: F401


class RasterizeGLContext:
    """opaque handle (train.py:1674); the HIP rasterizer needs no GL/CUDA context"""
    def __init__(self, *a, **k):
        pass


RasterizeCudaContext = RasterizeGLContext


def rasterize(glctx, pos, tri, resolution, ranges=None, grad_db=True):
    """nvdiffrast's defaults: with grad_db (the default) the pixel derivatives are differentiable in pos; without, they come back detached"""
    return _rasterize(pos, tri, resolution, grad_db=grad_db)


class DepthPeeler:
    """render/render.py:400-403 uses exactly one layer; the first layer is a plain rasterize (grad_db as in rasterize)"""
    def __init__(self, glctx, pos, tri, resolution, ranges=None, grad_db=True):
        self.pos, self.tri, self.res = pos, tri, resolution
        self.grad_db = grad_db
        self.layer = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def rasterize_next_layer(self, want_db=True):
        """want_db False (extension): the caller reads no pixel derivatives; the second result is None"""
        if self.layer > 0:
            raise NotImplementedError('d3h DepthPeeler: only the first layer (the reference asserts num_layers == 1)')
        self.layer += 1
        return _rasterize(self.pos, self.tri, self.res, want_db=want_db, grad_db=self.grad_db)


def texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode='auto', boundary_mode='wrap', max_mip_level=None):
    """nvdiffrast.texture, nvdiffrast's signature and defaults (d3h/texture.py states the contract).  Bilinear / clamp without mips and
    without a uv gradient -- the jitter taps of render/render.py -- stays on d3h.raster.texture; everything else runs d3h.texture."""
    mode = filter_mode
    if mode == 'auto':
        mode = 'linear-mipmap-linear' if (uv_da is not None or mip_level_bias is not None) else 'linear'
    if mode == 'linear' and boundary_mode == 'clamp' and mip is None and not uv.requires_grad:
        return _raster.texture(tex, uv, filter_mode='linear', boundary_mode='clamp')
    return _texture.texture(tex, uv, uv_da, mip_level_bias, mip, filter_mode, boundary_mode, max_mip_level)
