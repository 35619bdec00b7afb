"""Shim under the third-party name so `import nvdiffrast.torch as dr` (train.py:19, render/*.py) resolves to the
MI355X kernels of csrc/raster.hip and csrc/texture.hip: rasterize (instanced and range mode), DepthPeeler, interpolate, antialias,
antialias_construct_topology_hash, texture, texture_construct_mip.  The OpenGL-only options of nvdiffrast are not provided."""
from d3h import raster as _raster, texture as _texture
from d3h.raster import antialias, antialias_construct_topology_hash, interpolate, rasterize as _rasterize  # noqa: F401
from d3h.texture import TextureMip, texture_construct_mip  # noqa: F401


class RasterizeGLContext:
    """opaque handle (train.py:1674); the HIP rasterizer needs no GL/CUDA context"""
    def __init__(self, *a, **k):
        pass


RasterizeCudaContext = RasterizeGLContext


def rasterize(glctx, pos, tri, resolution, ranges=None, grad_db=True):
    """nvdiffrast's defaults: with grad_db (the default) the pixel derivatives are differentiable in pos; without, they come back detached.
    ranges: range mode with a 2-D pos [V, 4] (d3h/raster.py's docstring), ignored with a 3-D pos"""
    return _rasterize(pos, tri, resolution, grad_db=grad_db, ranges=ranges)


class DepthPeeler:
    """nvdiffrast's depth peeling (d3h/raster.py's docstring states the contract).  The first layer is a plain rasterize -- the same entry
    point and cost as before, the one layer render/render.py:400-403 uses; every later layer peels the previous one, whose `rast` this
    object keeps: modifying it in place between two calls is refused rather than peeled from.  After the last non-empty layer the calls
    return empty layers."""
    def __init__(self, glctx, pos, tri, resolution, ranges=None, grad_db=True):
        self.pos, self.tri, self.res = pos, tri, resolution
        self.ranges = ranges
        self.grad_db = grad_db
        self.layer = 0
        self.prev, self.prev_version = None, None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.prev = None
        return False

    def rasterize_next_layer(self, want_db=True):
        """want_db False (extension): the caller reads no pixel derivatives; the second result is None"""
        if self.layer > 0:
            if self.prev is None:
                raise RuntimeError('DepthPeeler: rasterize_next_layer after the peeler was closed')
            if self.prev._version != self.prev_version:
                raise RuntimeError('DepthPeeler: the previous layer\'s rast was modified in place; depth peeling needs it as it was returned')
        rast, db = _rasterize(self.pos, self.tri, self.res, want_db=want_db, grad_db=self.grad_db, prev_rast=self.prev, ranges=self.ranges)
        self.prev, self.prev_version = rast, rast._version
        self.layer += 1
        return rast, db


def texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode='auto', boundary_mode='wrap', max_mip_level=None):
    """nvdiffrast.texture, nvdiffrast's signature and defaults (d3h/texture.py states the contract).  Bilinear / clamp without mips and
    without a uv gradient -- the jitter taps of render/render.py -- stays on d3h.raster.texture; everything else runs d3h.texture."""
    mode = filter_mode
    if mode == 'auto':
        mode = 'linear-mipmap-linear' if (uv_da is not None or mip_level_bias is not None) else 'linear'
    if mode == 'linear' and boundary_mode == 'clamp' and mip is None and not uv.requires_grad:
        return _raster.texture(tex, uv, filter_mode='linear', boundary_mode='clamp')
    return _texture.texture(tex, uv, uv_da, mip_level_bias, mip, filter_mode, boundary_mode, max_mip_level)
