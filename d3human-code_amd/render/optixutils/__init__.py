"""render.optixutils on the MI355X: the reference's four names with its signatures and defaults (render/optixutils/ops.py:128-147), on the
project's own ray tracer instead of OptiX -- a device-built BVH with a stackless any-hit traversal (d3h.raytrace, csrc/bvh.hip), the
importance-sampled environment shading (d3h.envshade, csrc/envshade.hip) and the cross-bilateral denoiser (d3h.denoise, csrc/denoise.hip).

The BVH is built lazily.  The reference rebuilds it several times per getMesh_* (geometry/hmsdf.py:464-516) although training, with its
hard-wired bsdf='kd' (render/render.py:120), never traces a ray; so `optix_build_bvh` only records its arguments and the build happens at the
first `optix_env_shade` against the context (or at `ctx.build()`)."""
import numpy as np
import torch

from d3h import denoise as _denoise, envshade as _envshade, raytrace as _raytrace

__all__ = ['OptiXContext', 'optix_build_bvh', 'optix_env_shade', 'bilateral_denoiser']

_BSDFS = ['pbr', 'diffuse', 'white']        # the order is the kernel's mode number
_random_perm = {}                           # n_samples_x -> [32768, n_samples_x^2] int32, made on first use


class OptiXContext:
    """Holds the mesh given to optix_build_bvh (`pending`) and the BVH built from it (`bvh`); `frames`: (the record, one context per posed frame) when
    render_mesh traced a batch of posed meshes against it (render.render._frame_contexts)."""

    def __init__(self):
        self.pending = None
        self.bvh = None
        self.frames = None

    def build(self):
        """Build now what optix_build_bvh recorded -- for callers that overwrite the tensors before they shade."""
        if self.pending is not None:
            verts, tris = self.pending
            self.bvh = _raytrace.Bvh(verts.reshape(-1, 3), tris.reshape(-1, 3))
            self.pending = None
        if self.bvh is None:
            raise RuntimeError('OptiXContext: optix_build_bvh was never called on this context')
        return self.bvh


def optix_build_bvh(optix_ctx, verts, tris, rebuild):
    """Record the mesh of the next build.  Free: no kernel launch, no copy, no synchronisation -- the BVH is built at the first optix_env_shade
    against the context, or by optix_ctx.build().  The lazy build reads the CONTENTS the tensors have at that first use, not at this call: a caller
    that overwrites them in place in between calls optix_ctx.build() first.  Both values of `rebuild` mean "rebuild at next use" (there is no
    refit in place of a rebuild); a second call before use replaces the first.  An empty mesh is a valid scene in which nothing is occluded."""
    optix_ctx.pending = (verts, tris)
    optix_ctx.frames = None


def optix_env_shade(optix_ctx, mask, ro, gb_pos, gb_normal, gb_view_pos, gb_kd, gb_ks, light, pdf, rows, cols, BSDF='pbr', n_samples_x=8, rnd_seed=None,
                    shadow_scale=1.0):
    """-> (diffuse [B,H,W,3], specular [B,H,W,3]) of the pixels with mask > 0 under the lat-long environment `light`, shadowed by the context's mesh.

    rnd_seed=None draws np.random.randint(2**31) once for the forward and once more for the backward (the reference's behaviour under
    FLAGS.decorrelated: gradient noise independent of the image noise); an int is used for both passes.  The table of permutations that decorrelates
    the light and BSDF strata is cached per n_samples_x, [32768, n_samples_x^2], made on first use."""
    if BSDF not in _BSDFS:
        raise RuntimeError(f"optix_env_shade: BSDF must be one of 'pbr', 'diffuse', 'white', got {BSDF!r}")
    bvh = optix_ctx.build()
    n = int(n_samples_x)
    key = (n, str(gb_pos.device))
    if key not in _random_perm:
        _random_perm[key] = torch.argsort(torch.rand(32768, n * n, device=gb_pos.device), dim=-1).int()
    seed = np.random.randint(2 ** 31) if rnd_seed is None else int(rnd_seed)
    bwd_seed = np.random.randint(2 ** 31) if rnd_seed is None else int(rnd_seed)
    return _envshade.env_shade(bvh, mask, ro, gb_pos, gb_normal, gb_view_pos, gb_kd, gb_ks, light, pdf, rows, cols, _random_perm[key], _BSDFS.index(BSDF), n, seed,
                               bwd_seed, shadow_scale)


def bilateral_denoiser(col, nrm, zdz, sigma):
    col_w = _denoise.bilateral_denoise(col, nrm, zdz, sigma)
    return col_w[..., 0:3] / col_w[..., 3:4]
