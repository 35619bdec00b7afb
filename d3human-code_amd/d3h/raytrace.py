"""Host side of csrc/bvh.hip: a triangle BVH built on the device and the any-hit occlusion query on it.

    bvh = Bvh(verts, tris)                      # builds on the current stream; inputs are detached
    hit = bvh.occluded(origins, dirs)           # bool[...]: does origin + t dir cross a triangle at tmin <= t <= tmax

Any-hit, two-sided; zero-area triangles are never hit; F = 0 or V = 0 is a valid empty scene in which nothing is occluded.  The build takes the
centroid bounds with torch.amin / amax, writes 64-bit keys (30-bit Morton code << 32 | triangle index) in a kernel, sorts them with torch.sort and
builds the radix-tree hierarchy, the boxes and the miss links in two more kernels; nothing is read back to the host.

BUILDS counts the builds of this process (the laziness test of render.optixutils reads it)."""
import ctypes

import torch

from . import _lib as L

BUILDS = 0


def _layout(F):
    sizes = (ctypes.c_int64 * 4)()
    L.call('bvh_layout', F, sizes)
    return [int(v) for v in sizes]


class Bvh:
    def __init__(self, verts, tris):
        global BUILDS
        verts = verts.detach().reshape(-1, 3).float().contiguous()
        tris = tris.detach().reshape(-1, 3)
        if tris.dtype not in (torch.int32, torch.int64):
            raise RuntimeError(f'Bvh: tris must be int32 or int64, got {tris.dtype}')
        if tris.device != verts.device:
            raise RuntimeError('Bvh: verts and tris must live on the same device')
        tris = tris.contiguous()
        dev = verts.device
        self.device = dev
        V, F = int(verts.shape[0]), int(tris.shape[0])
        self.F = F if V > 0 else 0
        self.nodes = self.tri9 = None
        BUILDS += 1
        if self.F == 0:
            return
        n_nodes, n_tri, n_work, n_keys = _layout(F)
        wide = int(tris.dtype == torch.int64)
        cen = verts[tris.reshape(-1).long().clamp(0, V - 1)].reshape(F, 3, 3).mean(1)
        cbounds = torch.cat([cen.amin(0), cen.amax(0)]).contiguous()
        keys = torch.empty(n_keys, dtype=torch.int64, device=dev)
        self.nodes = torch.empty(n_nodes, dtype=torch.float32, device=dev)
        self.tri9 = torch.empty(n_tri, dtype=torch.float32, device=dev)
        work = torch.empty(n_work, dtype=torch.int32, device=dev)

        def phase(p, k):
            L.call('bvh_build', p, verts, V, tris, wide, F, cbounds, k, self.nodes, self.tri9, work)
        phase(0, keys)
        phase(1, torch.sort(keys).values.contiguous())

    def occluded(self, origins, dirs, tmin=0.0, tmax=1e16):
        if origins.shape != dirs.shape or origins.shape[-1] != 3:
            raise RuntimeError(f'Bvh.occluded: origins and dirs must both be [..., 3], got {tuple(origins.shape)} and {tuple(dirs.shape)}')
        shape = origins.shape[:-1]
        o = origins.detach().reshape(-1, 3).float().contiguous()
        d = dirs.detach().reshape(-1, 3).float().contiguous()
        out = torch.empty(o.shape[0], dtype=torch.uint8, device=o.device)
        L.call('bvh_occluded', self.nodes, self.tri9, self.F, o, d, o.shape[0], tmin, tmax, out)
        return out.bool().reshape(shape)
