"""Host side of csrc/bvh.hip and csrc/bvhdist.hip: a triangle BVH built on the device, the any-hit occlusion query and the distance queries on it.

    bvh = Bvh(verts, tris)                      # builds on the current stream; inputs are detached
    hit = bvh.occluded(origins, dirs)           # bool[...]: does origin + t dir cross a triangle at tmin <= t <= tmax
    d2, tri, bary = bvh.nearest(points)         # Nearest(d2 float32[...], tri int32[...], bary float32[..., 3]); detached, like occluded()
    w = bvh.winding(points, beta=3.0)           # float32[...]: generalised winding number in turns
    sdf = bvh.signed_distance(points, beta=3.0) # float32[...]: positive outside, meshops.mesh_wsdf's sign rule; one launch

Any-hit, two-sided; zero-area triangles are never hit; F = 0 or V = 0 is a valid empty scene in which nothing is occluded.  The build takes the
centroid bounds with torch.amin / amax, writes 64-bit keys (30-bit Morton code << 32 | triangle index) in a kernel, sorts them with torch.sort and
builds the radix-tree hierarchy, the boxes and the miss links in two more kernels; nothing is read back to the host.

Distance queries (points [..., 3], any float dtype, on the Bvh's device; nothing is differentiable):
  * nearest: the exact nearest triangle -- the minimum over all triangles of the very arithmetic of meshops.mesh_sdf / mesh_wsdf (Ericson's region test
    in float32), found by a greedy descent for a first bound and a rope walk that skips a subtree whose box is farther than the best so far (widened
    against rounding: a box may be entered needlessly, never skipped wrongly).  `tri` is the ORIGINAL triangle index, ties in d2 (float32 equality) going
    to the smallest, so the result is that of a first-minimum-wins loop over the triangles; `bary` are the weights of the closest point on the triangle's
    three vertices (each >= 0, sum 1).  Zero-area triangles are never returned -- the rule of occluded(); the brute-force kernels treat them as segments
    or points, so on a mesh that has such triangles the two can differ where a collapsed triangle is the nearest thing.  F = 0 (or no triangle of
    non-zero area), or a point with a non-finite coordinate: d2 = +inf, tri = -1, bary = 0.
    A differentiable distance is the caller's composition from `tri` and `bary`, both constants of the graph:
        (p - (bary[:, :, None] * verts[tris[tri.long()]]).sum(1)).norm(dim=-1)
    -- the gradient with respect to p and verts of the distance to the closest point held fixed on its triangle, which is the gradient of the distance.
  * winding: the tree is walked from the root; a node whose centre c (area-weighted centroid) is farther from the query than beta * r (r: from c to
    the farthest corner of the node's box) contributes the dipole of its summed area vector, n . (c - q) / |c - q|^3, any other node is opened, a leaf
    contributes its exact solid angle (with mesh_wsdf's float64 repair of a triangle in whose plane the query lies).  beta = inf opens everything: the
    exact sum, in tree order.  First order after Barill et al. 2018.  The node moments are built at the first winding / signed_distance call.
    beta = 3.0 came from a sketch on a median-split tree with r = the farthest vertex (1068 triangles: max |w - w64| 0.050 / 0.018 / 0.008 at beta 2 / 3 /
    4).  Measured on THIS tree, float64 walk of the read-back nodes against the float64 sum over all triangles (tests/bvhdist_cases.py, 1000 queries in
    1.5 x the box): 320-face icosphere max |w - w64| 0.026 / 0.013 / 0.0018 at beta 2 / 3 / 4, visiting on average 84 / 176 / 273 of 639 nodes (the
    box-corner r opens more than the sketch's r did).  At the hand-off's sizes on an MI355X (tools/gpu_probe_bvhdist.py, profiles/bvhdist_probe.md: 21 000 to
    49 280 faces, lattice and push queries, a 4096-query sample against the float64 sum): max |w - w64| 0.037-0.054 / 0.015-0.026 / 0.008-0.012 at beta
    2 / 3 / 4, mean 0.0037 / 0.0018 / 0.0009 on the lattices, for 45 / 53 / 65 ms per 17 M queries; no sign differs from the brute-force route at any
    of the three.  These figures do not argue against 3.0: it stays.
  * signed_distance: (|w| > 0.5 ? -1 : +1) * sqrt(nearest d2), the inside rule and the 1e-3 rad rule of mesh_wsdf, winding walk and nearest walk in one
    launch.  Across the surface of a closed mesh w jumps between 0 and 1, which an error of a few hundredths cannot flip; where |w| is within the
    approximation's error of 0.5 -- near the virtual cap of an open mesh -- the sign can differ from the brute-force route's.

BUILDS counts the builds of this process (the laziness test of render.optixutils reads it)."""
import collections
import ctypes

import torch

from . import _lib as L

BUILDS = 0
Nearest = collections.namedtuple('Nearest', 'd2 tri bary')


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
        self.nodes = self.tri9 = self.leaf_tri = self.moments = self._work = None
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
        work = self._work = torch.empty(n_work, dtype=torch.int32, device=dev)          # parent / right child: the moments pass climbs by them

        def phase(p, k):
            L.call('bvh_build', p, verts, V, tris, wide, F, cbounds, k, self.nodes, self.tri9, work)
        phase(0, keys)
        keys = torch.sort(keys).values.contiguous()
        phase(1, keys)
        self.leaf_tri = (keys & 0xffffffff).clamp_(max=F - 1).int()         # leaf j holds this triangle of the input

    def occluded(self, origins, dirs, tmin=0.0, tmax=1e16):
        if origins.shape != dirs.shape or origins.shape[-1] != 3:
            raise RuntimeError(f'Bvh.occluded: origins and dirs must both be [..., 3], got {tuple(origins.shape)} and {tuple(dirs.shape)}')
        shape = origins.shape[:-1]
        o = origins.detach().reshape(-1, 3).float().contiguous()
        d = dirs.detach().reshape(-1, 3).float().contiguous()
        out = torch.empty(o.shape[0], dtype=torch.uint8, device=o.device)
        L.call('bvh_occluded', self.nodes, self.tri9, self.F, o, d, o.shape[0], tmin, tmax, out)
        return out.bool().reshape(shape)

    def _points(self, what, points):
        if not torch.is_tensor(points) or points.dim() < 1 or points.shape[-1] != 3 or not points.is_floating_point():
            raise RuntimeError(f'Bvh.{what}: points must be a float tensor [..., 3], got '
                               + (f'{tuple(points.shape)} {points.dtype}' if torch.is_tensor(points) else type(points).__name__))
        if points.device != self.device:
            raise RuntimeError(f'Bvh.{what}: points live on {points.device}, the Bvh on {self.device}')
        return points.shape[:-1], points.detach().reshape(-1, 3).float().contiguous()

    def nearest(self, points):
        shape, p = self._points('nearest', points)
        n = p.shape[0]
        d2 = torch.empty(n, dtype=torch.float32, device=p.device)
        tri = torch.empty(n, dtype=torch.int32, device=p.device)
        bary = torch.empty(n, 3, dtype=torch.float32, device=p.device)
        L.call('bvh_nearest', self.nodes, self.tri9, self.leaf_tri, self.F, p, n, d2, tri, bary)
        return Nearest(d2.reshape(shape), tri.reshape(shape), bary.reshape(*shape, 3))

    def _wsdf(self, what, points, beta, want_sdf, want_w):
        beta = float(beta)
        if not beta > 0.0:                                  # NaN as well
            raise RuntimeError(f'Bvh.{what}: beta must be > 0 (inf: the exact sum), got {beta}')
        shape, p = self._points(what, points)
        if self.moments is None and self.F > 0:
            self.moments = torch.empty(self.nodes.shape[0], dtype=torch.float32, device=self.device)
            L.call('bvh_moments', self.nodes, self.tri9, self._work, self.F, self.moments)
        n = p.shape[0]
        sdf = torch.empty(n, dtype=torch.float32, device=p.device) if want_sdf else None
        w = torch.empty(n, dtype=torch.float32, device=p.device) if want_w else None
        L.call('bvh_wsdf', self.nodes, self.tri9, self.moments, self.F, p, n, beta, sdf, w)
        return (sdf.reshape(shape) if want_sdf else None), (w.reshape(shape) if want_w else None)

    def winding(self, points, beta=3.0):
        return self._wsdf('winding', points, beta, False, True)[1]

    def signed_distance(self, points, beta=3.0):
        return self._wsdf('signed_distance', points, beta, True, False)[0]
