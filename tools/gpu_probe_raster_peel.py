"""Time depth peeling and range mode of csrc/raster.hip on the GPU at 4 x 1024^2, with warm-up and device events, for the synth body mesh
(12.6 k faces) and a ~100 k-triangle random mesh:
  - layer 0 (d3h_rasterize_fwd) and layers 1-3, each split into the previous-key pass (d3h_rasterize_peel_keys) and the peeled raster
    (d3h_rasterize_peel_fwd on those keys);
  - range mode (the four frames' meshes concatenated, one range each) against instanced mode (pos [4, V, 4]).

Bytes the key pass must move (from the shapes): the previous rast read (16 B / pixel) and the key written (8 B / pixel), plus one
triangle's vertices per covered pixel (cached).  Reported: times, those bytes, bytes / time as a fraction of the HBM peak (8 TB/s), and
the layer-k / layer-0 ratio.

  python tools/gpu_probe_raster_peel.py [--iters N] [--out file.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'd3human-code_amd')]

import torch  # noqa: E402

HBM_PEAK = 8.0e12
B, RES = 4, 1024


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us


def body_clip():
    from d3h import mtets, synth
    v, t = (torch.from_numpy(a) for a in synth.kuhn_grid(72))
    o = mtets.marching_tets(v.cuda(), synth.body_sdf(v).cuda(), torch.ones(v.shape[0]).cuda(), t.cuda())
    verts, tri = o['verts'], o['faces32']
    _, mvp, _ = synth.camera(RES)
    offs = torch.tensor([[0.02 * b, 0.0, 0.0] for b in range(B)]).cuda()
    vh = torch.cat([verts[None] + offs[:, None], torch.ones(B, verts.shape[0], 1).cuda()], -1)
    return (vh @ torch.from_numpy(mvp).cuda().T).contiguous(), tri.contiguous()


def random_mesh(nf, size, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    cen = (torch.rand(B, nf, 1, 2, device='cuda', generator=g) * 2 - 1) * 0.9
    xy = (cen + (torch.rand(B, nf, 3, 2, device='cuda', generator=g) * 2 - 1) * size).reshape(B, nf * 3, 2)
    z = torch.rand(B, nf * 3, 1, device='cuda', generator=g) * 1.6 - 0.8
    w = torch.rand(B, nf * 3, 1, device='cuda', generator=g) * 2 + 1
    return torch.cat([xy * w, z * w, w], -1).contiguous(), torch.arange(nf * 3, dtype=torch.int32, device='cuda').reshape(nf, 3)


def probe(name, pos, tri, iters):
    from d3h import _lib as L, raster
    lib = L.lib()
    nb, V = pos.shape[:2]
    nf = tri.shape[0]
    npx = nb * RES * RES
    res = {'mesh': name, 'triangles': nf, 'frames': nb, 'res': RES}
    t0 = timed(lambda: raster.rasterize(pos, tri, (RES, RES)), iters)
    res['layer0_us'] = round(t0, 1)
    # layers 1..3: the previous-key pass and the peeled raster, timed apart on the same buffers
    rast = [raster.rasterize(pos, tri, (RES, RES))[0]]
    keys = torch.empty(npx, dtype=torch.int64, device='cuda')
    zbuf = torch.empty(npx, dtype=torch.int64, device='cuda')
    for k in (1, 2, 3):
        prev = rast[-1]
        out = torch.empty_like(prev)
        db = torch.empty_like(prev)
        kp = lambda: L.check(lib.d3h_rasterize_peel_keys(L.ptr(pos), L.i32(V * 4), L.ptr(tri), L.i32(nf), L.i32(nb), L.i32(RES), L.i32(RES),
                                                         L.ptr(prev), L.ptr(keys), L.stream()), 'peel_keys')
        rp = lambda: L.check(lib.d3h_rasterize_peel_fwd(L.ptr(pos), L.i32(V * 4), L.ptr(tri), L.i32(nf), L.i32(nb), L.i32(RES), L.i32(RES), L.ptr(None),
                                                        L.i32(0), L.ptr(None), L.ptr(keys), L.ptr(zbuf), L.ptr(out), L.ptr(db), L.stream()), 'peel_fwd')
        t_k = timed(kp, iters)
        kp()
        t_r = timed(rp, iters)
        t_all = timed(lambda: raster.rasterize(pos, tri, (RES, RES), prev_rast=prev), iters)
        ref, _ = raster.rasterize(pos, tri, (RES, RES), prev_rast=prev)
        assert torch.equal(out, ref)
        cov = float((prev[..., 3] > 0).float().mean())
        res[f'layer{k}'] = {'keys_us': round(t_k, 1), 'raster_us': round(t_r, 1), 'total_us': round(t_all, 1), 'ratio_to_layer0': round(t_all / t0, 2),
                            'key_bytes_per_px': 24, 'key_pass_hbm_frac': round(24 * npx / (t_k * 1e-6) / HBM_PEAK, 3),
                            'prev_covered_frac': round(cov, 3)}
        rast.append(ref)
    # range mode against instanced mode: the frames' meshes concatenated, one range each
    pos2 = pos.reshape(-1, 4).contiguous()
    tri_all = torch.cat([tri + b * V for b in range(nb)], 0).int().contiguous()
    ranges = torch.tensor([[b * nf, nf] for b in range(nb)], dtype=torch.int32)
    t_inst = timed(lambda: raster.rasterize(pos, tri, (RES, RES)), iters)
    t_rng = timed(lambda: raster.rasterize(pos2, tri_all, (RES, RES), ranges=ranges), iters)
    res['instanced_us'] = round(t_inst, 1)
    res['range_us'] = round(t_rng, 1)
    res['range_over_instanced'] = round(t_rng / t_inst, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available()
    out = []
    pos, tri = body_clip()
    out.append(probe('body', pos, tri, a.iters))
    pos, tri = random_mesh(100_000, 0.012)
    out.append(probe('random_100k', pos, tri, a.iters))
    for r in out:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
