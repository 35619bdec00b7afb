"""Host cost per call of crossing the C ABI from Python, on the emulation library (no GPU): three entry points with arguments that return
before any kernel runs, so that the time is the binding's alone.

    python tools/abi_call_cost.py [--pkg <d3human-code_amd of another checkout>] [--style call|raw] [--calls 20000] [--rounds 3]

--style call: d3h._lib.call() (the typed binding); raw: the hand-wrapped form `L.check(L.lib().d3h_x(L.ptr(t), L.i32(n), ..., L.stream()), 'x')`,
which is how every call site was written before the binding and still works.  --pkg times another checkout's package (A/B of two commits:
run the two alternately).  Prints the median, minimum and maximum of the rounds, microseconds per call.  Numbers: profiles/abi_call_cost.md."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--pkg', default=os.path.join(ROOT, 'd3human-code_amd'))
ap.add_argument('--style', default='call', choices=('call', 'raw'))
ap.add_argument('--calls', type=int, default=20000)
ap.add_argument('--rounds', type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, args.pkg)
import torch  # noqa: E402
from d3h import _lib as L  # noqa: E402

L._use_emulator_for_tests(os.path.join(ROOT, 'tests', 'emul', 'libd3h_emul.so'))
f = lambda *s: torch.zeros(*s)
x, g, w, act = f(0, 3), f(0, 1), f(64), f(64)
wpt3 = tiles = torch.zeros(64, dtype=torch.int32)
pos, tri, keys, vals, flags = f(1, 4, 4), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(1024, dtype=torch.int64), torch.zeros(2048, dtype=torch.int32), \
    torch.zeros(1, 1, dtype=torch.uint8)
img = f(0, 3)

if args.style == 'call':
    SITES = {
        'sdf_mlp_bwd (24 + stream)': lambda: L.call('sdf_mlp_bwd', x, None, 0.0, g, w, w, wpt3, act, act, 0, x, w, w, w, w, w, w, w, w, tiles, wpt3, 3, 3, 0),
        'antialias_flags (11 + stream)': lambda: L.call('antialias_flags', pos, 0, tri, 0, 1, keys, vals, 1024, 16, 16, flags),
        'image_loss_bwd (9 + stream)': lambda: L.call('image_loss_bwd', img, img, 0, 1, 1, w, 1.0, img, None),
    }
else:
    P, I, J, F = L.ptr, L.i32, L.i64, L.f32
    SITES = {
        'sdf_mlp_bwd (24 + stream)': lambda: L.check(L.lib().d3h_sdf_mlp_bwd(
            P(x), P(None), F(0.0), P(g), P(w), P(w), P(wpt3), P(act), P(act), J(0), P(x), P(w), P(w), P(w), P(w), P(w), P(w), P(w), P(w), P(tiles),
            P(wpt3), I(3), I(3), I(0), L.stream()), 'sdf_mlp_bwd'),
        'antialias_flags (11 + stream)': lambda: L.check(L.lib().d3h_antialias_flags(
            P(pos), I(0), P(tri), I(0), I(1), P(keys), P(vals), I(1024), I(16), I(16), P(flags), L.stream()), 'antialias_flags'),
        'image_loss_bwd (9 + stream)': lambda: L.check(L.lib().d3h_image_loss_bwd(
            P(img), P(img), J(0), I(1), I(1), P(w), F(1.0), P(img), P(None), L.stream()), 'image_loss_bwd'),
    }

for name, fn in SITES.items():
    fn()
    us = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        us.append((time.perf_counter() - t0) / args.calls * 1e6)
    print(f'{args.style:4s} {name:30s} median {statistics.median(us):6.2f} us  min {min(us):6.2f}  max {max(us):6.2f}')
