"""Device time per launch of e2_lrn_fwd / e2_lrn_bwd (spatial (1,3,3), channel 5) and of the linear
pool pair with the same access pattern (average (1,3,3), stride 1) on (1, 20, 23, 90, 90): HIP events
around single launches, median (and minimum) of 30 after 5 warm-up launches, in microseconds.
DESIGN.md section 14 holds the figures.

    python tools/lrn_bench.py [out.json]"""
import os, sys, json
import numpy as np, torch
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
from elektronn2_amd import backend
ctx = backend.Context(0)
sh = (1, 20, 23, 90, 90)
g = torch.Generator(device='cuda').manual_seed(1)
x = 2 * torch.randn(sh, device='cuda', generator=g)
dout = torch.randn(sh, device='cuda', generator=g)
out, q, tmp, dx = (torch.empty(sh, device='cuda') for _ in range(4))
al, k, be = (torch.tensor([v], device='cuda') for v in (0.7, 1.5, 0.75))
psh = (1, 20, 23, 88, 88)
pout, pdout = torch.empty(psh, device='cuda'), torch.randn(psh, device='cuda', generator=g)
torch.cuda.synchronize()

def med(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0); fn(); ctx.record(e1)
        ts.append(ctx.elapsed_ms(e0, e1) * 1e3)
    return float(np.median(ts)), float(np.min(ts))

res = {}
for name, mode, f in (("spatial_133", 'spatial', (1, 3, 3)), ("channel_5", 'channel', (5, 1, 1))):
    res["lrn_fwd_" + name] = med(lambda: ctx.lrn_fwd(x, mode, f, al, k, be, out, q=q))
    res["lrn_fwd_noq_" + name] = med(lambda: ctx.lrn_fwd(x, mode, f, al, k, be, out))
    res["lrn_bwd_" + name] = med(lambda: ctx.lrn_bwd(dout, x, q, mode, f, al, be, tmp, dx))
res["pool_lin_fwd_133_s1"] = med(lambda: ctx.pool_lin_fwd(x, (1, 3, 3), (1, 1, 1), 'avg', pout))
res["pool_lin_bwd_133_s1"] = med(lambda: ctx.pool_lin_bwd(pdout, (1, 3, 3), (1, 1, 1), 'avg', dx))
res["bytes_per_tensor"] = int(np.prod(sh)) * 4
for k_, v in res.items():
    print(k_, v)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], 'w'), indent=1)
