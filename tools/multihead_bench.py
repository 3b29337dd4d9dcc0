"""Times three classifier heads (3 / 4 / 3 classes) on one trunk both ways, on the top feature map
of a 2-D U-Net: trunk (1, 64, 1, 284, 284):

  * fused:    e2_multihead_fwd + e2_nll_mix + e2_multihead_bwd (csrc/multihead.hip): the trunk is
              read once per direction, dx is written once;
  * per head: three e2_head_fwd and three e2_head_bwd (csrc/head.hip), accumulate_dx on the 2nd
              and 3rd -- how three heads run as copies of the single-loss route.  (Those launches
              take no mixing coefficient; that does not change their time.)

each as eager launches and replayed from a captured graph.  One "pass" = zero the statistics,
forward, (mix), backward with dx.  Device time between two HIP events around ``batch`` passes,
``reps`` such windows after a warm-up, the forms alternating window by window; median, minimum
and maximum per pass.  Before anything is timed the two forms must agree: with mixing weights
w_k = K the fused coefficients are the per-head ones, so the total is the sum of the heads' losses
(1e-5) and dx is the same tensor (2e-5 of its largest magnitude).

Run by hand on one MI355X:   python tools/multihead_bench.py [reps=30] [batch=20]
Human-readable lines go to stderr, ONE JSON line to stdout."""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def main():
    import torch
    from elektronn2_amd import backend
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    assert reps >= 20
    assert torch.cuda.is_available(), "multihead_bench measures on the GPU only"
    cin, classes, sp = 64, (3, 4, 3), (1, 284, 284)
    K = len(classes)
    stream = torch.cuda.Stream()
    ctx = backend.Context(0)
    ctx.set_stream(stream)

    def say(*a):
        print(*a, file=sys.stderr)

    rng = np.random.RandomState(0)
    dev = lambda a: torch.tensor(np.asarray(a, np.float32), device='cuda')
    with torch.cuda.stream(stream):
        x = dev(rng.rand(1, cin, *sp))
        ws = [dev(rng.randn(c, cin) / np.sqrt(cin)) for c in classes]
        bs = [dev(rng.randn(c) / 4) for c in classes]
        tgs = []
        for c in classes:
            t = rng.randint(0, c, (1, 1) + sp).astype(np.float32)
            t.flat[::17] = -1
            tgs.append(dev(t))
        mix = dev([float(K)] * K)
        bufs = {}
        for form in ('fused', 'heads'):
            bufs[form] = dict(probs=[torch.empty((1, c) + sp, device='cuda') for c in classes],
                              dx=torch.empty_like(x), stats=torch.zeros(2 * K, device='cuda'),
                              dw=[torch.zeros_like(w) for w in ws], db=[torch.zeros_like(b) for b in bs],
                              loss=torch.zeros(K, device='cuda'))
        coef, term, count = (torch.zeros(8, device='cuda') for _ in range(3))
        ws_f = torch.empty(ctx.multihead_bwd_ws_bytes(x.shape, sum(classes)) // 4 + 16, device='cuda')
        ws_h = [torch.empty(ctx.head_bwd_ws_bytes(x.shape, c) // 4 + 16, device='cuda') for c in classes]

    def fused():
        b = bufs['fused']
        ctx.fill(b['stats'], 0.0)
        ctx.multihead_fwd(x, ws, bs, tgs, b['probs'], b['stats'])
        ctx.nll_mix(K, b['stats'], mix, coef, term, count, b['loss'][:1])
        ctx.multihead_bwd(x, ws, b['probs'], tgs, coef, b['dx'], False, b['dw'], b['db'], ws_f)

    def heads():
        b = bufs['heads']
        ctx.fill(b['stats'], 0.0)
        for k in range(K):
            ctx.head_fwd(x, ws[k], bs[k], tgs[k], b['probs'][k], b['stats'][2 * k:2 * k + 2])
        for k in range(K):
            ctx.head_bwd(x, ws[k], b['probs'][k], tgs[k], b['stats'][2 * k:2 * k + 2], b['dx'], k > 0,
                         b['dw'][k], b['db'][k], b['loss'][k:k + 1], ws=ws_h[k])

    forms = dict(fused=fused, heads=heads)
    for fn in forms.values():
        for _ in range(3):
            fn()
    ctx.synchronize()
    a, b = bufs['fused'], bufs['heads']
    la, lb = float(a['loss'][0]), float(b['loss'].sum())
    assert abs(la - lb) <= 1e-5 * abs(lb), (la, lb)
    ddx = float((a['dx'] - b['dx']).abs().max() / b['dx'].abs().max())
    assert ddx < 2e-5, ddx
    say("trunk %s, heads %s: total %.7f (fused) %.7f (per head), dx differs by %.1e of its largest magnitude"
        % (tuple(x.shape), classes, la, lb, ddx))

    graphs = {}
    for name, fn in forms.items():
        ctx.graph_begin()
        for _ in range(batch):
            fn()
        graphs[name] = ctx.graph_end()
    runs = dict(("%s_eager" % n, (lambda fn=fn: [fn() for _ in range(batch)])) for n, fn in forms.items())
    runs.update(("%s_graph" % n, (lambda g=g: ctx.graph_launch(g))) for n, g in graphs.items())
    for fn in runs.values():
        for _ in range(3):
            fn()
    ctx.synchronize()
    ts = dict((n, []) for n in runs)
    for _ in range(reps):
        for n in sorted(runs):                       # the forms alternate window by window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            runs[n]()
            e1.record(stream)
            e1.synchronize()
            ts[n].append(e0.elapsed_time(e1) / batch * 1e3)         # us per pass
    res = {}
    for n in sorted(ts):
        v = ts[n]
        res[n] = dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)))
        say("%-14s %7.2f us per pass (min %.2f, max %.2f)" % (n, res[n]['median_us'], res[n]['min_us'], res[n]['max_us']))
    for g in graphs.values():
        ctx.graph_destroy(g)
    print(json.dumps(dict(tool="multihead_bench", trunk=list(x.shape), classes=list(classes), reps=reps,
                          batch=batch, results=res)))


if __name__ == "__main__":
    main()
