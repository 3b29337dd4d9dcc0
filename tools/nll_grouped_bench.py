"""Times the loss of a net with E independent softmaxes both ways, on the output size of
nets.neuro3d at its benchmark patch (23, 185, 185) with 6 features (E = 3, k = 2):

  * grouped:   e2_softmax_nll_grouped_fwd + e2_softmax_nll_grouped_bwd, one launch each;
  * per slice: E launches of e2_softmax_nll_fwd into one stats buffer, then E launches of
    e2_softmax_nll_bwd -- the kernels of the n_indep = 1 nets on channel slices;

each as eager launches and replayed from a captured graph.  One "pass" = zero the statistics,
forward, backward.  Device time between two HIP events around ``batch`` passes, ``reps`` such
windows after a warm-up, the two forms alternating window by window; median, minimum and maximum
per pass.  The two forms must agree (loss to 1e-5, probabilities and dlogits bit for bit) before
anything is timed.

Run by hand on one MI355X:   python tools/nll_grouped_bench.py [reps=30] [batch=20]
Human-readable lines go to stderr, ONE JSON line to stdout."""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def out_shape():
    from elektronn2_amd import nets, neuromancer as nm
    nm.model_manager.reset()
    m = nets.neuro3d((None, 1, 23, 185, 185))
    sp = tuple(int(s) for s in m.prediction_node.shape.spatial_shape)
    nm.model_manager.reset()
    return sp


def main():
    import torch
    from elektronn2_amd import backend
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    assert reps >= 20
    assert torch.cuda.is_available(), "nll_grouped_bench measures on the GPU only"
    E, k = 3, 2
    sp = out_shape()
    stream = torch.cuda.Stream()
    ctx = backend.Context(0)
    ctx.set_stream(stream)

    def say(*a):
        print(*a, file=sys.stderr)

    rng = np.random.RandomState(0)
    with torch.cuda.stream(stream):
        lg = torch.tensor((rng.randn(1, E * k, *sp) * 3).astype(np.float32), device='cuda')
        t = rng.randint(0, k, (1, E) + sp).astype(np.float32)
        t.flat[::17] = -1
        tg = torch.tensor(t, device='cuda')
        bufs = {}
        for form in ('grouped', 'slices'):
            bufs[form] = dict(probs=torch.empty_like(lg), dl=torch.empty_like(lg),
                              stats=torch.zeros(2, device='cuda'), loss=torch.zeros(1, device='cuda'))

    def grouped():
        b = bufs['grouped']
        ctx.fill(b['stats'], 0.0)
        ctx.softmax_nll_grouped_fwd(lg, tg, b['probs'], E, b['stats'])
        ctx.softmax_nll_grouped_bwd(b['probs'], tg, E, b['stats'], b['dl'], b['loss'])

    def slices():
        b = bufs['slices']
        ctx.fill(b['stats'], 0.0)
        for g in range(E):
            sl = slice(g * k, (g + 1) * k)
            ctx.softmax_nll_fwd(lg[:, sl], tg[:, g:g + 1], b['probs'][:, sl], b['stats'])
        for g in range(E):
            sl = slice(g * k, (g + 1) * k)
            ctx.softmax_nll_bwd(b['probs'][:, sl], tg[:, g:g + 1], b['stats'], b['dl'][:, sl], b['loss'])

    forms = dict(grouped=grouped, slices=slices)
    for fn in forms.values():
        for _ in range(3):
            fn()
    ctx.synchronize()
    a, b = bufs['grouped'], bufs['slices']
    la, lb = float(a['loss']), float(b['loss'])
    assert abs(la - lb) <= 1e-5 * abs(lb), (la, lb)
    assert torch.equal(a['probs'], b['probs']) and torch.equal(a['dl'], b['dl'])
    say("output %s, E = %d, k = %d: loss %.7f (grouped) %.7f (per slice), probabilities and dlogits "
        "bit-equal" % ((1, E * k) + sp, E, k, la, lb))

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
    # bytes one pass has to move: logits read, probabilities written and read, dlogits written,
    # the target read twice
    nbytes = 4 * (4 * lg.numel() + 2 * tg.numel())
    for n in res:
        res[n]['tb_s'] = nbytes / (res[n]['median_us'] * 1e-6) / 1e12
    for g in graphs.values():
        ctx.graph_destroy(g)
    print(json.dumps(dict(tool="nll_grouped_bench", shape=[1, E * k] + list(sp), n_indep=E, reps=reps,
                          batch=batch, bytes_per_pass=nbytes, results=res)))


if __name__ == "__main__":
    main()
