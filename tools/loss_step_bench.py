"""What the element-wise losses cost, and what their kernels do against a yardstick:

  * e2_loss_fwd / e2_loss_mix / e2_loss_bwd (csrc/loss_elem.hip) for BinaryNLL, SquaredLoss (with
    margin and scale_correction) and GaussianNLL on a prediction of (1, 3, 116, 132, 132) -- a dense
    affinity map of the config-5 size -- next to e2_act_fwd (sigmoid) on the same tensor: HIP-event
    time per launch of 20 warm back-to-back launches in one process, median and minimum of 50
    windows, and bytes moved / duration (forward: two reads per element, three for GaussianNLL;
    backward: two reads + one write, GaussianNLL three reads + two writes; the mix: its slabs);
  * the neuro3d_lite trunk at 183^2 with a 3-feature 'sigmoid' head + BinaryNLL and with a 1-feature
    'lin' head + SquaredLoss, against the stock softmax net of the same build and a second stock
    net (what two plans of one net differ by), interleaved on one box (device time per step, the
    median of each block of steps).  The stock net runs the fused tail launch and these do not: the
    delta is the price of the un-fused route, the figure a later fused sigmoid + BinaryNLL head
    would be measured against.

Run by hand on one MI355X:

    python tools/loss_step_bench.py [steps=40] [rounds=3]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SPEC = [(20, (1, 4, 4), (1, 2, 2)), (40, (3, 3, 3), (1, 2, 2)), (150, (2, 4, 4), (2, 1, 1)),
        (200, (1, 3, 3), (1, 1, 1)), (200, (1, 3, 3), (1, 1, 1)), (200, (1, 1, 1), (1, 1, 1))]
SP = (23, 183, 183)


def build(head, name):
    """head: 'softmax' (the stock net), 'binary' (3 sigmoid features + BinaryNLL) or 'squared'"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.newmodel(name)
    np.random.seed(1)
    rng = np.random.RandomState(0)
    inp = nm.Input((1, 1) + SP, 'b,f,z,x,y', name='raw')
    out = inp
    for n_f, k, p in SPEC:
        out = nm.Conv(out, n_f, k, p)
    if head == 'softmax':
        out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin')
        pred = nm.Softmax(out)
        target = nm.Input_like(pred, override_f=1, name='target')
        loss = nm.AggregateLoss(nm.MultinoulliNLL(pred, target, target_is_sparse=True), name='loss')
        t = rng.randint(0, 2, (1, 1) + tuple(pred.shape.spatial_shape)).astype(np.float32)
    elif head == 'binary':
        pred = nm.Conv(out, 3, (1, 1, 1), activation_func='sigmoid')
        target = nm.Input_like(pred, name='target')
        loss = nm.AggregateLoss(nm.BinaryNLL(pred, target), name='loss')
        t = rng.randint(0, 2, (1, 3) + tuple(pred.shape.spatial_shape)).astype(np.float32)
    else:
        pred = nm.Conv(out, 1, (1, 1, 1), activation_func='lin')
        target = nm.Input_like(pred, name='target')
        loss = nm.AggregateLoss(nm.SquaredLoss(pred, target), name='loss')
        t = rng.randn(1, 1, *pred.shape.spatial_shape).astype(np.float32)
    m = nm.model_manager.current
    m.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=pred)
    m.set_opt_meta_params('Adam', dict(lr=5e-4, mom=0.9, beta2=0.999, wd=0.5e-4))
    return m, [rng.rand(1, 1, *SP).astype(np.float32), t]


def kernel_bench(reps=50):
    import torch
    from elektronn2_amd import backend
    from elektronn2_amd.neuromancer.plan import get_ctx
    ctx = get_ctx()
    shape = (1, 3, 116, 132, 132)
    p = torch.rand(shape, device=ctx.device) * 0.9 + 0.05
    s = torch.rand(shape, device=ctx.device) + 0.5
    t = (torch.rand(shape, device=ctx.device) > 0.5).float()
    t.view(-1)[::3] = -666.0
    dp, ds, y = torch.empty_like(p), torch.empty_like(p), torch.empty_like(p)
    n = p.numel()
    rows_n = ctx.loss_partials(p)
    slab = torch.empty(4 * rows_n, device=ctx.device)
    coef, tl, cnt = (torch.zeros(8, device=ctx.device) for _ in range(3))
    out = torch.zeros(1, device=ctx.device)
    mix = torch.ones(8, device=ctx.device)
    mg, sc = torch.tensor([0.3], device=ctx.device), torch.tensor([0.7], device=ctx.device)

    def timed(fn, batch=20):
        for _ in range(5):
            fn()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            for _ in range(batch):
                fn()
            e1.record(ctx.stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / batch)
        return float(np.median(ts)), float(min(ts))
    terms = [("binary_nll", backend.loss_term('binary_nll'), None),
             ("squared m+sc", backend.loss_term('squared', margin=mg, scale_correction=sc), None),
             ("gauss_nll", backend.loss_term('gauss_nll'), s)]
    rows = [("act_fwd sigmoid (yardstick)", 2 * 4 * n, lambda: ctx.act_fwd(p, None, 'sigmoid', y))]
    for name, term, sig in terms:
        ctx.loss_fwd(term, p, sig, t, slab)
        ctx.loss_mix([term], [slab], [n], mix, coef, tl, cnt, out)
        rd = 3 if sig is not None else 2
        rows.append(("loss_fwd %s" % name, rd * 4 * n,
                     (lambda tm, sg: lambda: ctx.loss_fwd(tm, p, sg, t, slab))(term, sig)))
        rows.append(("loss_bwd %s" % name, (rd + (2 if sig is not None else 1)) * 4 * n,
                     (lambda tm, sg: lambda: ctx.loss_bwd(tm, p, sg, t, coef[0:1], dp,
                                                          ds if sg is not None else None))(term, sig)))
    t3 = [terms[0][1]] * 3
    rows.append(("loss_mix, 1 term x %d rows" % rows_n, 16 * rows_n,
                 lambda: ctx.loss_mix(t3[:1], [slab], [n], mix, coef, tl, cnt, out)))
    rows.append(("loss_mix, 3 terms x %d rows" % rows_n, 3 * 16 * rows_n,
                 lambda: ctx.loss_mix(t3, [slab] * 3, [n] * 3, mix, coef, tl, cnt, out)))
    for name, nbytes, fn in rows:
        med, best = timed(fn)
        print("%-32s %s: median %.1f us  min %.1f us  %.2f TB/s at the median (%.2f MB moved; %.1f us at "
              "8 TB/s HBM)" % (name, shape, med * 1e3, best * 1e3, nbytes / (med * 1e-3) / 1e12,
                               nbytes / 1e6, nbytes / 8e12 * 1e6))


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    kernel_bench()
    nets = [("softmax",) + build('softmax', 'stock'), ("softmax2",) + build('softmax', 'stock2'),
            ("binary",) + build('binary', 'binary'), ("squared",) + build('squared', 'squared')]
    for _, m, args in nets:                    # eager step, capture, a few replays
        for _ in range(8):
            m.trainingstep(*args, optimiser='Adam')
    med = {k: [] for k, _, _ in nets}
    for r in range(rounds):
        for k, m, args in nets:
            ts = [m.trainingstep(*args, optimiser='Adam')[1] for _ in range(steps)]
            med[k].append(float(np.median(ts)) * 1e3)
            print("round %d %-8s median %.4f ms  min %.4f ms" % (r, k, med[k][-1], min(ts) * 1e3))
    u, u2 = np.array(med["softmax"]), np.array(med["softmax2"])
    print("two stock plans of the same net: %.4f vs %.4f ms (%+.1f us)"
          % (u.mean(), u2.mean(), (u2.mean() - u.mean()) * 1e3))
    for k in ("binary", "squared"):
        w = np.array(med[k])
        print("softmax %.4f ms (spread of the rounds %.4f), %s %.4f ms (spread %.4f): delta %+.1f us / step"
              % (u.mean(), u.max() - u.min(), k, w.mean(), w.max() - w.min(), (w.mean() - u.mean()) * 1e3))
    plan = nets[0][1].optimisers['Adam'].step.func
    convs = [n for n in plan.nodes if type(n).__name__ == 'Conv']
    print("stock plan: tail %s, head %s" % (convs[-2]._tail(plan) is not None,
                                            convs[-1]._fused_head(plan) is not None))


if __name__ == "__main__":
    main()
