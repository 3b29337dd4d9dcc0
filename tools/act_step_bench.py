"""What an activation other than relu / lin costs, and what the act kernels do against their yardstick:

  * e2_act_fwd / e2_act_bwd (csrc/act.hip) for tanh and elu (and relu, through the same kernels) on
    a tensor of neuro3d_lite@183's largest activation (1, 20, 23, 90, 90), next to the bias + relu
    stream kernels of the relu route on the same tensor (e2_pool_bias_act_fwd / _bwd with a
    (1,1,1) window = pool_fwd_fixed<1,1,1> / pool_bwd_fixed<1,1,1>): HIP-event time per launch of 20
    warm back-to-back launches in one process, median and minimum of 50 windows, and bytes moved /
    duration (forward: one read + one write per element; backward: two reads + one write);
  * neuro3d_lite at 183^2 with every hidden Conv on 'elu' against the relu net of the same build
    and a second relu net (what two plans of one net differ by), interleaved on one box (device
    time per step, the median of each block of steps).  The elu net gives up the fused first
    layer, the fused epilogues, the activation backward inside the consumer's data gradient and
    the tail: the delta is the price of the un-fused route, the figure a later fusion is measured
    against.

Run by hand on one MI355X:

    python tools/act_step_bench.py [steps=40] [rounds=3] [hidden activation=elu]

Under `rocprofv3 --kernel-trace --stats -- python tools/act_step_bench.py 20 1` the per-kernel side
of the step delta is e2act_fwd_kernel / e2act_bwd_kernel + maxpool kernels against the fused
kernels the relu net runs instead."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SPEC = [(20, (1, 4, 4), (1, 2, 2)), (40, (3, 3, 3), (1, 2, 2)), (150, (2, 4, 4), (2, 1, 1)),
        (200, (1, 3, 3), (1, 1, 1)), (200, (1, 3, 3), (1, 1, 1)), (200, (1, 1, 1), (1, 1, 1))]
SP = (23, 183, 183)


def build(act, name):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.newmodel(name)
    np.random.seed(1)
    inp = nm.Input((1, 1) + SP, 'b,f,z,x,y', name='raw')
    out = inp
    for n_f, k, p in SPEC:
        out = nm.Conv(out, n_f, k, p, activation_func=act)
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin')
    probs = nm.Softmax(out)
    target = nm.Input_like(probs, override_f=1, name='target')
    loss = nm.AggregateLoss(nm.MultinoulliNLL(probs, target, target_is_sparse=True), name='loss')
    m = nm.model_manager.current
    m.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=probs)
    m.set_opt_meta_params('Adam', dict(lr=5e-4, mom=0.9, beta2=0.999, wd=0.5e-4))
    rng = np.random.RandomState(0)
    osp = tuple(probs.shape.spatial_shape)
    args = [rng.rand(1, 1, *SP).astype(np.float32),
            rng.randint(0, 2, (1, 1) + osp).astype(np.float32)]
    return m, args


def kernel_bench(reps=50):
    import torch
    from elektronn2_amd.neuromancer.plan import get_ctx
    ctx = get_ctx()
    shape = (1, 20, 23, 90, 90)
    x = (torch.randn(shape, device=ctx.device) * 2.0).contiguous()
    g = torch.randn(shape, device=ctx.device)
    y = torch.empty_like(x)
    bias = torch.zeros(shape[1], device=ctx.device)
    dbias = torch.zeros(shape[1], device=ctx.device)
    n = x.numel()

    def timed(fn, batch=20):
        """per-launch time of `batch` back-to-back launches between two events: median and minimum
        over `reps` such windows (a single ~10 us launch is mostly launch boundary)"""
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
    rows = [("fwd", "bias + relu, window (1,1,1)", 2, lambda: ctx.pool_bias_act_fwd(x, bias, (1, 1, 1), 'relu', y)),
            ("bwd", "bias + relu, window (1,1,1)", 3, lambda: ctx.pool_bias_act_bwd(g, x, bias, (1, 1, 1), 'relu', y, dbias))]
    for act in ('relu', 'tanh', 'elu'):
        rows.append(("fwd", "act_fwd %s" % act, 2, (lambda a: lambda: ctx.act_fwd(x, bias, a, y))(act)))
        rows.append(("bwd", "act_bwd %s" % act, 3, (lambda a: lambda: ctx.act_bwd(g, x, bias, a, y, dbias))(act)))
    base = {}
    for kind, name, streams, fn in rows:
        med, best = timed(fn)
        base.setdefault(kind, med)
        nbytes = streams * 4 * n
        print("%s %-28s %s: median %.1f us  min %.1f us  %.2f TB/s at the median (%.1f MB moved; %.1f us at "
              "8 TB/s HBM)  x%.2f of the relu pass"
              % (kind, name, shape, med * 1e3, best * 1e3, nbytes / (med * 1e-3) / 1e12, nbytes / 1e6,
                 nbytes / 8e12 * 1e6, med / base[kind]))


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    act = sys.argv[3] if len(sys.argv) > 3 else 'elu'
    kernel_bench()
    nets = [("relu",) + build('relu', 'relu'), ("relu2",) + build('relu', 'relu2'),
            (act,) + build(act, 'new')]
    for _, m, args in nets:                    # eager step, capture, a few replays
        for _ in range(8):
            m.trainingstep(*args, optimiser='Adam')
    med = {k: [] for k, _, _ in nets}
    for r in range(rounds):
        for k, m, args in nets:
            ts = [m.trainingstep(*args, optimiser='Adam')[1] for _ in range(steps)]
            med[k].append(float(np.median(ts)) * 1e3)
            print("round %d %-8s median %.4f ms  min %.4f ms" % (r, k, med[k][-1], min(ts) * 1e3))
    u, w, u2 = np.array(med["relu"]), np.array(med[act]), np.array(med["relu2"])
    print("two relu plans of the same net: %.4f vs %.4f ms (%+.1f us)"
          % (u.mean(), u2.mean(), (u2.mean() - u.mean()) * 1e3))
    print("relu %.4f ms (spread of the rounds %.4f), %s %.4f ms (spread %.4f): delta %+.1f us / step"
          % (u.mean(), u.max() - u.min(), act, w.mean(), w.max() - w.min(), (w.mean() - u.mean()) * 1e3))
    plan = nets[2][1].optimisers['Adam'].step.func
    convs = [n for n in plan.nodes if type(n).__name__ == 'Conv']
    print("%s plan: first layer fused %s, fused epilogues %d, tail %s, head %s"
          % (act, convs[0]._fused_first(plan), sum(bool(n._fused_act(plan)) for n in convs[1:-1]),
             convs[-2]._tail(plan) is not None, convs[-1]._fused_head(plan) is not None))


if __name__ == "__main__":
    main()
