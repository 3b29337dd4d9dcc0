"""What dropout costs per training step, and what the gate kernel does against its yardstick:

  * neuro3d_lite at 183^2 with dropout_rate=0.5 on every Conv against the plain net of the same
    build and a second plain net (what two plans of one net differ by), interleaved on one box
    (HIP-event device time per step, the median of each block of steps);
  * e2_dropout_fwd in place on a tensor of the net's largest activation (1, 20, 23, 90, 90)
    next to the bias + relu pass with a (1,1,1) window on a tensor of the same size (the existing
    stream kernel with the same traffic: one read, one write per element): bytes moved / duration.

Run by hand on one MI355X:

    python tools/dropout_step_bench.py [steps=40] [rounds=3]

Under `rocprofv3 --kernel-trace --stats -- python tools/dropout_step_bench.py 20 1` the per-kernel
side of the step delta is (a) dropout_kernel + dropout_tick_kernel and (b) what the plain net runs
fused and the dropout net does not (tail_kernel, head_*_kernel against the conv, bias / activation
and softmax launches that replace them)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SPEC = [(20, (1, 4, 4), (1, 2, 2)), (40, (3, 3, 3), (1, 2, 2)), (150, (2, 4, 4), (2, 1, 1)),
        (200, (1, 3, 3), (1, 1, 1)), (200, (1, 3, 3), (1, 1, 1)), (200, (1, 1, 1), (1, 1, 1))]
SP = (23, 183, 183)


def build(rate, name):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.newmodel(name)
    np.random.seed(1)
    inp = nm.Input((1, 1) + SP, 'b,f,z,x,y', name='raw')
    out = inp
    for n_f, k, p in SPEC:
        out = nm.Conv(out, n_f, k, p, dropout_rate=rate)
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin', dropout_rate=rate)
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
    x = torch.rand(shape, device=ctx.device)
    y = torch.empty_like(x)
    bias = torch.zeros(shape[1], device=ctx.device)
    rate = torch.full((1,), 0.5, device=ctx.device)
    state = torch.zeros(4, dtype=torch.int32, device=ctx.device)
    nbytes = 2 * 4 * x.numel()

    def timed(fn):
        for _ in range(5):
            fn()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ctx.stream)
            fn()
            e1.record(ctx.stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), float(min(ts))
    for name, fn in (("dropout_fwd (in place)", lambda: ctx.dropout_fwd(x, x, rate, state, 0)),
                     ("dropout_fwd (x -> y)", lambda: ctx.dropout_fwd(x, y, rate, state, 0)),
                     ("bias + relu, window (1,1,1)", lambda: ctx.pool_bias_act_fwd(x, bias, (1, 1, 1), 'relu', y))):
        med, best = timed(fn)
        print("%-28s %s: median %.1f us  min %.1f us  %.2f TB/s at the median (%.1f MB moved)"
              % (name, shape, med * 1e3, best * 1e3, nbytes / (med * 1e-3) / 1e12, nbytes / 1e6))


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    nets = [("plain",) + build(0, 'plain'), ("plain2",) + build(0, 'plain2'),
            ("dropout",) + build(0.5, 'dropout')]
    for _, m, args in nets:                    # eager step, capture, a few replays
        for _ in range(8):
            m.trainingstep(*args, optimiser='Adam')
    med = {k: [] for k, _, _ in nets}
    for r in range(rounds):
        for k, m, args in nets:
            ts = [m.trainingstep(*args, optimiser='Adam')[1] for _ in range(steps)]
            med[k].append(float(np.median(ts)) * 1e3)
            print("round %d %-8s median %.4f ms  min %.4f ms" % (r, k, med[k][-1], min(ts) * 1e3))
    u, w, u2 = np.array(med["plain"]), np.array(med["dropout"]), np.array(med["plain2"])
    print("two plain plans of the same net: %.4f vs %.4f ms (%+.1f us)"
          % (u.mean(), u2.mean(), (u2.mean() - u.mean()) * 1e3))
    print("plain %.4f ms (spread of the rounds %.4f), dropout %.4f ms (spread %.4f): delta %+.1f us / step"
          % (u.mean(), u.max() - u.min(), w.mean(), w.max() - w.min(), (w.mean() - u.mean()) * 1e3))
    plan = nets[2][1].optimisers['Adam'].step.func
    convs = [n for n in plan.nodes if type(n).__name__ == 'Conv']
    print("dropout plan: %d gate launches forward + %d backward + 1 tick; first layer fused %s, "
          "tail %s, head %s" % (len(plan._drop_nodes), len(plan._drop_nodes), convs[0]._fused_first(plan),
                                 convs[-2]._tail(plan) is not None, convs[-1]._fused_head(plan) is not None))
    kernel_bench()


if __name__ == "__main__":
    main()
