"""What the 'same' border mode costs, and what the pad kernel does against its yardstick:

  * step time of nets.unet3d_lite((1,1,22,136,136), conv_mode='same'), f32, with plan option
    pad_inplace on and off, alternated in one process (device time per step between HIP events,
    the median of each block of steps); per plan the number of e2_pad5 launches per step (counted
    on an eager step of a graph=False twin of the plan's options);
  * e2_pad5 (csrc/pad.hip) on the largest framed image of that net: per-launch time of 20 warm
    back-to-back launches, median and minimum of 50 windows, and achieved bytes/s =
    4 * (src + dst elements) / time against the HBM peak (8 TB/s, MI355X).

Run by hand on one MI355X:

    python tools/bench_same.py [steps=30] [rounds=3]
    python tools/bench_same.py profile on|off [steps=20]

The second form runs warm replays of ONE plan only, for a profiler run of its own:
`rocprofv3 --kernel-trace --stats -- python tools/bench_same.py profile on` gives the share of
e2pad_kernel in the step's kernel time."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SP = (22, 136, 136)


def build(name, **opts):
    from elektronn2_amd import nets, neuromancer as nm
    with nm.plan_options(**opts):
        np.random.seed(1)
        m = nets.unet3d_lite((1, 1) + SP, name=name, conv_mode='same')
        m.set_opt_meta_params('Adam', dict(lr=5e-4, mom=0.9, beta2=0.999, wd=0.5e-4))
        rng = np.random.RandomState(0)
        args = [rng.rand(1, 1, *SP).astype(np.float32),
                rng.randint(0, 2, (1, 1) + SP).astype(np.float32)]
        m.trainingstep(*args, optimiser='Adam')          # (the plan is built inside the options)
    return m, args


def pad_launches(plan):
    return sum(1 for k in plan.scratch if isinstance(k, tuple) and len(k) == 2 and k[1] == 'xf_launch')


def largest_framed(plan):
    best = None
    for k, v in plan.scratch.items():
        if isinstance(k, tuple) and len(k) == 2 and k[1] == 'xf':
            if best is None or v.numel() > best[1].numel():
                best = (k[0], v)
    return best


def kernel_bench(plan, reps=50):
    import torch
    ctx = plan.ctx
    node, xf = largest_framed(plan)
    q = node._q3
    dst = torch.zeros(tuple(xf.shape), device=ctx.device)
    src = torch.randn(tuple(plan.out_shape(node.parent)), device=ctx.device)

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
    med, best = timed(lambda: ctx.pad5(src, dst, q))
    nbytes = 4 * (src.numel() + dst.numel())
    print("e2_pad5 %s -> %s (frame %s, conv %s): median %.1f us  min %.1f us  %.2f TB/s at the median "
          "(%.1f MB moved; %.1f us at 8 TB/s HBM = %.0f %% of peak)"
          % (tuple(src.shape), tuple(dst.shape), q, node.name, med * 1e3, best * 1e3,
             nbytes / (med * 1e-3) / 1e12, nbytes / 1e6, nbytes / 8e12 * 1e6,
             100.0 * nbytes / (med * 1e-3) / 8e12))
    fmed, fbest = timed(lambda: ctx.pad5(None, dst, q, frame_only=True))
    print("e2_pad5 frame only, same image: median %.1f us  min %.1f us" % (fmed * 1e3, fbest * 1e3))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == 'profile':
        on = (sys.argv[2] if len(sys.argv) > 2 else 'on') == 'on'
        steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
        m, args = build('prof', pad_inplace=on)
        for _ in range(4 + steps):
            m.trainingstep(*args, optimiser='Adam')
        plan = m.optimisers['Adam'].step.func
        print("pad_inplace=%s: %d e2_pad5 launches per step, %d steps run" % (on, pad_launches(plan), 5 + steps))
        return
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    nets_ = [("in place", ) + build('on', pad_inplace=True), ("by launch", ) + build('off', pad_inplace=False)]
    for _, m, args in nets_:                      # capture + a few replays
        for _ in range(8):
            m.trainingstep(*args, optimiser='Adam')
    med = {k: [] for k, _, _ in nets_}
    for r in range(rounds):
        for k, m, args in nets_:
            ts = [m.trainingstep(*args, optimiser='Adam')[1] for _ in range(steps)]
            med[k].append(float(np.median(ts)) * 1e3)
            print("round %d %-10s median %.4f ms  min %.4f ms" % (r, k, med[k][-1], min(ts) * 1e3))
    for k, m, _ in nets_:
        plan = m.optimisers['Adam'].step.func
        framed = sum(1 for q in plan.scratch if isinstance(q, tuple) and len(q) == 2 and q[1] == 'xf')
        by = [n.parent.name + ":" + type(n.parent).__name__ for n in plan.nodes
              if plan.scratch.get((n, 'xf_launch'))]
        print("%-10s %.4f ms (spread of the rounds %.4f): %d convs with a frame, %d e2_pad5 launches per step %s"
              % (k, np.mean(med[k]), max(med[k]) - min(med[k]), framed, pad_launches(plan), by))
    a, b = np.mean(med["in place"]), np.mean(med["by launch"])
    print("pad_inplace on %.4f ms, off %.4f ms: %+.1f us / step" % (a, b, (b - a) * 1e3))
    kernel_bench(nets_[1][1].optimisers['Adam'].step.func)


if __name__ == "__main__":
    main()
