"""What the feature-axis loss kernels reach against a plain copy of the same bytes:

  * e2_fdist_fwd / e2_fdist_bwd (csrc/loss_map.hip) and e2_beta_nll_fwd / e2_beta_nll_bwd
    (csrc/loss_elem.hip) on (1, 3, 20, 128, 128) and (1, 16, 20, 128, 128): HIP-event time of one
    launch, 20 warm-ups, the median of 100, and the bytes the launch must move / that time
    (fdist forward: two F-feature reads + a one-feature write; backward: two F-feature reads, two
    one-feature reads, two F-feature writes; BetaNLL forward: three reads; backward: three reads +
    two writes);
  * next to each, the rate e2_copy5 reaches in the same process on a dense tensor of the same
    number of bytes (half read, half written).

At F = 3 every operand is 3.9 MB and the whole working set of a launch stays in the caches between
the back-to-back launches: that row is a cache rate, for the kernel and for the copy alike, not an
HBM rate.  At F = 16 a launch moves 44 - 105 MB.

A record, not a gate: nothing asserts on these figures (DESIGN.md quotes them).  Run by hand on one
MI355X:

    python tools/loss_map_bench.py"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SHAPES = [(1, 3, 20, 128, 128), (1, 16, 20, 128, 128)]
WARM, REPS = 20, 100


def timed(ctx, fn):
    import torch
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ctx.stream)
        fn()
        e1.record(ctx.stream)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    import torch
    from elektronn2_amd.neuromancer.plan import get_ctx
    ctx = get_ctx()
    dev = ctx.device
    print("%-34s %12s %10s %10s %12s" % ("launch", "bytes", "us", "GB/s", "copy5 GB/s"))
    for shape in SHAPES:
        one = (shape[0], 1) + shape[2:]
        n, n1 = int(np.prod(shape)), int(np.prod(one))
        p, t = torch.randn(shape, device=dev), torch.randn(shape, device=dev)
        out, dout = torch.empty(one, device=dev), torch.randn(one, device=dev)
        dp, dt = torch.empty(shape, device=dev), torch.empty(shape, device=dev)
        m = torch.rand(shape, device=dev) * 0.96 + 0.02
        c = torch.rand(shape, device=dev) * 20 + 2.1
        x = torch.rand(shape, device=dev)
        slab = torch.empty(4 * ctx.loss_partials(m), device=dev)
        coef = torch.full((1,), 1.0 / n, device=dev)
        ctx.fdist_fwd(p, t, out)
        rows = [("fdist_fwd", 4 * (2 * n + n1), lambda: ctx.fdist_fwd(p, t, out)),
                ("fdist_bwd", 4 * (4 * n + 2 * n1), lambda: ctx.fdist_bwd(p, t, out, dout, dp, dt)),
                ("beta_nll_fwd", 4 * 3 * n, lambda: ctx.beta_nll_fwd(m, c, x, slab)),
                ("beta_nll_bwd", 4 * 5 * n, lambda: ctx.beta_nll_bwd(m, c, x, coef, dp, dt))]
        for name, nbytes, fn in rows:
            ms = timed(ctx, fn)
            half = nbytes // 8                               # floats read = floats written
            src, dst = torch.empty((1, 1, 1, 1, half), device=dev), torch.empty((1, 1, 1, 1, half), device=dev)
            src.normal_()
            ms_c = timed(ctx, lambda: ctx.copy5(src, dst))
            print("%-34s %12d %10.2f %10.1f %12.1f"
                  % ("%s F=%d" % (name, shape[1]), nbytes, ms * 1e3, nbytes / ms / 1e6,
                     8 * half / ms_c / 1e6), flush=True)


if __name__ == "__main__":
    main()
