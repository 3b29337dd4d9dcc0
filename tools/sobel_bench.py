"""What the SobelizedLoss stencil kernels (csrc/loss_sobel.hip) reach against a plain copy of the
bytes they must move:

  * e2_sobel_abs_fwd / e2_sobel_abs_bwd on one prediction-sized tensor (1, 2, 64, 128, 128), dim 3,
    with a margin: HIP-event time of one launch, 20 warm-ups, the median of 100, and the bytes the
    launch must move (forward: p + t read; backward: p + t read, dp written) / that time;
  * next to each, the rate e2_copy5 reaches in the same process on a dense tensor of the same
    number of bytes (half read, half written).

Each operand is 8.4 MB: the working set of back-to-back launches stays in the last-level cache, for
the kernel and for the copy alike.  The second shape, (1, 8, 96, 256, 256) at 201 MB per operand,
does not.

A record, not a gate: nothing asserts on these figures (DESIGN.md section 25 quotes them).  Run by
hand on one MI355X:

    python tools/sobel_bench.py"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from loss_map_bench import timed

SHAPES = [(1, 2, 64, 128, 128), (1, 8, 96, 256, 256)]


def main():
    import torch
    from elektronn2_amd import backend
    from elektronn2_amd.neuromancer.plan import get_ctx
    ctx = get_ctx()
    dev = ctx.device
    print("%-34s %12s %10s %10s %12s" % ("launch", "bytes", "us", "GB/s", "copy5 GB/s"))
    for shape in SHAPES:
        n = int(np.prod(shape))
        p, t, dp = (torch.randn(shape, device=dev) for _ in range(3))
        term = backend.loss_term('abs', margin=torch.full((1,), 0.1, device=dev))
        slab = torch.empty(4 * ctx.sobel_partials(p), device=dev)
        coef = torch.full((1,), 1.0 / (3 * n), device=dev)
        rows = [("sobel_abs_fwd", 4 * 2 * n, lambda: ctx.sobel_abs_fwd(term, 3, p, t, slab)),
                ("sobel_abs_bwd", 4 * 3 * n, lambda: ctx.sobel_abs_bwd(term, 3, p, t, coef, dp))]
        for name, nbytes, fn in rows:
            ms = timed(ctx, fn)
            half = nbytes // 8                               # floats read = floats written
            src, dst = torch.randn((1, 1, 1, 1, half), device=dev), torch.empty((1, 1, 1, 1, half), device=dev)
            ms_c = timed(ctx, lambda: ctx.copy5(src, dst))
            print("%-34s %12d %10.2f %10.1f %12.1f"
                  % ("%s %s" % (name, "x".join(map(str, shape[1:]))), nbytes, ms * 1e3, nbytes / ms / 1e6,
                     8 * half / ms_c / 1e6), flush=True)


if __name__ == "__main__":
    main()
