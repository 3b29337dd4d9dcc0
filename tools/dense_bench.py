"""The Perceptron's three products through the one-thread-per-output kernels (csrc/dense_bn.hip)
and through the MFMA GEMMs (csrc/dense_gemm.hip), in the same process on the same tensors.

For each (n, k, m) and each of fwd / dgrad / wgrad: HIP events around WINDOW warm back-to-back
launches (the split-K form counts its two launches as one call), the median of REPS windows per
call, 2 n k m flops over that time, and its share of the fp32-MFMA peak bench.py uses.  The
operands of every shape here fit the caches: these are launch-to-launch rates of cache-resident
GEMMs, not HBM rates.  The two routes alternate window by window, so that a drift of the clocks
touches both alike; `spread` is (max - min) / median over the windows of the new route.

A record, not a gate: nothing asserts on these figures (DESIGN.md quotes them).  Run by hand on one
MI355X:

    python tools/dense_bench.py"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SHAPES = [(128, 784, 512), (128, 512, 784), (32, 20000, 256), (20, 576, 200), (32, 600, 256)]
PEAK_FP32_MFMA_TFLOPS = 157.3        # bench.py
WARM, WINDOW, REPS = 20, 50, 15


def window(ctx, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ctx.stream)
    for _ in range(WINDOW):
        fn()
    e1.record(ctx.stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / WINDOW


def main():
    import torch
    from elektronn2_amd.neuromancer.plan import get_ctx
    ctx = get_ctx()
    dev = ctx.device
    print("%-22s %-6s %9s %9s %8s %9s %7s %7s  %s" % ("(n, k, m)", "op", "old us", "new us", "old/new",
                                                      "TFLOP/s", "% peak", "spread", "tile, splits"))
    for n, k, m in SHAPES:
        x, w, dy = (torch.randn(s, device=dev) for s in ((n, k), (k, m), (n, m)))
        y, dx, dw = (torch.empty(s, device=dev) for s in ((n, m), (n, k), (k, m)))
        nb = ctx.dense_gemm_workspace_bytes(n, k, m)
        ws = torch.empty(max(nb // 4, 1), device=dev)
        rows = [("fwd", lambda: ctx.dense_fwd(x, w, y), lambda: ctx.dense_gemm_fwd(x, w, y, ws=ws)),
                ("dgrad", lambda: ctx.dense_dgrad(dy, w, dx), lambda: ctx.dense_gemm_dgrad(dy, w, dx, ws=ws)),
                ("wgrad", lambda: ctx.dense_wgrad(x, dy, dw), lambda: ctx.dense_gemm_wgrad(x, dy, dw, ws=ws))]
        for op, old, new in rows:
            for fn in (old, new):
                for _ in range(WARM):
                    fn()
            t_old, t_new = [], []
            for _ in range(REPS):
                t_old.append(window(ctx, old))
                t_new.append(window(ctx, new))
            mo, mn = float(np.median(t_old)), float(np.median(t_new))
            tf = 2.0 * n * k * m / (mn * 1e-3) / 1e12
            c = ctx.dense_gemm_choice(op, n, k, m)
            print("%-22s %-6s %9.2f %9.2f %8.2f %9.2f %7.2f %6.1f%%  %dx%d, %d"
                  % ((n, k, m), op, mo * 1e3, mn * 1e3, mo / mn, tf, 100 * tf / PEAK_FP32_MFMA_TFLOPS,
                     100 * (max(t_new) - min(t_new)) / mn, c['tile'][0], c['tile'][1], c['splits']),
                  flush=True)


if __name__ == "__main__":
    main()
