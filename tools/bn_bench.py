"""Batch normalisation through one work-group per channel (csrc/dense_bn.hip) and through C x slabs
work-groups (csrc/bn_wide.hip), in the same process on the same tensors.

For each shape and each of fwd / bwd (train mode, relu, every output asked for): HIP events around a
window of warm back-to-back calls (the wide forward is three launches, its backward two; a call is
what a node issues), the median of REPS windows per route, and GB/s against the bytes the operation
has to move -- forward 2 reads + 1 write of the tensor, backward 4 reads + 1 write -- whatever a
route actually reads.  The two routes alternate window by window, so that a drift of the clocks
touches both alike; `spread` is (max - min) / median over the windows of the new route.  The window
length is set per shape from one timed call, so that the large layers do not take minutes.

A record, not a gate: nothing asserts on these figures (DESIGN.md section 28 quotes them, and the
'auto' threshold NeuralLayer.BN_WIDE_MIN_COUNT is read off them).  Run by hand on one MI355X:

    python tools/bn_bench.py"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

# config 1's two largest; a ladder over the 'auto' threshold; a neuro3d-sized layer; a unet3d_lite-sized
# layer; a 200-channel layer; the config-5 U-Net layer of the issue
SHAPES = [(20, 12, 1, 12, 12), (20, 12, 1, 24, 24), (1, 32, 4, 64, 64), (1, 32, 8, 64, 64),
          (1, 32, 16, 64, 64), (1, 32, 32, 64, 64), (1, 20, 23, 90, 90), (1, 64, 26, 60, 60),
          (1, 200, 17, 39, 39), (1, 32, 116, 132, 132)]
WARM, REPS = 5, 9
WINDOW_MS, WINDOW_MIN, WINDOW_MAX = 20.0, 3, 50


def window(ctx, fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ctx.stream)
    for _ in range(calls):
        fn()
    e1.record(ctx.stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    import torch
    from elektronn2_amd.neuromancer.plan import get_ctx
    ctx = get_ctx()
    dev = ctx.device
    print("%-24s %9s %-4s %10s %10s %8s %9s %9s %7s  %s" % ("(n, c, d, h, w)", "per chan", "op", "old us", "new us",
                                                            "old/new", "old GB/s", "new GB/s", "spread", "slabs"))
    for shape in SHAPES:
        C = shape[1]
        x, dout = 3 + 2 * torch.randn(shape, device=dev), torch.randn(shape, device=dev)
        out, dx = torch.empty(shape, device=dev), torch.empty(shape, device=dev)
        gamma, bias = torch.rand(C, device=dev) + 0.5, 0.3 * torch.randn(C, device=dev)
        rm, rs = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        save, dg, db = torch.zeros(2 * C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        ws = torch.empty(ctx.batchnorm_wide_workspace_bytes(shape) // 4, device=dev)
        fargs = (x, gamma, bias, rm, rs, True, True, 'relu', out, save)
        bargs = (dout, x, gamma, bias, save, True, 'relu', dx, dg, db)
        rows = [("fwd", 3, lambda: ctx.batchnorm_act_fwd(*fargs), lambda: ctx.batchnorm_wide_fwd(*fargs, ws=ws)),
                ("bwd", 5, lambda: ctx.batchnorm_act_bwd(*bargs), lambda: ctx.batchnorm_wide_bwd(*bargs, ws=ws))]
        for op, passes, old, new in rows:
            for fn in (old, new):
                for _ in range(WARM):
                    fn()
            calls = int(min(max(WINDOW_MS / window(ctx, old, 1), WINDOW_MIN), WINDOW_MAX))
            t_old, t_new = [], []
            for _ in range(REPS):
                t_old.append(window(ctx, old, calls))
                t_new.append(window(ctx, new, calls))
            mo, mn = float(np.median(t_old)), float(np.median(t_new))
            gb = passes * 4.0 * int(np.prod(shape)) / 1e9
            print("%-24s %9d %-4s %10.1f %10.1f %8.2f %9.1f %9.1f %6.1f%%  %d"
                  % (shape, int(np.prod(shape)) // C, op, mo * 1e3, mn * 1e3, mo / mn, gb / (mo * 1e-3),
                     gb / (mn * 1e-3), 100 * (max(t_new) - min(t_new)) / mn,
                     ctx.batchnorm_wide_choice(shape)['slabs']), flush=True)


if __name__ == "__main__":
    main()
