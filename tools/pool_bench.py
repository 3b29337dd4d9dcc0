"""Times e2_pool3d_lin_fwd / e2_pool3d_lin_bwd (csrc/pool.hip) on the Pool shapes of nets.unet3d and
nets.unet3d_lite at their benchmark patches (read off the built graphs), against the max-pool
kernels e2_maxpool3d_fwd / _bwd on the same tensors in the same process:

  * per Pool node of the two nets: AVG and SUM at pool == stride, and AVG at (3,3,3 | 2,2,2) on the
    same parent (overlapping windows: no yardstick, reported as effective bandwidth);
  * the max yardstick is timed TWICE (before and after the new kernels) -- the difference of its
    two medians is the run-to-run spread a ratio has to be read against;
  * every figure: device time between two HIP events around ``batch`` back-to-back launches,
    ``reps`` such windows after a warm-up; median, minimum and maximum per launch;
  * effective bandwidth = bytes the algorithm has to move / median time:
    forward 4 (V_in + V_out) for both kinds; backward 4 (V_in + V_out) for the linear modes (dout
    read, dx written), 4 (2 V_in + V_out) for max (which also reads x).

Run by hand on one MI355X:   python tools/pool_bench.py [reps=30] [batch=10]
Human-readable lines go to stderr, ONE JSON line to stdout."""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def pool_shapes():
    """[(net, node name, parent's device shape at batch 1, pool)] of every Pool node"""
    from elektronn2_amd import nets, neuromancer as nm
    out = []
    for net in ("unet3d", "unet3d_lite"):
        nm.model_manager.reset()
        m = getattr(nets, net)()
        for node in m.nodes.values():
            if type(node).__name__ == 'Pool':
                sh = tuple(1 if s is None else int(s) for s in node.parent.shape.shape)
                out.append((net, node.name, sh, tuple(node.pool_shape)))
    nm.model_manager.reset()
    return out


def extent(sp, pool, stride):
    return tuple((i - p) // s + 1 for i, p, s in zip(sp, pool, stride))


def main():
    import torch
    from elektronn2_amd import backend
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    assert reps >= 20
    assert torch.cuda.is_available(), "pool_bench measures on the GPU only"
    ctx = backend.Context(0)
    stream = ctx.stream

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(batch):
                fn()
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / batch * 1e3)            # us per launch
        return dict(median_us=float(np.median(ts)), min_us=float(min(ts)), max_us=float(max(ts)))

    def say(*a):
        print(*a, file=sys.stderr)

    rows = []
    for net, name, sh, pool in pool_shapes():
        x = torch.randn(sh, device='cuda')
        v_in = x.numel()
        osh = sh[:2] + extent(sh[2:], pool, pool)
        out, dout, dx = torch.empty(osh, device='cuda'), torch.randn(osh, device='cuda'), torch.empty_like(x)
        v_out = out.numel()
        b_fwd, b_lin_bwd, b_max_bwd = 4 * (v_in + v_out), 4 * (v_in + v_out), 4 * (2 * v_in + v_out)
        r = dict(net=net, node=name, parent=list(sh), pool=list(pool), bytes_fwd=b_fwd,
                 bytes_lin_bwd=b_lin_bwd, bytes_max_bwd=b_max_bwd)
        torch.cuda.synchronize()
        r['max_fwd_a'] = timed(lambda: ctx.maxpool3d_fwd(x, pool, out))
        r['max_bwd_a'] = timed(lambda: ctx.maxpool3d_bwd(dout, x, pool, dx))
        for mode in ('avg', 'sum'):
            r[mode + '_fwd'] = timed(lambda: ctx.pool_lin_fwd(x, pool, pool, mode, out))
            r[mode + '_bwd'] = timed(lambda: ctx.pool_lin_bwd(dout, pool, pool, mode, dx))
        r['max_fwd_b'] = timed(lambda: ctx.maxpool3d_fwd(x, pool, out))
        r['max_bwd_b'] = timed(lambda: ctx.maxpool3d_bwd(dout, x, pool, dx))
        # overlapping windows on the same parent
        op, os_ = (3, 3, 3), (2, 2, 2)
        oosh = sh[:2] + extent(sh[2:], op, os_)
        oout, odout = torch.empty(oosh, device='cuda'), torch.randn(oosh, device='cuda')
        r['overlap_bytes'] = 4 * (v_in + oout.numel())
        r['overlap_fwd'] = timed(lambda: ctx.pool_lin_fwd(x, op, os_, 'avg', oout))
        r['overlap_bwd'] = timed(lambda: ctx.pool_lin_bwd(odout, op, os_, 'avg', dx))
        for d in ('fwd', 'bwd'):
            ya, yb = r['max_%s_a' % d]['median_us'], r['max_%s_b' % d]['median_us']
            y = 0.5 * (ya + yb)
            r['max_%s_spread' % d] = abs(ya - yb) / y
            for mode in ('avg', 'sum'):
                r['%s_%s_over_max' % (mode, d)] = r['%s_%s' % (mode, d)]['median_us'] / y
        tb = lambda nbytes, key: nbytes / (r[key]['median_us'] * 1e-6) / 1e12
        r['tb_s'] = dict(max_fwd=tb(b_fwd, 'max_fwd_a'), avg_fwd=tb(b_fwd, 'avg_fwd'),
                         sum_fwd=tb(b_fwd, 'sum_fwd'), max_bwd=tb(b_max_bwd, 'max_bwd_a'),
                         avg_bwd=tb(b_lin_bwd, 'avg_bwd'), sum_bwd=tb(b_lin_bwd, 'sum_bwd'),
                         overlap_fwd=tb(r['overlap_bytes'], 'overlap_fwd'),
                         overlap_bwd=tb(r['overlap_bytes'], 'overlap_bwd'))
        say("%s %s %s pool %s" % (net, name, sh, pool))
        for d in ('fwd', 'bwd'):
            say("  %s: max %.1f / %.1f us (spread %.1f %%)  avg %.1f us (x%.3f)  sum %.1f us (x%.3f)  "
                "overlap (3,3,3|2,2,2) %.1f us = %.2f TB/s effective"
                % (d, r['max_%s_a' % d]['median_us'], r['max_%s_b' % d]['median_us'],
                   100 * r['max_%s_spread' % d], r['avg_' + d]['median_us'], r['avg_%s_over_max' % d],
                   r['sum_' + d]['median_us'], r['sum_%s_over_max' % d],
                   r['overlap_' + d]['median_us'], r['tb_s']['overlap_' + d]))
        say("  TB/s at the median: %s" % ", ".join("%s %.2f" % kv for kv in sorted(r['tb_s'].items())))
        rows.append(r)
        del x, out, dout, dx, oout, odout
    print(json.dumps(dict(tool="pool_bench", reps=reps, batch=batch, rows=rows)))


if __name__ == "__main__":
    main()
