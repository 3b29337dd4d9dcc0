"""Times the target forms of PatchSampler.getbatch (csrc/targets.hip) at the target geometry of
neuro3d_lite on (1, 1, 23, 183, 183): target patch (19, 145, 145), strides (2, 4, 4) -> (10, 37, 37).

  * wall time per ``getbatch(1, 'train', affinities='affinity')`` with the three unit edges and
    with one edge, and per ``RingFeeder.fill`` (k = 4 slots) with the one-edge arguments --
    neuro3d_lite's target slot has one feature, so the ring takes a one-edge affinity target;
    a host clock around ``batch`` calls that ends in a device synchronise, ``reps`` such windows
    after a warm-up; median, minimum and maximum per call;
  * the plain ``getbatch(1, 'train')`` is timed TWICE, before and after -- the difference of its
    two medians is the run-to-run spread the other figures have to be read against;
  * where the library has them, the device time of each new launch between two HIP events
    around ``batch`` back-to-back launches: e2_count_negative, e2_target_stride,
    e2_target_nhood (7 edges), e2_target_affinity (3 edges) on the (1, 1, 19, 145, 145) patch, and
    e2_ids2barriers on a (64, 256, 256) volume.

The tool runs unchanged on a tree without csrc/targets.hip (there the affinity target is made on
the host and the launch rows are absent), so that both can be measured in one session.

Run by hand on one MI355X:   python tools/targets_bench.py [reps=30] [batch=10]
Human-readable lines go to stderr, ONE JSON line to stdout."""
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

PS, STRIDES, OFFSETS = (23, 183, 183), (2, 4, 4), (2, 19, 19)
NH3 = np.array([[-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.int32)
NH1 = NH3[2:]
NH7 = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]],
               np.int32)


def id_volume(shape, rng):
    """ids 0..5 in (4, 8, 8) blocks: neighbours mostly agree, as in a segmentation"""
    coarse = rng.randint(0, 6, tuple((n + 7) // 4 for n in shape))
    v = np.repeat(np.repeat(np.repeat(coarse, 4, 0), 8, 1), 8, 2)
    return v[:shape[0], :shape[1], :shape[2]].astype(np.float32)


def main():
    import torch
    from elektronn2_amd import nets, neuromancer as nm
    from elektronn2_amd.data import PatchSampler, RingFeeder
    from elektronn2_amd.neuromancer.plan import get_ctx
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    assert reps >= 20
    assert torch.cuda.is_available(), "targets_bench measures on the GPU only"
    ctx = get_ctx()
    stream = ctx.stream

    def say(*a):
        print(*a, file=sys.stderr)

    def stats(ts):
        return dict(median_us=float(np.median(ts)), min_us=float(min(ts)), max_us=float(max(ts)))

    def wall(fn, per=batch):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(per):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / per * 1e6)
        return stats(ts)

    def device(fn):
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
            ts.append(e0.elapsed_time(e1) / batch * 1e3)
        return stats(ts)

    rng = np.random.RandomState(0)
    vsh = (48, 320, 320)
    vol = rng.rand(1, *vsh).astype(np.float32)
    ids = id_volume(vsh, rng)[None]
    smp = PatchSampler([vol], [ids], PS, STRIDES, OFFSETS, seed=0)
    kw = dict(grey_augment_channels=[0], warp=0.5)
    r = dict(tool="targets_bench", reps=reps, batch=batch, device_side=hasattr(ctx, 'target_affinity'),
             patch=list(PS), target_patch=list(smp.target_ps), strides=list(STRIDES))
    r['plain_a'] = wall(lambda: smp.getbatch(1, 'train', **kw))
    r['affinity_3'] = wall(lambda: smp.getbatch(1, 'train', affinities='affinity', nhood=NH3, **kw))
    r['affinity_1'] = wall(lambda: smp.getbatch(1, 'train', affinities='affinity', nhood=NH1, **kw))

    nm.model_manager.reset()
    np.random.seed(0)
    model = nets.neuro3d_lite((None, 1) + PS)
    model.set_opt_meta_params('Adam', dict(lr=5e-4, mom=0.9, beta2=0.999, wd=0.5e-4))
    d, a = smp.getbatch(1, 'train', affinities='affinity', nhood=NH1, **kw)
    model.trainingstep(d, a, optimiser='Adam')
    k = 4
    feeder = RingFeeder(smp, model, 'Adam', k, affinities='affinity', nhood=NH1, **kw)
    r['fill_k'] = k
    r['fill_affinity_1'] = wall(feeder.fill, per=max(1, batch // k))
    r['plain_b'] = wall(lambda: smp.getbatch(1, 'train', **kw))
    pa, pb = r['plain_a']['median_us'], r['plain_b']['median_us']
    r['plain_spread'] = abs(pa - pb) / (0.5 * (pa + pb))
    for key in ('plain_a', 'affinity_3', 'affinity_1', 'fill_affinity_1', 'plain_b'):
        say("%-16s wall per call: median %.1f us (min %.1f, max %.1f)"
            % (key, r[key]['median_us'], r[key]['min_us'], r[key]['max_us']))
    say("plain getbatch, before / after: spread %.1f %%" % (100 * r['plain_spread']))

    if r['device_side']:
        t = smp.getbatch(1, 'train', force_dense=True)[1]
        sp = tuple(-(-n // s) for n, s in zip(smp.target_ps, STRIDES))
        out = lambda c: torch.empty((1, c) + sp, device='cuda')
        o1, o3, o7 = out(1), out(3), out(7)
        cnt = torch.zeros(1, dtype=torch.int32, device='cuda')
        bsh = (64, 256, 256)
        bids = torch.tensor(id_volume(bsh, rng), device='cuda')[None, None]
        bout = torch.empty_like(bids)
        launches = dict(
            count_negative=lambda: ctx.count_negative(t, cnt),
            target_stride=lambda: ctx.target_stride(t, STRIDES, o1),
            target_nhood_7=lambda: ctx.target_nhood(t, NH7, STRIDES, o7),
            target_affinity_3=lambda: ctx.target_affinity(t, NH3, STRIDES, o3),
            ids2barriers=lambda: ctx.ids2barriers(bids, (1, 1, 1), (1, 1, 1), 1, bout))
        r['launches'] = {}
        for name, fn in launches.items():
            r['launches'][name] = device(fn)
            say("%-18s device per launch: median %.2f us (min %.2f, max %.2f)"
                % (name, r['launches'][name]['median_us'], r['launches'][name]['min_us'],
                   r['launches'][name]['max_us']))
        r['launch_shapes'] = dict(target=list(t.shape), strided=list(sp), barriers=list(bsh))
    print(json.dumps(r))


if __name__ == "__main__":
    main()
