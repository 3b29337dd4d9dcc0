"""What the weighted MultinoulliNLL costs per training step: neuro3d_lite at 183^2 with
class_weights=[1, 4], both lazy-labelling masks and example weights against the unweighted step
of the same build, interleaved on one box (HIP-event device time per step, the median of each
block of steps).  Run by hand on one MI355X:

    python tools/weighted_step_bench.py [steps=40] [rounds=3]

Under `rocprofv3 --kernel-trace --stats -- python tools/weighted_step_bench.py 20 1` the per-kernel
side of it is the difference between tail_kernel<2, 2, 16, false> and tail_w_kernel<2, 2, 16>."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SPEC = [(20, (1, 4, 4), (1, 2, 2)), (40, (3, 3, 3), (1, 2, 2)), (150, (2, 4, 4), (2, 1, 1)),
        (200, (1, 3, 3), (1, 1, 1)), (200, (1, 3, 3), (1, 1, 1)), (200, (1, 1, 1), (1, 1, 1))]
SP = (23, 183, 183)


def build(weighted, name):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.newmodel(name)
    np.random.seed(1)
    inp = nm.Input((1, 1) + SP, 'b,f,z,x,y', name='raw')
    out = inp
    for n_f, k, p in SPEC:
        out = nm.Conv(out, n_f, k, p)
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin')
    probs = nm.Softmax(out)
    target = nm.Input_like(probs, override_f=1, name='target')
    kw = {}
    if weighted:
        osp = tuple(probs.shape.spatial_shape)
        kw = dict(class_weights=[1.0, 4.0],
                  example_weights=nm.Input((1,) + osp, 'b,z,x,y', name='ew'),
                  mask_class_labeled=nm.Input((1, 2), 'b,f', name='ll'),
                  mask_class_not_present=nm.Input((1, 2), 'b,f', name='np'))
    loss = nm.AggregateLoss(nm.MultinoulliNLL(probs, target, target_is_sparse=True, **kw),
                            name='loss')
    m = nm.model_manager.current
    m.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=probs)
    m.set_opt_meta_params('Adam', dict(lr=5e-4, mom=0.9, beta2=0.999, wd=0.5e-4))
    rng = np.random.RandomState(0)
    osp = tuple(probs.shape.spatial_shape)
    args = [rng.rand(1, 1, *SP).astype(np.float32),
            rng.randint(0, 2, (1, 1) + osp).astype(np.float32)]
    if weighted:
        args += [(0.5 + rng.rand(1, *osp)).astype(np.float32), np.array([[1, 1]], np.float32),
                 np.array([[0, 1]], np.float32)]
    return m, args


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    # (a second unweighted model: what two plans of the SAME net differ by on this box)
    nets = [("unweighted",) + build(False, 'plain'), ("unweighted2",) + build(False, 'plain2'),
            ("weighted",) + build(True, 'weighted')]
    for _, m, args in nets:                    # eager step, capture, a few replays
        for _ in range(8):
            m.trainingstep(*args, optimiser='Adam')
    med = {k: [] for k, _, _ in nets}
    for r in range(rounds):
        for k, m, args in nets:
            ts = [m.trainingstep(*args, optimiser='Adam')[1] for _ in range(steps)]
            med[k].append(float(np.median(ts)) * 1e3)
            print("round %d %-10s median %.4f ms  min %.4f ms" % (r, k, med[k][-1], min(ts) * 1e3))
    u, w, u2 = np.array(med["unweighted"]), np.array(med["weighted"]), np.array(med["unweighted2"])
    print("two unweighted plans of the same net: %.4f vs %.4f ms (%+.1f us)"
          % (u.mean(), u2.mean(), (u2.mean() - u.mean()) * 1e3))
    print("unweighted %.4f ms (spread of the rounds %.4f), weighted %.4f ms (spread %.4f): delta %+.1f us / step"
          % (u.mean(), u.max() - u.min(), w.mean(), w.max() - w.min(), (w.mean() - u.mean()) * 1e3))
    plan = nets[2][1].optimisers['Adam'].step.func
    nll = [n for n in plan.nodes if type(n).__name__ == 'MultinoulliNLL'][0]
    print("weighted plan: tail launch %s" % ((nll, 'tail_slots') in plan.scratch))


if __name__ == "__main__":
    main()
