"""Conv border modes 'same' / 'full' and the Pad node on the GPU (csrc/pad.hip; the valid conv
kernels on a zero-framed image; neural.py:520-530,731-737,1195-1279 and computations.py:287-291,
320-326 of the reference).

The reference of every number is the float64 torch-CPU restatement of tests/test_conv_modes_host.py
(``Ref``: F.conv3d(F.pad(x, q), w.flip(2,3,4)) -> pool -> bias -> activation, the loss as the other
suites restate it, autograd on the float32 inputs the kernels saw; pinned there against
scipy.signal.convolve) -- never the code under test.  Bounds are the project's own: ops 2e-5 of the
reference's largest magnitude (tests/test_ops_gpu.py:16); loss, prediction, every gradient and the
parameters after Adam steps 1e-4 (tests/test_model_gpu.py:17); one route against another 1e-5
(losses) / 1e-4 (parameters).  e2_pad5 moves bits: its results are compared bit for bit."""
import numpy as np
import pytest
import torch

from test_conv_modes_host import Ref, frame_of
from test_dropout_gpu import SHAPES, VIEWS

pytestmark = pytest.mark.gpu
TOL = 2e-5
TOL_STEP = 1e-4
ADAM = dict(lr=5e-4, mom=0.9, beta2=0.999, wd=0.5e-4)


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device='cuda')


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


# ---- A. the e2_pad5 op -----------------------------------------------------------------------------
PADS = [(0, 1, 1), (1, 1, 1), (2, 3, 3), (0, 0, 2)]


@pytest.mark.parametrize("value", [0.0, 1.5])
@pytest.mark.parametrize("pad", PADS, ids=["%d%d%d" % p for p in PADS])
@pytest.mark.parametrize("dview", VIEWS, ids=["dst_" + v[0] for v in VIEWS])
@pytest.mark.parametrize("sview", VIEWS, ids=["src_" + v[0] for v in VIEWS])
def test_pad5_is_numpy_pad_bit_for_bit(ctx, sview, dview, pad, value):
    """dst == numpy.pad(src) bit for bit over SHAPES x VIEWS (source and destination views
    independently); the poisoned memory around the destination view and the whole source storage
    are untouched; the frame-only form leaves the interior's bits alone"""
    rng = np.random.RandomState(17)
    pz, px, py = pad
    for shape in SHAPES:
        x = rng.randn(*shape).astype(np.float32)
        x.flat[::7] = -0.0                                  # (a sign bit a float compare would lose)
        want = np.pad(x, [(0, 0), (0, 0), (pz, pz), (px, px), (py, py)], constant_values=np.float32(value))
        dshape = want.shape
        sstore, sv = sview[1](shape)
        sstore.fill_(-77.0)
        sv.copy_(dev(x))
        sbefore = sstore.clone()
        dstore, dv = dview[1](dshape)
        dstore.fill_(-55.0)
        dbefore = dstore.clone()
        ctx.pad5(sv, dv, pad, value)
        assert np.array_equal(bits(dv.cpu().numpy()), bits(want)), (shape, pad)
        assert torch.equal(sstore, sbefore)
        mstore, mview = dview[1](dshape)                     # same geometry: where the view lies
        mstore.fill_(0); mview.fill_(1)
        outside = mstore == 0
        assert torch.equal(dstore[outside], dbefore[outside]), (shape, pad)
        # frame only: other interior bits stay, the frame is rewritten
        inner = rng.randn(*shape).astype(np.float32)
        dv[:, :, pz:pz + shape[2], px:px + shape[3], py:py + shape[4]].copy_(dev(inner))
        dv_np = dv.cpu().numpy()
        frame = np.ones(dshape, bool)
        frame[:, :, pz:pz + shape[2], px:px + shape[3], py:py + shape[4]] = False
        dv.copy_(torch.where(torch.from_numpy(frame).cuda(), torch.full_like(dv, 9.0), dv))
        ctx.pad5(None, dv, pad, value, frame_only=True)
        want2 = np.where(frame, np.float32(value), dv_np)
        assert np.array_equal(bits(dv.cpu().numpy()), bits(want2)), (shape, pad)
        assert torch.equal(dstore[outside], dbefore[outside]), (shape, pad)


def test_pad5_rejects_mismatched_sizes(ctx):
    from elektronn2_amd import backend
    src = torch.zeros((1, 2, 3, 4, 5), device='cuda')
    with pytest.raises(backend.E2Error, match="e2_pad5"):
        ctx.pad5(src, torch.zeros((1, 2, 3, 6, 8), device='cuda'), (0, 1, 1))
    with pytest.raises(backend.E2Error, match="e2_pad5"):
        ctx.pad5(src, torch.zeros((1, 2, 5, 6, 7), device='cuda'), (1, 1, -1))
    with pytest.raises(backend.E2Error, match="e2_pad5"):
        ctx.pad5(None, torch.zeros((1, 2, 2, 6, 7), device='cuda'), (1, 1, 1), frame_only=True)


# ---- B. one non-valid conv behind each kind of parent ----------------------------------------------
def _finish(nm, inp, logits):
    probs = nm.Softmax(logits)
    target = nm.Input_like(probs, override_f=1, name='target')
    loss = nm.AggregateLoss(nm.MultinoulliNLL(probs, target, target_is_sparse=True), name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=probs,
                          prediction_ext=[loss, probs])
    model.set_opt_meta_params('Adam', ADAM)
    return model


def _fit(base, k, pool, mode, even=False):
    """the smallest extents >= base that the conv can pool: (s + border) % p == 0 per axis
    (``even``: and x / y even, for a merge with a once-pooled branch)"""
    out = []
    for i, (s, f, p) in enumerate(zip(base, k, pool)):
        b = {'valid': 1 - f, 'same': 0, 'full': f - 1}[mode]
        for s in range(s, s + 8):
            if (s + b) % p == 0 and s + b > 0 and not (even and i > 0 and s % 2):
                break
        else:
            raise ValueError("no extent for kernel %d, pool %d, mode %s" % (f, p, mode))
        out.append(s)
    return tuple(out)


PARENTS = ['input', 'input1', 'conv_generic', 'conv_fused', 'pool', 'merge', 'crop']
# which parents hand their output over in place (no pad launch) -- listed in the PR description
IN_PLACE = {'input': False, 'input1': False, 'conv_generic': True, 'conv_fused': False,
            'pool': True, 'merge': True, 'crop': False}


def single_net(parent, mode, k, pool, act, bn=False, seed=41):
    """<parent> -> Conv(k, pool, conv_mode=mode, act) -> (1,..) 'lin' head; ``k`` with two entries
    builds the 2-D form ('b,f,y,x')"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    nd = len(k)
    one, k3 = (1,) * nd, (1, 3, 3)[3 - nd:]
    tags = 'b,f,z,x,y' if nd == 3 else 'b,f,y,x'
    # extents of the tensor the conv under test reads
    base = (80, 12, 12) if parent == 'conv_fused' else ((5, 10, 12) if nd == 3 else (10, 12))
    s = _fit(base, k, pool, mode, even=(parent == 'merge'))
    grow = lambda sp, d: tuple(a + b for a, b in zip(sp, d))
    if parent in ('input', 'input1'):
        inp = nm.Input((1, 2 if parent == 'input' else 1) + s, tags, name='raw')
        par = inp
    elif parent in ('conv_generic', 'conv_fused'):
        inp = nm.Input((1, 2) + grow(s, (0, 2, 2)[3 - nd:]), tags, name='raw')
        par = nm.Conv(inp, 4, k3, name='parent')
    elif parent == 'pool':
        inp = nm.Input((1, 2) + (s[0], 2 * s[1] + 2, 2 * s[2] + 2), tags, name='raw')
        par = nm.Pool(nm.Conv(inp, 4, k3, name='parent'), (1, 2, 2))
    elif parent == 'merge':
        # skip branch (s) with a Crop; low branch pooled once, one conv, UpConv back up
        inp = nm.Input((1, 2) + grow(s, (0, 6, 6)), tags, name='raw')
        c1 = nm.Conv(inp, 4, k3, name='parent')                        # s + (0, 4, 4)
        lo = nm.Conv(nm.Pool(c1, (1, 2, 2)), 5, k3, name='low')        # s / 2
        par = nm.UpConvMerge(c1, lo, 3)                                 # crop c1 by (0, 2, 2)
    elif parent == 'crop':
        inp = nm.Input((1, 2) + grow(s, (0, 4, 4)), tags, name='raw')
        par = nm.Crop(nm.Conv(inp, 4, k3, name='parent'), (0, 1, 1))
    else:
        raise ValueError(parent)
    out = nm.Conv(par, 5, k, pool, conv_mode=mode, activation_func=act,
                  batch_normalisation='train' if bn else False, name='probe')
    hk = one
    if parent == 'merge':
        # input - output extent must be even per axis (model.py:141-152): a head of extent 2 where
        # the probe's border leaves it odd
        diff = [a - b for a, b in zip(inp.shape.spatial_shape, out.shape.spatial_shape)]
        hk = tuple(2 if d % 2 else 1 for d in diff)
    out = nm.Conv(out, 2, hk, activation_func='lin', name='head')
    return _finish(nm, inp, out)


def batch_for(model, seed, n_class=2):
    rng = np.random.RandomState(seed)
    x = rng.rand(*model.input_node.shape.shape).astype(np.float32)
    t = rng.randint(0, n_class, model.target_node.shape.shape).astype(np.float32)
    t.flat[::17] = -1                          # unlabelled voxels
    return x, t


KERNELS = [('same', (1, 3, 3)), ('same', (3, 3, 3)), ('same', (1, 5, 5)), ('same', (3, 1, 1)),
           ('full', (1, 3, 3)), ('full', (3, 3, 3)), ('full', (1, 5, 5)), ('full', (3, 1, 1)),
           ('full', (2, 4, 4))]


def _cases():
    """every parent x every (mode, kernel); pools (1,1,1) / (1,2,2) and relu / tanh alternate so
    that each parent and each kernel meets both; 2-D (3,3) behind the parents that exist in 2-D;
    batch normalisation once per mode"""
    out = []
    for i, parent in enumerate(PARENTS):
        for j, (mode, k) in enumerate(KERNELS):
            pool = (1, 2, 2) if (i + j) % 2 else (1, 1, 1)
            if parent == 'merge':
                # (a net with an UpConv takes its fov from input - output extent, which must be
                # even per axis -- model.py:141-152: behind the merge of this net no border
                # admits a pooled probe; Pool -> pooled probe and the U-Net of C cover pooling)
                pool = (1, 1, 1)
            act = 'tanh' if ((i + j) // 2) % 2 else 'relu'
            out.append((parent, mode, k, pool, act, False))
    for parent in ('input', 'conv_generic'):
        for j, mode in enumerate(('same', 'full')):
            out.append((parent, mode, (3, 3), (2, 2) if j else (1, 1), 'relu' if j else 'tanh', False))
    out.append(('pool', 'same', (3, 3, 3), (1, 2, 2), 'relu', True))
    out.append(('conv_generic', 'full', (1, 3, 3), (1, 1, 1), 'tanh', True))
    return out


CASES = _cases()


def _case_id(c):
    return "%s-%s-%s-p%s-%s%s" % (c[0], c[1], "x".join(map(str, c[2])), "".join(map(str, c[3])), c[4],
                                  "-bn" if c[5] else "")


def check_loss_and_grads(m, x, t, what=""):
    ref = Ref(m)
    lref, pref = ref.loss_and_grads(x, t)
    loss = float(m.loss(x, t))
    e_l = abs(loss - lref) / abs(lref)
    got = m.gradients(x, t)
    names = list(m.loss_node.all_trainable_params.keys())
    want = ref.grads()
    assert len(got) == len(want) == len(names)
    errs = dict((nme, rel(g, w)) for nme, g, w in zip(names, got, want))
    print("%s: loss %.7f ref %.7f (%.1e); gradients worst %s"
          % (what, loss, lref, e_l, sorted(errs.items(), key=lambda kv: -kv[1])[:3]))
    assert e_l < TOL_STEP, (loss, lref)
    for nme, w in zip(names, want):
        assert np.abs(w).max() > 0, nme
        assert errs[nme] < TOL_STEP, (nme, errs[nme])
    return ref


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_single_conv_behind_each_parent(case):
    """loss and ALL gradients -- the parent conv's among them, which only the interior's data
    gradient reaches -- against float64; and the route the framed image took"""
    parent, mode, k, pool, act, bn = case
    m = single_net(parent, mode, k, pool, act, bn)
    x, t = batch_for(m, 43)
    check_loss_and_grads(m, x, t, _case_id(case))
    plan = m._grad_func.func
    probe = m.nodes['probe']
    assert tuple(probe._q3)[3 - len(k):] == frame_of(mode, k)
    assert (probe, 'xf') in plan.scratch
    assert ((probe, 'xf_launch') not in plan.scratch) == IN_PLACE[parent], parent
    if parent in ('conv_generic', 'conv_fused'):
        assert m.nodes['parent']._fused_act(plan) == (parent == 'conv_fused')


# ---- C. whole steps, batch 2 -----------------------------------------------------------------------
def net_unet_same(batch=2, seed=51, mode='same', sp=(4, 16, 16)):
    """two levels, UpConvMerge, every Conv in 'same' mode: prediction extent == input extent"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 1) + tuple(sp), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 6, (1, 3, 3), conv_mode=mode)
    c1 = nm.Conv(c0, 6, (3, 3, 3), conv_mode=mode)
    p1 = nm.Pool(c1, (1, 2, 2))
    c2 = nm.Conv(p1, 8, (3, 3, 3), conv_mode=mode)
    c3 = nm.Conv(c2, 8, (1, 3, 3), conv_mode=mode, activation_func='tanh')
    mrg = nm.UpConvMerge(c1, c3, 8)
    c4 = nm.Conv(mrg, 6, (3, 3, 3), conv_mode=mode)
    out = nm.Conv(c4, 2, (1, 1, 1), activation_func='lin', conv_mode=mode)
    return _finish(nm, inp, out)


def net_full2(batch=2, seed=52):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 2, 4, 9, 9), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 4, (2, 4, 4), (1, 2, 2), conv_mode='full')         # (5, 6, 6)
    out = nm.Conv(out, 5, (1, 3, 3), conv_mode='full', activation_func='tanh')   # (5, 8, 8)
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin')
    return _finish(nm, inp, out)


def net_mixed(batch=2, seed=53, value=0.0):
    """all three modes, a Pad in front of the valid conv"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 1, 5, 14, 14), 'b,f,z,x,y', name='raw')
    a = nm.Conv(inp, 4, (1, 3, 3), conv_mode='same', activation_func='tanh')     # (5, 14, 14)
    b = nm.Conv(a, 5, (3, 3, 3), (1, 2, 2), conv_mode='full')                    # (7, 8, 8)
    pd = nm.Pad(b, (1, 0, 2), value=value)                                       # (9, 8, 12)
    c = nm.Conv(pd, 6, (3, 3, 3), conv_mode='valid')                             # (7, 6, 10)
    out = nm.Conv(c, 2, (1, 1, 1), activation_func='lin')
    return _finish(nm, inp, out)


NETS = [("unet_same", net_unet_same, 61), ("full2", net_full2, 62), ("mixed", net_mixed, 63)]


@pytest.mark.parametrize("name,make,data_seed", NETS, ids=[n[0] for n in NETS])
def test_whole_steps_against_float64(name, make, data_seed):
    """batch 2: loss, prediction, every gradient (eager, captured, replayed), then the parameters
    after each of 3 Adam steps"""
    m = make()
    x, t = batch_for(m, data_seed)
    assert x.shape[0] == 2
    ref = None
    for call in range(3):
        ref = check_loss_and_grads(m, x, t, "%s call %d" % (name, call))
        e = rel(m.predict(x), ref.predict(x))
        print("%s call %d: prediction %.2e" % (name, call, e))
        assert e < TOL_STEP
    for step in range(3):
        lref, _ = ref.loss_and_grads(x, t)
        ref.adam(**ADAM)
        loss = float(m.trainingstep(x, t, optimiser='Adam')[0])
        assert abs(loss - lref) / abs(lref) < TOL_STEP, (step, loss, lref)
        worst = ('', 0.0)
        for nme, p in m.loss_node.all_trainable_params.items():
            e = rel(p.get_value(), ref.p(p).detach().numpy())
            worst = max(worst, (nme, e), key=lambda kv: kv[1])
            assert e < TOL_STEP, (step, nme, e)
        print("%s step %d: loss %.7f ref %.7f, parameters worst %s" % (name, step, loss, lref, worst))


# ---- D. route equivalences -------------------------------------------------------------------------
def _steps(m, x, t, n=3):
    losses = [float(m.trainingstep(x, t, optimiser='Adam')[0]) for _ in range(n)]
    return losses, [p.get_value() for p in m.loss_node.all_trainable_params.values()]


def _same_routes(a, b):
    for u, v in zip(a[0], b[0]):
        assert abs(u - v) < 1e-5 * abs(v), (a[0], b[0])
    assert len(a[1]) == len(b[1])
    for u, v in zip(a[1], b[1]):
        assert rel(u, v) < 1e-4


def test_same_conv_equals_pad_node_plus_valid_conv():
    from elektronn2_amd import neuromancer as nm

    def build(explicit):
        nm.model_manager.reset()
        np.random.seed(71)
        inp = nm.Input((1, 2, 5, 10, 12), 'b,f,z,x,y', name='raw')
        h = nm.Conv(inp, 4, (1, 3, 3), name='parent')
        if explicit:
            h = nm.Conv(nm.Pad(h, (1, 2, 1)), 5, (3, 5, 3), (1, 2, 2), conv_mode='valid', name='probe')
        else:
            h = nm.Conv(h, 5, (3, 5, 3), (1, 2, 2), conv_mode='same', name='probe')
        return _finish(nm, inp, nm.Conv(h, 2, (1, 1, 1), activation_func='lin', name='head'))
    a, b = build(False), build(True)
    for pa, pb in zip(a.trainable_params, b.trainable_params):
        pb.set_value(pa.get_value())                        # shared weight VALUES
    x, t = batch_for(a, 72)
    assert abs(float(a.loss(x, t)) - float(b.loss(x, t))) < 1e-5 * abs(float(b.loss(x, t)))
    assert rel(a.predict(x), b.predict(x)) < 1e-5
    for ga, gb in zip(a.gradients(x, t), b.gradients(x, t)):
        assert rel(ga, gb) < 1e-4
    _same_routes(_steps(a, x, t), _steps(b, x, t))


def test_pad_inplace_on_equals_off():
    from elektronn2_amd.neuromancer import plan_options
    res = {}
    for on in (True, False):
        with plan_options(pad_inplace=on):
            m = net_unet_same()
            x, t = batch_for(m, 61)
            res[on] = _steps(m, x, t)
            plan = m.optimisers['Adam'].step.func
            n_launch = sum(1 for k_ in plan.scratch if isinstance(k_, tuple) and len(k_) == 2
                           and k_[1] == 'xf_launch')
            n_framed = sum(1 for k_ in plan.scratch if isinstance(k_, tuple) and len(k_) == 2
                           and k_[1] == 'xf')
            print("pad_inplace=%s: %d framed convs, %d pad launches" % (on, n_framed, n_launch))
            # five convs with a border.  In place: the three behind the Pool, a Conv on its
            # pooling / activation pass and the Concat; by launch: the one that reads the Input
            # node and the one behind it, whose parent is the fused first layer
            by_launch = sorted(k_[0].name for k_ in plan.scratch if isinstance(k_, tuple)
                               and len(k_) == 2 and k_[1] == 'xf_launch')
            assert n_framed == 5
            assert m.nodes['conv']._fused_first(plan)
            assert by_launch == (['conv', 'conv1'] if on else ['conv', 'conv1', 'conv2', 'conv3', 'conv4'])
    _same_routes(res[True], res[False])


def test_graph_replay_equals_eager():
    from elektronn2_amd.neuromancer import plan_options
    res = {}
    for graph in (True, False):
        with plan_options(graph=graph):
            m = net_mixed()
            x, t = batch_for(m, 63)
            res[graph] = _steps(m, x, t, 4)
            assert m.optimisers['Adam'].step.func.use_graph == graph
    _same_routes(res[True], res[False])


def test_several_steps_in_one_graph_equal_single_steps():
    m0 = net_unet_same()
    x, t = batch_for(m0, 61)

    def fresh():
        mm = net_unet_same()
        for _ in range(2):
            mm.trainingstep(x, t, optimiser='Adam')
        return mm
    a = fresh()
    single = [float(a.trainingstep(x, t, optimiser='Adam')[0]) for _ in range(4)]
    b = fresh()
    pl = b.optimisers['Adam'].step.func
    ring = torch.empty((3, pl.input_arena.numel()), device='cuda')
    ring[:] = pl.input_arena
    losses, tsec = b.trainingsteps(4, optimiser='Adam', ring=ring)
    assert len(losses) == 4
    for u, v in zip(single, losses):
        assert abs(u - float(v)) / abs(u) < 1e-5, (single, list(losses))
    for pa, pb in zip(a.loss_node.all_trainable_params.values(), b.loss_node.all_trainable_params.values()):
        assert rel(pb.get_value(), pa.get_value()) < 1e-4


def test_pad_node_with_a_value_against_the_restatement():
    m = net_mixed(batch=1, value=1.5)
    x, t = batch_for(m, 64)
    ref = check_loss_and_grads(m, x, t, "pad value 1.5")
    assert rel(m.predict(x), ref.predict(x)) < TOL_STEP
    # the Pad node's own output, as an op: bit-equal to numpy.pad of its parent's output
    pd = [n for n in m.nodes.values() if type(n).__name__ == 'Pad'][0]
    got, src = pd(x), pd.parent(x)
    want = np.pad(src, [(0, 0), (0, 0), (1, 1), (0, 0), (2, 2)], constant_values=np.float32(1.5))
    assert np.array_equal(bits(got), bits(want))


# ---- E. launch count -------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["pool", "merge"])
def test_in_place_chains_issue_no_pad_launch(chain, monkeypatch):
    from elektronn2_amd.neuromancer import plan_options, plan as plan_mod
    c = plan_mod.get_ctx()
    calls = []
    orig = c.pad5
    monkeypatch.setattr(c, 'pad5', lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    for on, want in ((True, 0), (False, 1)):
        with plan_options(graph=False, pad_inplace=on):
            m = single_net(chain, 'same', (3, 3, 3), (1, 1, 1), 'relu')
            x, t = batch_for(m, 43)
            m.trainingstep(x, t, optimiser='Adam')           # builds the plan
            del calls[:]
            m.trainingstep(x, t, optimiser='Adam')           # ONE eager step
            assert m.optimisers['Adam'].step.func.use_graph is False
            assert len(calls) == want, (chain, on, len(calls))


# ---- F. bf16 mode ----------------------------------------------------------------------------------
@pytest.fixture()
def process_bf16():
    import elektronn2_amd
    elektronn2_amd.set_mfma_dtype('bf16')
    yield
    elektronn2_amd.set_mfma_dtype('f32')


def test_bf16_step_of_the_same_mode_unet(process_bf16):
    """one step of the small same-mode U-Net with bf16 operands in the conv GEMMs against the
    float64 evaluation of the f32 net, at the bounds of the suite's bf16 step of a net of this depth
    (tests/test_bf16_gpu.py::test_training_step_bf16_close_to_f32_oracle, seven layers): loss within
    1e-2 and not the f32 result, every gradient tensor within 0.1 of its largest element and at a
    cosine above 0.995; the step then runs and stays finite"""
    m = net_unet_same(sp=(4, 32, 32))
    x, t = batch_for(m, 66)            # (seed chosen on the reference alone: Ref's MIN_PRE holds)
    ref = Ref(m)
    lref, _ = ref.loss_and_grads(x, t)
    loss = float(m.loss(x, t))
    print("bf16 same-mode U-Net: loss %.7f ref %.7f" % (loss, lref))
    assert abs(loss - lref) < 1e-2 * abs(lref)
    assert abs(loss - lref) > 1e-7 * abs(lref)              # not the f32 path
    got = m.gradients(x, t)
    for nme, g, w in zip(m.loss_node.all_trainable_params.keys(), got, ref.grads()):
        e = float(np.abs(g - w).max() / np.abs(w).max())
        cos = float((g * w).sum() / np.sqrt((g.astype(np.float64) ** 2).sum() * (w * w).sum() + 1e-300))
        print("%-14s max-element error %.4f, cosine %.6f" % (nme, e, cos))
        assert e < 0.1, (nme, e)
        assert cos > 0.995, (nme, cos)
    losses = [float(m.trainingstep(x, t, optimiser='Adam')[0]) for _ in range(3)]
    assert np.isfinite(losses).all()


# ---- G. prediction and rejections ------------------------------------------------------------------
def test_prediction_has_the_inputs_extent_and_rewrites_are_rejected(tmp_path):
    from elektronn2_amd import neuromancer as nm
    m = net_unet_same(batch=1)
    x, t = batch_for(m, 61)
    ref = Ref(m)
    pred = m.predict(x)
    assert pred.shape[2:] == x.shape[2:] and pred.shape[1] == 2
    assert rel(pred, ref.predict(x)) < TOL_STEP
    lref, _ = ref.loss_and_grads(x, t)
    ext = m.predict_ext(x, t)
    assert abs(float(ext[0]) - lref) < TOL_STEP * abs(lref)
    assert rel(ext[-1], ref.predict(x)) < TOL_STEP
    assert rel(m.nodes['conv1'](x), ref.forward(x, upto=m.nodes['conv1']).detach().numpy()) < TOL_STEP
    with pytest.raises(NotImplementedError, match="same"):
        m.predict_dense(np.zeros((1, 8, 40, 40), np.float32))
    f = str(tmp_path / "same_unet.mdl")
    m.save(f)
    m2 = nm.modelload(f, name='reloaded')
    assert np.array_equal(bits(m2.predict(x)), bits(pred))
    with pytest.raises(NotImplementedError, match="same"):
        nm.modelload(f, name='mfp', override_mfp_to_active=True)
    with pytest.raises(NotImplementedError, match="full"):
        nm.Conv(m2.input_node, 4, (1, 3, 3), (1, 2, 2), conv_mode='full', mfp=True)
