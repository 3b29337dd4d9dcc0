"""tanh / sigmoid / abs / elu / selu / soft+ on the GPU (csrc/act.hip; computations.py:57-134).

The reference of every comparison is the float64 restatement of tests/test_activations_host.py
(``act_f`` / ``act_df``, checked there against torch-CPU) on the float32 inputs the kernel saw, and
float64 torch-CPU autograd of the nets with it -- never the kernels.  Bounds are the project's own:
ops at 2e-5 max-norm relative (tests/test_ops_gpu.py:16); loss, prediction, every gradient and the
parameters after Adam steps at 1e-4 (tests/test_model_gpu.py:17); several steps in one graph
against single steps at 1e-5 (losses) / 1e-4 (parameters); MFP against the offset interleave at
max abs 1e-5 (tests/test_mfp_gpu.py:58-62); bf16 mode layer by layer at tests/test_bf16_gpu.py's
2e-5."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import e2_oracle as O
from test_activations_host import act_f, act_df, act_torch, CANON, KINKED, SELU_A, SELU_S
from test_dropout_host import restated_gate
from test_dropout_gpu import VIEWS, SHAPES

pytestmark = pytest.mark.gpu
TOL = 2e-5          # ops
TOL_STEP = 1e-4     # loss, gradients, parameters after an Adam step
ADAM = dict(lr=5e-4, mom=0.9, beta2=0.999, wd=0.5e-4)
NAMES = ['lin', 'relu', 'tanh', 'sigmoid', 'abs', 'elu', 'selu', 'soft+']     # E2_ACT_* 0..7
PLANTED = np.array([0.0, -0.0, 1e-42, -1e-42, 30.0, -30.0, 100.0, -100.0], np.float32)


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device='cuda')


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def planted_input(rng, shape):
    """randn scaled to cover +-8, plus the planted values (as many as the tensor holds; the small
    shapes get them over several draws: the caller loops) at random places; returns (x, places)"""
    x = (rng.randn(*shape) * 2.7).astype(np.float32)
    k = min(PLANTED.size, x.size)
    where = rng.permutation(x.size)[:k]
    what = PLANTED[rng.permutation(PLANTED.size)[:k]]
    x.flat[where] = what
    return x, where


# ---- 1. the op pair through the C ABI ------------------------------------------------------------
@pytest.mark.parametrize("view", VIEWS, ids=[v[0] for v in VIEWS])
@pytest.mark.parametrize("act", NAMES)
def test_fwd_and_bwd_through_the_c_abi(ctx, act, view):
    """forward and backward at 2e-5, with and without bias; in place == src -> dst bit for bit;
    nothing outside a view written; dbias added to a non-zero start, NULL accepted; every output
    and slope finite; the slopes at +-0; relu / lin equal to the (1,1,1) pooling pair"""
    rng = np.random.RandomState(100 + 7 * CANON[act] + len(view[0]))
    code = CANON[act]
    for shape in SHAPES:
        c = shape[1]
        for draw in range(1 if np.prod(shape) >= 8 else 4):
            x, where = planted_input(rng, shape)
            g = rng.randn(*shape).astype(np.float32)
            g[np.abs(g) < 1e-3] = 1.0
            for with_bias in (False, True):
                b = (rng.randn(c) * 0.5).astype(np.float32) if with_bias else None
                bd = dev(b) if with_bias else None
                v32 = x if b is None else (x + b.reshape(1, -1, 1, 1, 1)).astype(np.float32)
                v = v32.astype(np.float64)                   # the value the kernel applied f to
                f_ref, df_ref = act_f(act, v), act_df(act, v)
                # ---- forward: strided view -> dense, then in place on the view
                store, xv = view[1](shape)
                store.fill_(-77.0)
                xv.copy_(dev(x))
                before = store.clone()
                out = torch.full(shape, 5.0, device='cuda')
                ctx.act_fwd(xv, bd, act, out)
                got = out.cpu().numpy()
                assert np.all(np.isfinite(got)), (shape, act)
                assert rel(got, f_ref) < TOL, (shape, act, with_bias, rel(got, f_ref))
                assert torch.equal(store, before)            # (the source view is only read)
                ctx.act_fwd(xv, bd, act, xv)                 # in place, strided
                assert np.array_equal(bits(xv.cpu().numpy()), bits(got)), (shape, act)
                mstore, mview = view[1](shape)               # same geometry: where the view lies
                mstore.fill_(0); mview.fill_(1)
                outside = mstore == 0
                assert torch.equal(store[outside], before[outside]), shape
                # ---- backward: dout and pre through views, dpre dense; then in place on dout
                xv.copy_(dev(x))
                gstore, gv = view[1](shape)
                gstore.fill_(-55.0)
                gv.copy_(dev(g))
                gbefore = gstore.clone()
                db0 = rng.randn(c).astype(np.float32)
                db = dev(db0)
                dpre = torch.full(shape, 3.0, device='cuda')
                ctx.act_bwd(gv, xv, bd, act, dpre, db)
                dgot = dpre.cpu().numpy()
                d_ref = g.astype(np.float64) * df_ref
                assert np.all(np.isfinite(dgot)), (shape, act)
                assert rel(dgot, d_ref) < TOL, (shape, act, with_bias, rel(dgot, d_ref))
                assert rel(db.cpu().numpy(), db0.astype(np.float64) + d_ref.sum(axis=(0, 2, 3, 4))) < TOL, (shape, act)
                assert np.array_equal(bits(xv.cpu().numpy()), bits(x)) and torch.equal(gstore, gbefore)
                ctx.act_bwd(gv, xv, bd, act, gv, None)       # in place on the gradient, no dbias
                assert np.array_equal(bits(gv.cpu().numpy()), bits(dgot)), (shape, act)
                assert torch.equal(gstore[outside], gbefore[outside]), shape
                # ---- the slopes at the planted zeros, from the kernel's own output
                if not with_bias:
                    slope = dgot.ravel()[where] / g.ravel()[where]
                    for s, xv0 in zip(slope, x.ravel()[where]):
                        if xv0 == 0:                         # +0 and -0
                            want = {1: 0.5, 4: 0.0, 5: 1.0, 6: SELU_S * SELU_A}.get(code)
                            if want is not None:
                                # (exact for 0.5, 0 and 1; s * a * e^0 carries the f32 rounding of
                                # two constants, two products and this quotient: < 5 * 2^-24 relative)
                                assert abs(s - want) <= 1e-6 * max(1.0, want), (act, xv0, s, want)
                # ---- relu / lin: the pooling pair with a (1,1,1) window on the same data
                if code in (0, 1) and with_bias:
                    xd, gd = dev(x), dev(g)
                    o2 = torch.empty(shape, device='cuda')
                    ctx.pool_bias_act_fwd(xd, bd, (1, 1, 1), act, o2)
                    assert np.array_equal(bits(o2.cpu().numpy()), bits(got)), (shape, act)
                    d2 = torch.empty(shape, device='cuda')
                    db2 = dev(db0)
                    ctx.pool_bias_act_bwd(gd, xd, bd, (1, 1, 1), act, d2, db2)
                    assert np.array_equal(bits(d2.cpu().numpy()), bits(dgot)), (shape, act)
                    # (the bias gradient is summed in another order: the op bound)
                    assert rel(db2.cpu().numpy(), db.cpu().numpy()) < TOL


def test_unknown_activation_and_mismatched_views_are_errors(ctx):
    from elektronn2_amd import backend
    x = torch.zeros((1, 2, 3, 4, 5), device='cuda')
    y = torch.zeros((1, 2, 3, 4, 6), device='cuda')
    with pytest.raises(backend.E2Error):
        ctx.act_fwd(x, None, 'tanh', y)
    with pytest.raises(backend.E2Error):
        ctx.act_bwd(x, y, None, 'tanh', x, None)
    with pytest.raises(KeyError):
        ctx.act_fwd(x, None, 'prelu', x)
    # the kernels of the fused routes keep refusing the new values
    with pytest.raises(backend.E2Error):
        ctx.pool_bias_act_fwd(x, None, (1, 1, 1), 'tanh', x)


# ---- 2. whole steps against float64 --------------------------------------------------------------
# A unit of a KINKED function (relu, abs, selu: the slope jumps at 0) whose float64 pre-activation
# lies within float32 rounding of zero makes the comparison ill-posed: the f32 pass may take the
# other slope (tests/test_dropout_gpu.py, MIN_PRE).  Every evaluation of the reference asserts that
# no such unit is closer to zero than 1e-6; the data seeds below were chosen with the reference
# alone, on the CPU, so that this holds for every call and step.  No element is exempted.
MIN_PRE = 1e-6


class Ref(object):
    """float64 torch-CPU restatement of a model's graph (conv -> pool -> (BN) + bias -> act ->
    dropout per node) with the activations of test_activations_host.py"""

    def __init__(self, model):
        self.model = model
        self.t = 0
        self.min_pre = np.inf          # smallest |v| of a kinked unit in the last forward
        self.n_kinked = 0
        self.P, self.m, self.s = {}, {}, {}
        for node in model.nodes.values():
            for p in node.params.values():
                if id(p) not in self.P:
                    self.P[id(p)] = torch.tensor(p.get_value().astype(np.float64),
                                                 requires_grad=bool(p.apply_train))
        self.streams = dict((id(n), i) for i, n in enumerate(model.dropout_nodes()))

    def p(self, param):
        return self.P[id(param)]

    def drop(self, node, h, seed, counter):
        if node.params.get('dropout_rate') is None:
            return h
        rate = np.float32(node.dropout_rate.get_value()[0])
        if node._drop_per_feature:
            keep, scale = restated_gate(h.shape[1], rate, seed, counter, self.streams[id(node)])
            keep = keep.reshape((1, -1) + (1,) * (h.dim() - 2))
        else:
            keep, scale = restated_gate(h.numel(), rate, seed, counter, self.streams[id(node)])
            keep = keep.reshape(tuple(h.shape))
        return h * torch.tensor(keep.astype(np.float64) * np.float64(scale))

    def act(self, node, v):
        if CANON[node.activation_func] in KINKED:
            self.min_pre = min(self.min_pre, float(v.detach().abs().min()))
            self.n_kinked += v.numel()
        return act_torch(node.activation_func, v)

    @staticmethod
    def bn(y, g, b, red):
        bsh = [1] * y.dim()
        bsh[1] = -1
        mean = y.mean(dim=red)
        std = torch.sqrt(((y - mean.view(bsh)) ** 2).mean(dim=red)) + 1e-6
        return (g / std).view(bsh) * y + (b - g * mean / std).view(bsh)

    def forward(self, x, t, seed=0, counter=0):
        m = self.model
        self.min_pre, self.n_kinked = np.inf, 0
        val = {}
        for node in m.nodes.values():
            kind = type(node).__name__
            par = node.parent
            if node is m.input_node:
                val[node] = torch.tensor(np.asarray(x, np.float64))
            elif node is m.target_node:
                val[node] = torch.tensor(np.asarray(t, np.float64))
            elif kind in ('Conv', 'UpConv'):
                h, w, b = val[par], self.p(node.w), self.p(node.b)
                nd = h.dim() - 2
                bsh = (1, -1) + (1,) * nd
                if kind == 'UpConv':
                    y = F.conv_transpose3d(h, w.permute(1, 0, 2, 3, 4), stride=tuple(node.pool_shape))
                else:
                    y = (F.conv3d if nd == 3 else F.conv2d)(h, w.flip(*range(2, 2 + nd)))
                    if any(q != 1 for q in node.pool_shape):
                        y = (F.max_pool3d if nd == 3 else F.max_pool2d)(y, tuple(node.pool_shape))
                if node.batch_normalisation == 'train':
                    y = self.bn(y, self.p(node.gamma), b, [i for i in range(y.dim()) if i != 1])
                else:
                    assert not node.batch_normalisation
                    y = y + b.view(bsh)
                val[node] = self.drop(node, self.act(node, y), seed, counter)
            elif kind == 'Perceptron':
                h = val[par].flatten(1) if node.flatten else val[par]
                y = h @ self.p(node.w)
                if node.batch_normalisation == 'train':
                    y = self.bn(y, self.p(node.gamma), self.p(node.b), [0])
                else:
                    assert not node.batch_normalisation
                    y = y + self.p(node.b)
                val[node] = self.drop(node, self.act(node, y), seed, counter)
            elif kind == 'Pool':
                val[node] = F.max_pool3d(val[par], tuple(node.pool_shape))
            elif kind == 'Crop':
                val[node] = val[par][node._slicer()]
            elif kind == 'Concat':
                val[node] = torch.cat([val[q] for q in par], dim=1)
            elif kind == 'Softmax':
                val[node] = torch.softmax(val[par], dim=1)
            elif kind == 'MultinoulliNLL':
                pr, tg = val[par[0]], val[par[1]]
                C = pr.shape[1]
                classes = torch.arange(C, dtype=tg.dtype).view((1, C) + (1,) * (pr.dim() - 2))
                onehot = (tg == classes).to(pr.dtype)
                nll = -(onehot * torch.log(pr + 1e-5)) * pr.numel() / (onehot.sum() + 1e-5) / C
                val[node] = nll.sum(dim=1, keepdim=True)
            elif kind == 'AggregateLoss':
                val[node] = val[par[0] if isinstance(par, (list, tuple)) else par].mean()
            elif kind == 'Errors':
                continue
            else:
                raise NotImplementedError(kind)
        return val[m.loss_node], val[m.prediction_node]

    def loss_and_grads(self, x, t, seed=0, counter=0):
        for v in self.P.values():
            v.grad = None
        loss, probs = self.forward(x, t, seed, counter)
        assert self.min_pre >= MIN_PRE, "ill-posed case: a kinked unit at %.1e (counter %d)" % (self.min_pre, counter)
        loss.backward()
        return float(loss.detach()), probs.detach().numpy()

    def grads(self):
        """in the order of Model.gradients"""
        return [self.p(p).grad.numpy() for p in self.model.trainable_params]

    @torch.no_grad()
    def adam(self, lr, mom, beta2, wd):
        """optimiser.py:273-334, weight decay times the parameter's apply_reg multiplier"""
        self.t += 1
        factor = np.sqrt(1 - beta2 ** self.t) / (1 - mom ** self.t)
        for par in self.model.trainable_params:
            p = self.p(par)
            g = p.grad
            m = self.m.setdefault(id(par), torch.zeros_like(p))
            s = self.s.setdefault(id(par), torch.zeros_like(p))
            m.mul_(mom).add_(g, alpha=1 - mom)
            s.mul_(beta2).addcmul_(g, g, value=1 - beta2)
            reg = par.apply_reg
            reg = float(reg) if (reg and reg is not True) else (1.0 if reg else 0.0)
            p.sub_(lr * (factor * m / torch.sqrt(s + 1e-5) + wd * reg * p))


def _finish(nm, inp, logits):
    probs = nm.Softmax(logits)
    target = nm.Input_like(probs, override_f=1, name='target')
    loss = nm.AggregateLoss(nm.MultinoulliNLL(probs, target, target_is_sparse=True), name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=probs)
    model.set_opt_meta_params('Adam', ADAM)
    return model


def net_convs(acts=('tanh', 'elu', 'selu'), drop=(0, 0, 0), seed=21):
    """(i): a Cin = 1 first layer with pooling, a pooled 3-D conv, a (1,1,1) conv and the 'lin'
    head -- with the default activations the fused first layer, the tail and the head fire"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((1, 1, 7, 47, 47), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 8, (1, 4, 4), (1, 2, 2), activation_func=acts[0], dropout_rate=drop[0])
    out = nm.Conv(out, 12, (3, 3, 3), (1, 2, 2), activation_func=acts[1], dropout_rate=drop[1])
    out = nm.Conv(out, 16, (1, 1, 1), activation_func=acts[2], dropout_rate=drop[2])
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin')
    return _finish(nm, inp, out)


def net_convs_relu():
    return net_convs(acts=('relu', 'relu', 'relu'))


def net_convs_dropout():
    return net_convs(drop=(0.2, 0.3, 0))


def net_unet(seed=22):
    """(ii): 'abs' on the skip branch the Crop reads, 'sigmoid' on the conv that feeds the UpConv,
    a 'tanh' UpConv whose output and gradient are channel slices of the Concat's buffers"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((1, 1, 6, 20, 20), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 8, (1, 3, 3))
    c1 = nm.Conv(c0, 8, (1, 3, 3), activation_func='abs')
    p1 = nm.Pool(c1, (1, 2, 2))
    c2 = nm.Conv(p1, 16, (3, 3, 3))
    c3 = nm.Conv(c2, 16, (3, 3, 3), activation_func='sigmoid')
    mrg = nm.UpConvMerge(c1, c3, 24, upconv_kwargs=dict(activation_func='tanh'))
    c4 = nm.Conv(mrg, 8, (1, 3, 3))
    out = nm.Conv(c4, 2, (1, 1, 1), activation_func='lin')
    return _finish(nm, inp, out)


def net_mnist(bn_perceptron=True, batch=8, seed=23):
    """(iii): 2-D convs with train-mode batch norm and 'soft+'; the first Perceptron 'tanh' with
    batch norm, or 'sigmoid' without"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 1, 26, 26), 'b,f,y,x', name='raw')
    out = nm.Conv(inp, 12, (3, 3), (2, 2), batch_normalisation='train', activation_func='soft+')
    out = nm.Conv(out, 36, (3, 3), (2, 2), batch_normalisation='train', activation_func='soft+')
    out = nm.Conv(out, 64, (3, 3), (1, 1), batch_normalisation='train', activation_func='soft+')
    if bn_perceptron:
        out = nm.Perceptron(out, 200, flatten=True, activation_func='tanh', batch_normalisation='train')
    else:
        out = nm.Perceptron(out, 200, flatten=True, activation_func='sigmoid')
    out = nm.Perceptron(out, 10, activation_func='lin')
    return _finish(nm, inp, out)


def net_mnist_sigmoid():
    return net_mnist(bn_perceptron=False)


def net_fused_epilogue(second='elu', seed=24):
    """(iv): un-pooled convs with enough output tiles (160 planes) for the fused kernels: with
    relu the second conv takes the bias + activation epilogue"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((1, 1, 160, 8, 8), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 4, (1, 3, 3))
    out = nm.Conv(out, 6, (1, 3, 3), activation_func=second)
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin')
    return _finish(nm, inp, out)


def batch_for(model, seed, n_class=2):
    rng = np.random.RandomState(seed)
    x = rng.rand(*model.input_node.shape.shape).astype(np.float32)
    t = rng.randint(0, n_class, model.target_node.shape.shape).astype(np.float32)
    if t.ndim == 5:
        t.flat[::17] = -1                      # unlabelled voxels
    return x, t


# name, constructor, classes, seed of the batch (chosen on the reference alone: see MIN_PRE),
# the activations the net must contain
NETS = [("convs", net_convs, 2, 31, {'tanh', 'elu', 'selu'}),
        ("unet", net_unet, 2, 31, {'abs', 'sigmoid', 'tanh'}),
        ("mnist_bn", net_mnist, 10, 31, {'soft+', 'tanh'}),
        ("mnist_sigmoid", net_mnist_sigmoid, 10, 31, {'soft+', 'sigmoid'}),
        ("fused_epilogue", net_fused_epilogue, 2, 31, {'elu'}),
        ("convs_dropout", net_convs_dropout, 2, 32, {'tanh', 'elu', 'selu'})]


def reference_schedule(m, x, t, seed):
    """the reference side of test_loss_gradients_and_adam_step_against_float64 on its own: every
    evaluation the test makes, with the counters a dropout net uses; returns the smallest |v| of
    a kinked unit over all of them.  (Used on the CPU to choose the data seeds.)"""
    ref = Ref(m)
    worst = np.inf
    drops = bool(m.dropout_nodes())
    try:
        for c in range(9 if drops else 1):
            ref.loss_and_grads(x, t, seed, c)
            worst = min(worst, ref.min_pre)
        for step in range(3):
            ref.loss_and_grads(x, t, seed, 9 + step)
            worst = min(worst, ref.min_pre)
            ref.adam(**ADAM)
    except AssertionError:
        return min(worst, ref.min_pre), ref.n_kinked
    return worst, ref.n_kinked


@pytest.mark.parametrize("name,make,ncls,data_seed,acts", NETS, ids=[n[0] for n in NETS])
def test_loss_gradients_and_adam_step_against_float64(name, make, ncls, data_seed, acts):
    """loss, prediction, EVERY parameter gradient -- eager, captured and replayed calls -- and
    three Adam steps (eager, captured, replayed) against float64 autograd"""
    m = make()
    have = set(n.activation_func for n in m.nodes.values() if hasattr(n, 'activation_func'))
    assert acts <= have, (acts, have)
    x, t = batch_for(m, data_seed, ncls)
    ref = Ref(m)
    seed = 20250 + len(name)
    drops = bool(m.dropout_nodes())
    if drops:
        m.set_dropout_seed(seed)
    counter = lambda: m.dropout_state()['counter'] if drops else 0
    for call in range(3):                                   # eager, capture, replay
        lref, pref = ref.loss_and_grads(x, t, seed, counter())
        loss = float(m.loss(x, t))
        print("%s call %d: loss %.7f ref %.7f (%d kinked units, closest to zero %.1e)"
              % (name, call, loss, lref, ref.n_kinked, ref.min_pre))
        assert abs(loss - lref) / abs(lref) < TOL_STEP, (call, loss, lref)
        lref, pref = ref.loss_and_grads(x, t, seed, counter())
        e = rel(m.predict(x), pref)
        print("%s call %d: prediction %.2e" % (name, call, e))
        assert e < TOL_STEP
        ref.loss_and_grads(x, t, seed, counter())
        got = m.gradients(x, t)
        names = list(m.loss_node.all_trainable_params.keys())
        want = ref.grads()
        assert len(got) == len(want) == len(names)
        errs = dict((nme, rel(g, w)) for nme, g, w in zip(names, got, want))
        print("%s call %d: gradients, worst %s" % (name, call, sorted(errs.items(), key=lambda kv: -kv[1])[:3]))
        for nme, g, w in zip(names, got, want):
            assert np.abs(w).max() > 0, nme
            assert errs[nme] < TOL_STEP, (call, nme, errs[nme])
    for step in range(3):                                   # Adam: eager, captured, replayed
        lref, _ = ref.loss_and_grads(x, t, seed, counter())
        ref.adam(**ADAM)
        loss = float(m.trainingstep(x, t, optimiser='Adam')[0])
        assert abs(loss - lref) / abs(lref) < TOL_STEP, (step, loss, lref)
        worst = ('', 0.0)
        for nme, p in m.loss_node.all_trainable_params.items():
            e = rel(p.get_value(), ref.p(p).detach().numpy())
            worst = max(worst, (nme, e), key=lambda kv: kv[1])
            assert e < TOL_STEP, (step, nme, e)
        print("%s step %d: loss %.7f ref %.7f, parameters worst %s" % (name, step, loss, lref, worst))
    if drops:
        assert m.dropout_state()['counter'] == 12


# ---- 3. routes -------------------------------------------------------------------------------------
def test_new_activation_nodes_give_up_the_fused_routes_and_nobody_else_does():
    """net (i): with the default activations the fused first layer, the tail and the head fire as
    before; with tanh / elu / selu the first layer takes the generic conv path, there is no tail,
    no gradient or pre-activation arrives as slabs, and the 'lin' head is still fused.  Net (iv):
    the fused epilogue is on for the relu layer and off for the elu layer."""
    for new in (False, True):
        m = net_convs() if new else net_convs_relu()
        x, t = batch_for(m, 31)
        m.gradients(x, t)
        plan = m._grad_func.func
        convs = [n for n in plan.nodes if type(n).__name__ == 'Conv']
        assert convs[0]._fused_first(plan) == (not new)
        assert convs[3]._fused_head(plan) is not None
        assert (convs[2]._tail(plan) is None) == (new or not plan.opt['fuse_tail'])
        for n in convs[:3]:
            assert n._plain_act() == (not new)
            if new:
                assert not n._parts_ok(plan) and not n._fused_act(plan)
                assert (n, 'grad_parts') not in plan.scratch
                assert plan.scratch[n, 'y_parts'].shape[0] == 1
                assert not n._actbwd_into_parent(plan)
    for second in ('relu', 'elu'):
        m = net_fused_epilogue(second)
        x, t = batch_for(m, 31)
        m.gradients(x, t)
        plan = m._grad_func.func
        convs = [n for n in plan.nodes if type(n).__name__ == 'Conv']
        assert convs[0]._fused_first(plan)
        assert convs[1]._fused_act(plan) == (second == 'relu')
        assert ((convs[1], 'y') in plan.scratch) == (second == 'elu')


# ---- 4. protocol -----------------------------------------------------------------------------------
def test_several_steps_in_one_graph_equal_single_steps():
    """trainingsteps(4, ring) == four trainingstep calls (losses 1e-5, parameters 1e-4)"""
    m0 = net_convs()
    x, t = batch_for(m0, 31)

    def fresh():
        mm = net_convs()
        for _ in range(2):                                   # eager + capture (builds the plan)
            mm.trainingstep(x, t, optimiser='Adam')
        return mm
    a = fresh()
    single = [float(a.trainingstep(x, t, optimiser='Adam')[0]) for _ in range(4)]
    b = fresh()
    pl = b.optimisers['Adam'].step.func
    ring = torch.empty((3, pl.input_arena.numel()), device='cuda')
    ring[:] = pl.input_arena
    losses, tsec = b.trainingsteps(4, optimiser='Adam', ring=ring)
    assert len(losses) == 4 and len(set(float(v) for v in losses)) == 4
    for u, v in zip(single, losses):
        assert abs(u - float(v)) / abs(u) < 1e-5, (single, list(losses))
    for (ka, pa), (kb, pb) in zip(a.loss_node.all_trainable_params.items(),
                                  b.loss_node.all_trainable_params.items()):
        assert rel(pb.get_value(), pa.get_value()) < 1e-4, ka


def test_checkpoint_after_two_steps_resumes_to_the_same_third_step(tmp_path):
    """bounds of tests/test_checkpoint.py's resume test: losses 2e-6, parameters 1e-5 relative"""
    from elektronn2_amd.neuromancer.model import modelload
    a = net_convs()
    x, t = batch_for(a, 31)
    for _ in range(2):
        a.trainingstep(x, t, optimiser='Adam')
    f = str(tmp_path / "act.mdl")
    a.save(f)
    third = float(a.trainingstep(x, t, optimiser='Adam')[0])
    end_p = [p.get_value() for p in a.loss_node.all_trainable_params.values()]
    b = net_convs(seed=99)                                   # other weights, nothing on the device
    modelload(f, b)
    assert [n.activation_func for n in b.nodes.values() if type(n).__name__ == 'Conv'] == \
        ['tanh', 'elu', 'selu', 'lin']
    got = float(b.trainingstep(x, t, optimiser='Adam')[0])
    assert abs(third - got) <= 2e-6 * abs(third), (third, got)
    for v, p in zip(end_p, b.loss_node.all_trainable_params.values()):
        assert np.abs(v - p.get_value()).max() <= 1e-5 * np.abs(v).max()


def _lite_act(in_sh, params, mfp=False):
    """neuro3d_lite's first layers with tanh / elu / selu (prediction only)"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    P = lambda i: dict(w=params[i][0], b=params[i][1])
    inp = nm.Input(in_sh, 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 8, (1, 4, 4), (1, 2, 2), activation_func='tanh', mfp=mfp, **P(0))
    out = nm.Conv(out, 12, (3, 3, 3), (1, 2, 2), activation_func='elu', mfp=mfp, **P(1))
    out = nm.Conv(out, 12, (2, 4, 4), (2, 1, 1), activation_func='selu', mfp=mfp, **P(2))
    out = nm.Conv(out, 16, (1, 3, 3), activation_func='soft+', mfp=mfp, **P(3))
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin', mfp=mfp, **P(4))
    probs = nm.Softmax(out)
    model = nm.model_manager.getmodel()
    if mfp:
        model.designate_nodes(input_node=inp, prediction_node=nm.FragmentsToDense(probs))
    else:
        model.designate_nodes(input_node=inp, prediction_node=probs)
    return model


def test_mfp_prediction_equals_the_offset_interleave():
    """tests/test_mfp_gpu.py's comparison on a tanh / elu / selu / soft+ net, at its bound (max
    abs 1e-5): the MFP fragments take the 'lin' pooling launches + e2_act_fwd in place"""
    rng = np.random.RandomState(6)
    shapes = [(8, 1, 1, 4, 4), (12, 8, 3, 3, 3), (12, 12, 2, 4, 4), (16, 12, 1, 3, 3), (2, 16, 1, 1, 1)]
    params = [((rng.randn(*s) / np.sqrt(np.prod(s[1:]))).astype(np.float32),
               (rng.randn(s[0]) * 0.1).astype(np.float32)) for s in shapes]
    raw = rng.rand(1, 10, 62, 58).astype(np.float32)
    plain = _lite_act((None, 1, 7, 47, 47), params)
    want = plain.predict_dense(raw)                  # one shifted pass per offset
    mfp = _lite_act((1, 1, 8, 54, 54), params, mfp=True)
    x = raw[None, :, :8, :54, :54]
    dense = mfp.predict(x)
    assert dense.shape[:2] == (1, 2)
    d = dense.shape[2:]
    assert np.abs(dense[0] - want[:, :d[0], :d[1], :d[2]]).max() < 1e-5
    got = mfp.predict_dense(raw)
    assert got.shape == want.shape
    assert np.abs(got - want).max() < 1e-5
    # ... and the plain prediction itself against float64 at a few positions' own fields of view
    P = [(torch.tensor(w.astype(np.float64)), torch.tensor(b.astype(np.float64))) for w, b in params]
    acts, pools = ['tanh', 'elu', 'selu', 'soft+', 'lin'], [(1, 2, 2), (1, 2, 2), (2, 1, 1), None, None]
    h = torch.tensor(raw[None, :, :7, :47, :47].astype(np.float64))
    for (w, b), a, p in zip(P, acts, pools):
        h = F.conv3d(h, w.flip(2, 3, 4))
        if p is not None:
            h = F.max_pool3d(h, p)
        h = act_torch(a, h + b.view(1, -1, 1, 1, 1))
    ref = torch.softmax(h, dim=1).numpy()
    one = plain.predict(raw[None, :, :7, :47, :47])
    assert rel(one, ref) < TOL_STEP


# ---- 5. bf16 mode ----------------------------------------------------------------------------------
@pytest.fixture()
def process_bf16():
    import elektronn2_amd
    elektronn2_amd.set_mfma_dtype('bf16')
    yield
    elektronn2_amd.set_mfma_dtype('f32')


def bf16_round(a):
    t = torch.tensor(np.asarray(a, np.float32))
    return t.to(torch.bfloat16).to(torch.float32).numpy().astype(np.float64)


def test_bf16_step_keeps_the_act_pair_in_f32_and_reads_no_stale_image(process_bf16):
    """one gradient evaluation (third call: replayed graph) of a conv stack with an elu and a tanh
    layer between relu layers, every conv launch pinned to the kernels with bf16 operands in
    memory and the operands made ahead (bf16_ahead.py).  Layer by layer on the tensors the pass
    produced, at tests/test_bf16_gpu.py's 2e-5: a node's output is f(pool(conv(bf16(x_hip),
    bf16(w))) + b) with x_hip the parent's ACTIVATED output -- a consumer that read an image made
    from anything else would miss; no new-activation node produces a 'next' image."""
    from elektronn2_amd import autotune, neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(26)
    sp = (9, 71, 71)
    spec = [(20, (1, 4, 4), (1, 2, 2), 'relu'), (24, (3, 3, 3), (1, 2, 2), 'elu'),
            (32, (1, 3, 3), (1, 1, 1), 'relu'), (32, (1, 3, 3), (1, 1, 1), 'relu'),
            (32, (1, 3, 3), (1, 1, 1), 'tanh'), (32, (1, 3, 3), (1, 1, 1), 'relu'),
            (2, (1, 1, 1), (1, 1, 1), 'lin')]
    with nm.plan_options(bf16_ahead=True, bf16_ahead_min=0.0):
        inp = nm.Input((1, 1) + sp, 'b,f,z,x,y', name='raw')
        out = inp
        for n_f, k, p, act in spec:
            out = nm.Conv(out, n_f, k, p, activation_func=act)
        m = _finish(nm, inp, out)
        m._grad_func.compile()
    x, t = batch_for(m, 32)
    autotune.force('igemm', "32,1,2")
    autotune.force('wgrad', "32,1,2,0,1")
    try:
        for _ in range(3):
            g = m.gradients(x, t)
    finally:
        autotune.force('igemm', None)
        autotune.force('wgrad', None)
    plan = m._grad_func.func
    torch.cuda.synchronize()
    assert {'fwd', 'dgrad'} <= set(k for (_, k) in plan.bf16a), sorted(set(k for (_, k) in plan.bf16a))
    convs = [n for n in plan.nodes if type(n).__name__ == 'Conv']
    new = [n for n in convs if not n._plain_act()]
    assert [n.activation_func for n in new] == ['elu', 'tanh']
    nexts = [n.name for (n, k) in plan.bf16a if k == 'next']
    print("producers of a 'next' image:", nexts)
    assert not set(nexts) & set(n.name for n in new), nexts
    assert convs[2].name in nexts, nexts                 # (relu -> relu: the mechanism is on)
    for n in new:                                        # ... and none is planned as bf16-only
        assert not any(node is n for (node, k) in plan.bf16a), n.name
    names = list(m.loss_node.all_trainable_params.keys())
    ys = dict((n, plan.scratch[n, 'y'].detach().cpu().numpy().astype(np.float64)) for n in convs[1:-1])
    outs = dict((n, plan.out[n].detach().cpu().numpy().astype(np.float64)) for n in [inp] + convs[:-1])
    douts = dict((n, plan.grad[n].detach().cpu().numpy().astype(np.float64)) for n in convs[:-1])
    worst = {}
    for i, node in enumerate(convs[:-1]):
        n_f, k, p, act = spec[i]
        rnd = (lambda a: a) if i == 0 else bf16_round        # (the fused first layer computes in f32)
        x_hip = outs[node.parent]
        w, b = node.w.get_value().astype(np.float64), node.b.get_value().astype(np.float64)
        bb = b.reshape(1, -1, 1, 1, 1)
        cv_ref = O.conv3d_fwd(rnd(x_hip), rnd(w))
        worst['fwd ' + node.name] = rel(outs[node], act_f(act, O.maxpool3d_fwd(cv_ref, p) + bb))
        if i == 0:
            continue
        # backward with the decisions of the HIP pass (its own conv output: which unit is active,
        # which element of a window is the largest -- tests/test_bf16_gpu.py)
        cv = ys[node]
        dp = douts[node] * act_df(act, O.maxpool3d_fwd(cv, p) + bb)
        dc = O.maxpool3d_bwd(dp, cv, p)
        worst['dW ' + node.name] = rel(g[names.index(node.name + '_w')],
                                       O.conv3d_wgrad(rnd(dc), rnd(x_hip), w.shape))
        worst['dx ' + node.name] = rel(douts[node.parent], O.conv3d_dgrad(rnd(dc), rnd(w), x_hip.shape))
    print(worst)
    bad = dict((k, v) for k, v in worst.items() if not v < TOL)
    assert not bad, bad
