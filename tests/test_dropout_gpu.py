"""Dropout on the GPU (csrc/dropout.hip, neural.py:391-397,714-720,1064-1070).

The reference of every comparison is the NumPy restatement of the gate contract of
include/e2hip.h (tests/test_dropout_host.py: Philox4x32-10, checked there against the Random123
known answers) plus float64 torch-CPU autograd of the nets -- never the kernels.  Bounds: ops at
the project's op bound 2e-5 (tests/test_ops_gpu.py:16); losses, gradients and the parameters
after one Adam step at the whole-step bound 1e-4 (tests/test_model_gpu.py:17); several steps in
one graph against single steps at 1e-5 (losses) / 1e-4 (parameters); the bf16 step at
tests/test_bf16_gpu.py's own 2e-5."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import e2_oracle as O
from test_dropout_host import restated_gate, threshold_fraction

pytestmark = pytest.mark.gpu
TOL = 2e-5          # ops
TOL_STEP = 1e-4     # loss, gradients, parameters after an Adam step
ADAM = dict(lr=5e-4, mom=0.9, beta2=0.999, wd=0.5e-4)


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device='cuda')


def state_tensor(seed, counter):
    """the device-side generator state of the C ABI: seed lo, seed hi, counter, -"""
    w = np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff, counter & 0xffffffff, 0], np.uint32)
    return torch.from_numpy(w.view(np.int32).copy()).cuda()


def expect(x, rate, seed, counter, stream, feature=False):
    """out = keep ? x * scale : 0 with the restated gate; x: numpy (n, c, d, h, w)"""
    if feature:
        keep, scale = restated_gate(x.shape[1], rate, seed, counter, stream)
        keep = np.broadcast_to(keep.reshape(1, -1, 1, 1, 1), x.shape)
    else:
        keep, scale = restated_gate(x.size, rate, seed, counter, stream)
        keep = keep.reshape(x.shape)
    return keep, np.where(keep, x.astype(np.float64) * np.float64(scale), 0.0)


# ---- views: name -> (logical shape, function making (storage, view)) ---------------------------
def _dense(shape):
    t = torch.empty(shape, device='cuda')
    return t, t


def _concat_slice(shape):
    n, c, d, h, w = shape
    t = torch.empty((n, c + 5, d, h, w), device='cuda')
    return t, t[:, 3:3 + c]


def _padded_rows(shape):
    """the interior of a zero-padded gradient buffer whose row pitch is odd (neural.py: dy_pad)"""
    n, c, d, h, w = shape
    t = torch.empty((n, c, d + 2, h + 4, w + 3), device='cuda')
    return t, t[:, :, 1:1 + d, 2:2 + h, 1:1 + w]


def _crop(shape):
    n, c, d, h, w = shape
    t = torch.empty((n, c, d, h + 2, w + 8), device='cuda')
    return t, t[:, :, :, 1:1 + h, 4:4 + w]          # (16-byte aligned row starts, rows of their own)


VIEWS = [("dense", _dense), ("concat_slice", _concat_slice), ("padded_rows", _padded_rows),
         ("crop", _crop)]
SHAPES = [(2, 3, 4, 5, 8), (1, 2, 3, 5, 7), (2, 5, 1, 3, 13), (1, 1, 1, 1, 3), (3, 7, 1, 1, 1),
          (1, 3, 2, 9, 16), (1, 1, 5, 33, 34)]


@pytest.mark.parametrize("feature", [False, True], ids=["element", "feature"])
@pytest.mark.parametrize("view", VIEWS, ids=[v[0] for v in VIEWS])
def test_fwd_and_bwd_through_the_c_abi(ctx, view, feature):
    """zero pattern == the restated gate EXACTLY; kept values at the op bound; bwd draws the gate
    of fwd; src -> dst and in place agree; what lies around the view is untouched"""
    rng = np.random.RandomState(11)
    seed, counter, stream, rate = (7 << 32) + 1234, 5, 3, 0.3
    st = state_tensor(seed, counter)
    r = dev([rate])
    for shape in SHAPES:
        x = rng.randn(*shape).astype(np.float32)
        x[np.abs(x) < 1e-3] = 1.0                        # (a zero in the output is a dropped element)
        keep, ref = expect(x, np.float32(rate), seed, counter, stream, feature)
        store, v = view[1](shape)
        store.fill_(-77.0)
        v.copy_(dev(x))
        before = store.clone()
        out = torch.full(shape, 5.0, device='cuda')
        ctx.dropout_fwd(v, out, r, st, stream, feature_mode=feature)
        got = out.cpu().numpy()
        assert np.array_equal(got != 0, keep), shape
        assert rel(got, ref) < TOL, shape
        assert torch.equal(store, before)                # (the source view is only read)
        ctx.dropout_fwd(v, v, r, st, stream, feature_mode=feature)          # in place, strided
        assert np.array_equal(v.cpu().numpy(), got), shape
        mstore, mview = view[1](shape)                   # same geometry: where the view lies
        mstore.fill_(0); mview.fill_(1)
        outside = mstore == 0
        assert torch.equal(store[outside], before[outside]), shape          # nothing around it written
        # backward: the same gate on another tensor, through another view
        dy = rng.randn(*shape).astype(np.float32)
        dy[np.abs(dy) < 1e-3] = 1.0
        gstore, gv = view[1](shape)
        gv.copy_(dev(dy))
        ctx.dropout_bwd(gv, gv, r, st, stream, feature_mode=feature)
        dgot = gv.cpu().numpy()
        assert np.array_equal(dgot != 0, keep), shape
        assert rel(dgot, expect(dy, np.float32(rate), seed, counter, stream, feature)[1]) < TOL, shape


def test_rate_zero_is_bit_identical_and_the_gate_follows_counter_stream_seed(ctx):
    rng = np.random.RandomState(12)
    shape = (2, 3, 4, 6, 10)
    x = rng.randn(*shape).astype(np.float32)
    x.flat[::7] = -0.0
    x.flat[3] = np.float32(1e-42)                        # a denormal survives too
    xd = dev(x)
    out = torch.empty_like(xd)
    ctx.dropout_fwd(xd, out, dev([0.0]), state_tensor(99, 1), 0)
    assert np.array_equal(out.cpu().numpy().view(np.int32), x.view(np.int32))
    x[x == 0] = 1.0
    xd = dev(x)
    r = dev([0.5])

    def gate(seed, counter, stream):
        o = torch.empty_like(xd)
        ctx.dropout_fwd(xd, o, r, state_tensor(seed, counter), stream)
        k = o.cpu().numpy() != 0
        assert np.array_equal(k, expect(x, np.float32(0.5), seed, counter, stream)[0])
        return k
    base = gate(1234, 7, 3)
    assert np.array_equal(base, gate(1234, 7, 3))
    for other in ((1234, 8, 3), (1234, 7, 4), (1235, 7, 3), (1234 + (1 << 32), 7, 3), (1234, 7, 3 + (1 << 16))):
        assert 0.3 < (gate(*other) != base).mean() < 0.7, other
    # the rate is read from device memory when the kernel runs
    o = torch.empty_like(xd)
    r.fill_(0.9)
    ctx.dropout_fwd(xd, o, r, state_tensor(1234, 7), 3)
    assert np.array_equal(o.cpu().numpy() != 0, expect(x, np.float32(0.9), 1234, 7, 3)[0])


def test_tick_advances_the_counter_the_gates_read(ctx):
    st = state_tensor(42, 0xffffffff)                    # (wraps to 0)
    x = np.ones((1, 2, 3, 4, 8), np.float32)
    xd, r = dev(x), dev([0.5])
    for expect_counter in (0, 1, 2):
        ctx.dropout_tick(st)
        o = torch.empty_like(xd)
        ctx.dropout_fwd(xd, o, r, st, 1)
        assert np.array_equal(o.cpu().numpy() != 0, expect(x, np.float32(0.5), 42, expect_counter, 1)[0])
    w = st.cpu().numpy().view(np.uint32)
    assert list(w) == [42, 0, 2, 0]


@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_kept_fraction(ctx, rate):
    """n = 2^22, seed 1234, stream 3, counter 7: the kept fraction is within 5 sqrt(r (1 - r) / n)
    of 1 - T / 2^32 (derived bound; deterministic for a fixed seed)"""
    n = 1 << 22
    xd = torch.ones((1, 4, 16, 256, 256), device='cuda')
    o = torch.empty_like(xd)
    ctx.dropout_fwd(xd, o, dev([rate]), state_tensor(1234, 7), 3)
    frac = float((o != 0).double().mean().item())
    print("rate %.1f: kept %.6f, contract %.6f, bound %.6f" % (
        rate, frac, threshold_fraction(rate), 5 * np.sqrt(rate * (1 - rate) / n)))
    assert abs(frac - threshold_fraction(rate)) < 5 * np.sqrt(rate * (1 - rate) / n)
    assert np.array_equal((o != 0).cpu().numpy().ravel(), restated_gate(n, np.float32(rate), 1234, 7, 3)[0])


# ---- model level: float64 autograd of the graph with restated gates ----------------------------
def _relu(x):
    return 0.5 * (x + x.abs())           # relu'(0) = 0.5, as the kernels


# A relu unit whose float64 pre-activation lies within float32 rounding of zero makes the
# comparison ill-posed: the f32 pass may take the other slope, depending on the order of its sums
# (tiling, atomics), and ONE such unit moves a small net's gradients by 1e-4 of their largest
# element (seen here: |pre| = 3.8e-8 in one unit, conv gradients off by 1.2e-4 and 2.1e-4 in some
# runs and by 2e-7 in others; tests/test_bf16_gpu.py meets the same and exempts the elements).  An
# f32 sum of K <= 432 products of magnitude <= 0.3 carries an error of about sqrt(K) 2^-24 0.3 =
# 4e-7, so every evaluation below first checks on the REFERENCE that no unit is closer to zero
# than 1e-6; the data seeds were chosen (with the reference alone, on the CPU) so that this holds.
MIN_PRE = 1e-6


class Ref(object):
    """float64 torch-CPU restatement of a model's graph (conv -> pool -> (BN) + bias -> act ->
    dropout per node) with the gates of include/e2hip.h"""

    def __init__(self, model):
        self.model = model
        self.t = 0
        self.min_pre = np.inf          # smallest |pre-activation| of a relu unit in the last forward
        self.P, self.m, self.s = {}, {}, {}
        for node in model.nodes.values():
            for p in node.params.values():
                if id(p) not in self.P:
                    self.P[id(p)] = torch.tensor(p.get_value().astype(np.float64),
                                                 requires_grad=bool(p.apply_train))
        self.streams = dict((id(n), i) for i, n in enumerate(model.dropout_nodes()))

    def p(self, param):
        return self.P[id(param)]

    def drop(self, node, h, seed, counter, rates):
        if node.params.get('dropout_rate') is None:
            return h
        rate = np.float32(rates[self.streams[id(node)]])
        if node._drop_per_feature:
            keep, scale = restated_gate(h.shape[1], rate, seed, counter, self.streams[id(node)])
            keep = keep.reshape((1, -1) + (1,) * (h.dim() - 2))
        else:
            keep, scale = restated_gate(h.numel(), rate, seed, counter, self.streams[id(node)])
            keep = keep.reshape(tuple(h.shape))
        return h * torch.tensor(keep.astype(np.float64) * np.float64(scale))

    def relu(self, y):
        self.min_pre = min(self.min_pre, float(y.detach().abs().min()))
        return _relu(y)

    def forward(self, x, t, seed, counter, rates=None):
        m = self.model
        self.min_pre = np.inf
        if rates is None:
            rates = [float(v) for v in m.dropout_rates.ravel()]
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
                    red = [i for i in range(y.dim()) if i != 1]
                    mean = y.mean(dim=red)
                    std = torch.sqrt(((y - mean.view(bsh)) ** 2).mean(dim=red)) + 1e-6
                    g = self.p(node.gamma)
                    y = (g / std).view(bsh) * y + (b - g * mean / std).view(bsh)
                else:
                    assert not node.batch_normalisation
                    y = y + b.view(bsh)
                y = self.relu(y) if node.activation_func == 'relu' else y
                val[node] = self.drop(node, y, seed, counter, rates)
            elif kind == 'Perceptron':
                assert not node.batch_normalisation
                h = val[par].flatten(1) if node.flatten else val[par]
                y = h @ self.p(node.w) + self.p(node.b)
                y = self.relu(y) if node.activation_func == 'relu' else y
                val[node] = self.drop(node, y, seed, counter, rates)
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

    def loss_and_grads(self, x, t, seed, counter, rates=None):
        for v in self.P.values():
            v.grad = None
        loss, probs = self.forward(x, t, seed, counter, rates)
        assert self.min_pre >= MIN_PRE, "ill-posed case: a relu unit at %.1e (counter %d)" % (self.min_pre, counter)
        loss.backward()
        return float(loss.detach()), probs.detach().numpy()

    def grads(self):
        """in the order of Model.gradients"""
        return [self.p(p).grad.numpy() for p in self.model.trainable_params]

    @torch.no_grad()
    def adam(self, lr, mom, beta2, wd):
        """optimiser.py:273-334 (oracle/torch_step.py TorchNet.adam), weight decay times the
        parameter's apply_reg multiplier"""
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


def net_convs(drop=True, batch=1, sp=(7, 47, 47), seed=21):
    """(i): fused first layer, pooling, a (1,1,1) relu conv + a (1,1,1) 'lin' head -- the net whose
    first-layer / tail / head fusions fire when no node has dropout"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    r = (lambda v: v) if drop else (lambda v: 0)
    inp = nm.Input((batch, 1) + tuple(sp), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 8, (1, 4, 4), (1, 2, 2), dropout_rate=r(0.2))
    out = nm.Conv(out, 12, (3, 3, 3), (1, 2, 2), dropout_rate=r(0.3))
    out = nm.Conv(out, 16, (1, 1, 1), dropout_rate=r(0.4))
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin', dropout_rate=r(0.1))
    return _finish(nm, inp, out)


def net_unet(batch=1, seed=22):
    """(ii): Conv / Pool / UpConvMerge (UpConv + Crop + Concat): dropout on the UpConv (its output
    and gradient are channel slices of the Concat's buffers) and on the skip branch the Crop reads.
    (The conv that FEEDS the UpConv carries none: a freshly built UpConv has a zero bias
    (identity_init), so positions whose input channels are all dropped have a pre-activation of
    exactly 0, where the UpConv backward takes slope 0 and the reference's relu 0.5 -- a property
    of that kernel at exact zeros, DESIGN "Dropout", not of the gates.)"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 1, 6, 20, 20), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 8, (1, 3, 3))
    c1 = nm.Conv(c0, 8, (1, 3, 3), dropout_rate=0.25)
    p1 = nm.Pool(c1, (1, 2, 2))
    c2 = nm.Conv(p1, 16, (3, 3, 3))
    c3 = nm.Conv(c2, 16, (3, 3, 3))
    mrg = nm.UpConvMerge(c1, c3, 24, upconv_kwargs=dict(dropout_rate=0.3))
    c4 = nm.Conv(mrg, 8, (1, 3, 3))
    out = nm.Conv(c4, 2, (1, 1, 1), activation_func='lin')
    return _finish(nm, inp, out)


def net_mnist(batch=8, seed=23):
    """(iii): elektronn2_amd.nets.mnist (2-D convs with train-mode batch norm, two Perceptrons)
    with dropout on the first Perceptron: one gate per feature, the same for every example"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 1, 26, 26), 'b,f,y,x', name='raw')
    out = nm.Conv(inp, 12, (3, 3), (2, 2), batch_normalisation='train')
    out = nm.Conv(out, 36, (3, 3), (2, 2), batch_normalisation='train', dropout_rate=0.2)
    out = nm.Conv(out, 64, (3, 3), (1, 1), batch_normalisation='train')
    out = nm.Perceptron(out, 200, flatten=True, dropout_rate=0.5)
    out = nm.Perceptron(out, 10, activation_func='lin')
    return _finish(nm, inp, out)


def net_fused_epilogue(seed=24):
    """(iv): un-pooled convs with enough output tiles (160 planes) for the fused kernels: the first runs the fused first-layer
    pair (also without pooling), the second the conv with the bias + activation epilogue, whose
    backward reads the ACTIVATED output (signed zeros) that dropout has gated in place"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((1, 1, 160, 8, 8), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 4, (1, 3, 3), dropout_rate=0.3)
    out = nm.Conv(out, 6, (1, 3, 3), dropout_rate=0.5)
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin')
    return _finish(nm, inp, out)


def batch_for(model, seed, n_class=2):
    rng = np.random.RandomState(seed)
    x = rng.rand(*model.input_node.shape.shape).astype(np.float32)
    t = rng.randint(0, n_class, model.target_node.shape.shape).astype(np.float32)
    if t.ndim == 5:
        t.flat[::17] = -1                      # unlabelled voxels
    return x, t


# name, constructor, classes, seed of the batch (chosen on the reference alone: see MIN_PRE)
NETS = [("convs", net_convs, 2, 31), ("unet", net_unet, 2, 45), ("mnist", net_mnist, 10, 31),
        ("fused_epilogue", net_fused_epilogue, 2, 31)]


@pytest.mark.parametrize("name,make,ncls,data_seed", NETS, ids=[n[0] for n in NETS])
def test_loss_gradients_and_adam_step_against_float64(name, make, ncls, data_seed):
    """fixed seed, gates restated from dropout_state(): loss, prediction, EVERY parameter gradient
    and one Adam step -- eager, captured and replayed calls, each with the counter it used"""
    m = make()
    x, t = batch_for(m, data_seed, ncls)
    ref = Ref(m)
    seed = 20240 + len(name)
    m.set_dropout_seed(seed)
    assert len(m.dropout_nodes()) >= 2
    losses = []
    for call in range(3):                                   # eager, capture, replay
        st = m.dropout_state()
        assert st == dict(seed=seed, counter=3 * call)
        lref, pref = ref.loss_and_grads(x, t, seed, st['counter'])
        loss = float(m.loss(x, t))
        print("%s call %d: loss %.7f ref %.7f" % (name, call, loss, lref))
        assert abs(loss - lref) / abs(lref) < TOL_STEP, (call, loss, lref)
        losses.append(loss)
        st = m.dropout_state()
        assert st['counter'] == 3 * call + 1                 # every plan run of the model ticks once
        lref, pref = ref.loss_and_grads(x, t, seed, st['counter'])
        assert rel(m.predict(x), pref) < TOL_STEP
        st = m.dropout_state()
        ref.loss_and_grads(x, t, seed, st['counter'])
        got = m.gradients(x, t)
        names = list(m.loss_node.all_trainable_params.keys())
        want = ref.grads()
        assert len(got) == len(want) == len(names)
        errs = dict((nme, rel(g, w)) for nme, g, w in zip(names, got, want))
        print("%s call %d: gradients, worst %s" % (name, call, sorted(errs.items(), key=lambda kv: -kv[1])[:3]))
        for nme, g, w in zip(names, got, want):
            assert np.abs(w).max() > 0, nme
            assert errs[nme] < TOL_STEP, (call, nme, errs[nme])
    assert len(set(losses)) == 3                            # three counters, three gates
    if name == "fused_epilogue":
        plan = m._grad_func.func
        first, second = m.dropout_nodes()
        assert first._fused_first(plan) and second._fused_act(plan)
    # Adam steps: eager, captured, replayed
    for step in range(3):
        st = m.dropout_state()
        lref, _ = ref.loss_and_grads(x, t, seed, st['counter'])
        ref.adam(**ADAM)
        loss = float(m.trainingstep(x, t, optimiser='Adam')[0])
        assert abs(loss - lref) / abs(lref) < TOL_STEP, (step, loss, lref)
        for nme, p in m.loss_node.all_trainable_params.items():
            e = rel(p.get_value(), ref.p(p).detach().numpy())
            assert e < TOL_STEP, (step, nme, e)
    assert m.dropout_state()['counter'] == 12


def test_dropout_nodes_give_up_exactly_the_routes_without_their_tensors():
    """net (i): without dropout the tail / head fusions fire; with dropout on every Conv neither
    does, the first layer stays fused (it materialises output and output gradient), and no
    dropout node's gradient arrives as slabs"""
    x = None
    for drop in (False, True):
        m = net_convs(drop=drop)
        x, t = batch_for(m, 31)
        m.gradients(x, t)
        plan = m._grad_func.func
        convs = [n for n in plan.nodes if type(n).__name__ == 'Conv']
        assert convs[0]._fused_first(plan)
        assert (convs[3]._fused_head(plan) is None) == drop
        assert (convs[2]._tail(plan) is None) == (drop or not plan.opt['fuse_tail'])
        assert bool(plan._drop_nodes) == drop
        for n in convs:
            assert not (drop and (n, 'grad_parts') in plan.scratch)


def test_replays_draw_new_gates_and_several_steps_in_one_graph_equal_single_steps():
    """three replays of one captured step: three losses, each the restated-gate reference's;
    trainingsteps(4, ring) == four trainingstep calls from the same seed (losses 1e-5,
    parameters 1e-4)"""
    m = net_convs()
    x, t = batch_for(m, 31)
    ref = Ref(m)
    m.set_dropout_seed(555)
    m.trainingstep(x, t, optimiser='Adam')                  # eager
    m.trainingstep(x, t, optimiser='Adam')                  # capture
    plan = m.optimisers['Adam'].step.func
    graphs = list(plan._graphs)
    assert graphs
    for c in range(2):
        ref.loss_and_grads(x, t, 555, c); ref.adam(**ADAM)
    seen = []
    for c in range(2, 5):                                   # replays
        assert m.dropout_state()['counter'] == c
        lref, _ = ref.loss_and_grads(x, t, 555, c); ref.adam(**ADAM)
        loss = float(m.trainingstep(x, t, optimiser='Adam')[0])
        assert abs(loss - lref) / abs(lref) < TOL_STEP, (c, loss, lref)
        seen.append(loss)
    assert len(set(seen)) == 3
    assert plan._graphs == graphs                            # the same captured graphs throughout

    def fresh():
        mm = net_convs()
        mm.set_dropout_seed(777)
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
    assert a.dropout_state() == b.dropout_state() == dict(seed=777, counter=6)
    for (ka, pa), (kb, pb) in zip(a.loss_node.all_trainable_params.items(),
                                  b.loss_node.all_trainable_params.items()):
        assert rel(pb.get_value(), pa.get_value()) < 1e-4, ka


def test_rates_to_zero_on_a_captured_plan_and_back():
    """the trainer's validation pass (training/trainer.py:378-403): rates to 0 -> predict / loss
    equal the twin net built without dropout, with the SAME captured graphs; restored rates bring
    dropout back"""
    m = net_convs()
    x, t = batch_for(m, 31)
    params = m.get_param_values()
    m.set_dropout_seed(99)
    for _ in range(2):
        l_drop = float(m.loss(x, t)); p_drop = m.predict(x)
    plans = [m.loss_node._output_func.func, m.prediction_node._output_func.func]
    graphs = [list(p._graphs) for p in plans]
    assert all(graphs)
    rates = m.dropout_rates
    m.dropout_rates = 0
    l0, p0 = float(m.loss(x, t)), m.predict(x)
    assert [list(p._graphs) for p in plans] == graphs          # no re-capture
    m.dropout_rates = rates
    c = m.dropout_state()['counter']
    l1 = float(m.loss(x, t))
    ref = Ref(m)
    lref, _ = ref.loss_and_grads(x, t, 99, c)
    assert abs(l1 - lref) / abs(lref) < TOL_STEP and abs(l1 - l0) / abs(l0) > 1e-3
    twin = net_convs(drop=False)
    assert twin.dropout_rates.size == 0
    twin.set_param_values(params_without_rates(params))
    lt, pt = float(twin.loss(x, t)), twin.predict(x)
    assert abs(l0 - lt) / abs(lt) < TOL_STEP, (l0, lt)
    assert rel(p0, pt) < TOL_STEP
    assert abs(l_drop - lt) / abs(lt) > 1e-3


def params_without_rates(params):
    return dict((k, dict((pk, pv) for pk, pv in v.items() if pk != 'dropout_rate'))
                for k, v in params.items())


# ---- bf16 mode ------------------------------------------------------------------------------
@pytest.fixture()
def process_bf16():
    import elektronn2_amd
    elektronn2_amd.set_mfma_dtype('bf16')
    yield
    elektronn2_amd.set_mfma_dtype('f32')


def bf16_round(a):
    t = torch.tensor(np.asarray(a, np.float32))
    return t.to(torch.bfloat16).to(torch.float32).numpy().astype(np.float64)


def test_bf16_step_reads_no_stale_operand_image(process_bf16):
    """one gradient evaluation of a dropout net in bf16 mode with every conv launch pinned to the
    kernels with bf16 operands in memory and the operands made ahead by their producers
    (bf16_ahead.py), third call (replayed graph).  Layer by layer on the tensors the HIP pass
    produced, as tests/test_bf16_gpu.py does and at its bound 2e-5: the node's output is the GATED
    oracle conv(bf16(x_hip), bf16(w)) -> pool -> bias -> relu, where x_hip is the parent's gated
    output -- a consumer that read an image written before the gate would miss by the dropped
    elements; the parent's output gradient is the gated dgrad(bf16(dc), bf16(w))."""
    from elektronn2_amd import autotune, neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(25)
    sp = (9, 71, 71)
    spec = [(20, (1, 4, 4), (1, 2, 2), 'relu', 0.2), (24, (3, 3, 3), (1, 2, 2), 'relu', 0.3),
            (32, (1, 3, 3), (1, 1, 1), 'relu', 0.0), (32, (1, 3, 3), (1, 1, 1), 'relu', 0.5),
            (2, (1, 1, 1), (1, 1, 1), 'lin', 0.0)]
    with nm.plan_options(bf16_ahead=True, bf16_ahead_min=0.0):
        inp = nm.Input((1, 1) + sp, 'b,f,z,x,y', name='raw')
        out = inp
        for n_f, k, p, act, r in spec:
            out = nm.Conv(out, n_f, k, p, activation_func=act, dropout_rate=r)
        m = _finish(nm, inp, out)
        m._grad_func.compile()
    x, t = batch_for(m, 32)
    m.set_dropout_seed(4242)
    autotune.force('igemm', "32,1,2")
    autotune.force('wgrad', "32,1,2,0,1")
    try:
        for _ in range(3):
            c = m.dropout_state()['counter']
            g = m.gradients(x, t)
    finally:
        autotune.force('igemm', None)
        autotune.force('wgrad', None)
    plan = m._grad_func.func
    torch.cuda.synchronize()
    assert {'fwd', 'dgrad'} <= set(k for (_, k) in plan.bf16a), sorted(set(k for (_, k) in plan.bf16a))
    convs = [n for n in plan.nodes if type(n).__name__ == 'Conv']
    # producers without dropout still write their consumer's image; dropout nodes never do
    nexts = [n.name for (n, k) in plan.bf16a if k == 'next']
    assert nexts == [convs[2].name], nexts
    names = list(m.loss_node.all_trainable_params.keys())
    ys = dict((n, plan.scratch[n, 'y'].detach().cpu().numpy().astype(np.float64)) for n in convs[1:-1])
    outs = dict((n, plan.out[n].detach().cpu().numpy().astype(np.float64)) for n in [inp] + convs[:-1])
    douts = dict((n, plan.grad[n].detach().cpu().numpy().astype(np.float64)) for n in convs[:-1])
    order = dict((id(n), i) for i, n in enumerate(m.dropout_nodes()))
    worst = {}

    def gate(node, a):
        if node.dropout_rate is None:
            return a
        keep, scale = restated_gate(a.size, node.dropout_rate.get_value()[0], 4242, c, order[id(node)])
        return np.where(keep.reshape(a.shape), a * np.float64(scale), 0.0)
    for i, node in enumerate(convs[:-1]):
        n_f, k, p, act, r = spec[i]
        rnd = (lambda a: a) if i == 0 else bf16_round        # (the fused first layer computes in f32)
        x_hip = outs[node.parent]
        w, b = node.w.get_value().astype(np.float64), node.b.get_value().astype(np.float64)
        out_ref, (cv, pooled) = O.conv_node_fwd(rnd(x_hip), rnd(w), b, p, act)
        worst['fwd ' + node.name] = rel(outs[node], gate(node, out_ref))
        if i == 0:
            continue
        # backward with the decisions of the HIP pass (its own conv output: which unit is active,
        # which element of a window is the largest -- tests/test_bf16_gpu.py): the (gated) output
        # gradient through the oracle's activation / pooling backward, then the weight gradient and
        # the data gradient into the parent -- which the parent's own gate launch has gated since
        cv = ys[node]
        dp, _ = O.bias_act_bwd(douts[node], O.maxpool3d_fwd(cv, p), b, act)
        dc = O.maxpool3d_bwd(dp, cv, p)
        worst['dW ' + node.name] = rel(g[names.index(node.name + '_w')],
                                       O.conv3d_wgrad(rnd(dc), rnd(x_hip), w.shape))
        dx_ref = O.conv3d_dgrad(rnd(dc), rnd(w), x_hip.shape)
        worst['dx ' + node.name] = rel(douts[node.parent], gate(node.parent, dx_ref))
    print(worst)
    bad = dict((k, v) for k, v in worst.items() if not v < TOL)
    assert not bad, bad
