"""Nets in which two nodes share a parameter object (``w=<other>.w``, ``b=...``, ``gamma=...``) and
their float64 reference, shared by tests/test_shared_params_host.py and test_shared_params_gpu.py.

``SRef`` is ``Ref`` of tests/test_conv_modes_host.py (leaves keyed by id(param): a shared parameter
is ONE leaf, autograd sums the contributions, ``adam`` updates it once) with the node kinds these
nets add: Perceptron, SplitPart and an AggregateLoss of several sparse NLL terms.  ``untied=True``
gives every node that borrows a parameter a leaf of its own holding the same values: the same
numbers forward, and the two contributions to each shared gradient apart (``contributions``)."""
import numpy as np
import torch
import torch.nn.functional as F

from test_conv_modes_host import Ref, conv_ref

ADAM = dict(lr=5e-4, mom=0.9, beta2=0.999, wd=0.5e-4)       # tests/test_model_gpu.py
TOL = 1e-4                                                  # tests/test_model_gpu.py:17
# bf16 operands against the f32 net's reference: test_training_step_bf16_close_to_f32_oracle of
# tests/test_bf16_gpu.py (loss within 1e-2, every gradient within 1e-1 of its largest entry)
BF16_LOSS, BF16_GRAD = 1e-2, 1e-1
BF16_NETS = ('S1',)
KEYS = ('w', 'b', 'gamma')
N_STEPS = 4


def borrowed(model):
    """[(node, key, param)] of every parameter a node takes from another node"""
    out = []
    for node in model.nodes.values():
        for key in KEYS:
            p = getattr(node, key, None)
            if p is not None and hasattr(p, 'get_value') and hasattr(node, 'params') \
                    and node.params.get(key) is not p:
                out.append((node, key, p))
    return out


class SRef(Ref):
    def __init__(self, model, untied=False):
        Ref.__init__(self, model)
        self.twin = {}
        if untied:
            for node, key, p in borrowed(model):
                self.twin[id(node), key] = self.P[id(p)].detach().clone().requires_grad_(True)

    def leaf(self, node, key):
        t = self.twin.get((id(node), key))
        return self.P[id(getattr(node, key))] if t is None else t

    def forward(self, x, t=None, upto=None):
        m = self.model
        self.min_pre = np.inf
        val = {}
        for node in m.nodes.values():
            kind = type(node).__name__
            par = node.parent
            if node is m.input_node:
                val[node] = torch.tensor(np.asarray(x, np.float64))
            elif node is m.target_node:
                if t is not None:
                    val[node] = torch.tensor(np.asarray(t, np.float64))
            elif isinstance(par, (list, tuple)) and any(q not in val for q in par) or \
                    (not isinstance(par, (list, tuple)) and par not in val):
                continue                                     # (behind the target: no target given)
            elif kind in ('Conv', 'UpConv', 'Perceptron'):
                h, w, b = val[par], self.leaf(node, 'w'), self.leaf(node, 'b')
                if kind == 'Perceptron':
                    y = (h.flatten(1) if node.flatten else h) @ w
                elif kind == 'UpConv':
                    y = F.conv_transpose3d(h, w.permute(1, 0, 2, 3, 4), stride=tuple(node.pool_shape))
                else:
                    y = conv_ref(h, w, node.conv_mode)
                    if any(q != 1 for q in node.pool_shape):
                        y = (F.max_pool3d if h.dim() == 5 else F.max_pool2d)(y, tuple(node.pool_shape))
                if node.batch_normalisation == 'train':
                    y = self.bn(y, self.leaf(node, 'gamma'), b, [i for i in range(y.dim()) if i != 1])
                else:
                    assert not node.batch_normalisation
                    y = y + b.view((1, -1) + (1,) * (y.dim() - 2))
                val[node] = self.act(node, y)
            elif kind == 'SplitPart':
                val[node] = val[par][:, node.lo:node.hi]
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
                ps = list(par) if isinstance(par, (list, tuple)) else [par]
                if len(ps) == 1:
                    val[node] = val[ps[0]].mean()
                else:                      # weighted mean of the terms (loss.py, AggregateLoss)
                    w = node.mixing_weights.get_value().astype(np.float64)
                    val[node] = sum(float(w[k]) * val[q].mean() for k, q in enumerate(ps)) / len(ps)
            elif kind in ('Errors', '_Errors', 'Classification'):
                continue
            else:
                raise NotImplementedError(kind)
            if upto is not None and node is upto:
                return val[node]
        return (val.get(m.loss_node), val[m.prediction_node])

    def loss_and_grads(self, x, t):
        for v in self.twin.values():
            v.grad = None
        return Ref.loss_and_grads(self, x, t)

    def contributions(self):
        """{(owner param name, key): (gA, gB)} after loss_and_grads of an UNTIED reference: the
        gradient of the owner's leaf and the sum over the borrowing nodes' leaves"""
        out = {}
        for node, key, p in borrowed(self.model):
            k = id(p)
            ga, gb = out.get(k, (self.P[k].grad.numpy().copy(), 0.0))
            out[k] = (ga, gb + self.twin[id(node), key].grad.numpy())
        return out


# ---- the nets ----------------------------------------------------------------------------------------
def _finish(nm, inp, logits, name):
    probs = nm.Softmax(logits)
    target = nm.Input_like(probs, override_f=1, name='target')
    loss = nm.AggregateLoss(nm.MultinoulliNLL(probs, target, target_is_sparse=True), name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=probs)
    model.set_opt_meta_params('Adam', ADAM)
    model._classes = (logits.n_f,)
    return model


def _s1(nm, same_sig=False):
    inp = nm.Input((1, 1, 5, 22, 24), 'b,f,z,x,y', name='raw')
    if same_sig:
        # S2: two trunks, the sharing convs see tensors of one shape and pitch
        a = nm.Conv(nm.Conv(inp, 4, (1, 3, 3), name='stem_a'), 4, (1, 3, 3), name='a')
        b = nm.Conv(nm.Conv(inp, 4, (1, 3, 3), name='stem_b'), 4, (1, 3, 3), name='b', w=a.w, b=a.b)
        out = nm.Concat([a, b], name='cat')
    else:
        # S1: one pools, the other sees other extents
        c0 = nm.Conv(inp, 4, (1, 3, 3), name='stem')
        a = nm.Conv(c0, 4, (1, 3, 3), (1, 2, 2), name='a')
        out = nm.Conv(a, 4, (1, 3, 3), name='b', w=a.w, b=a.b)
    return _finish(nm, inp, nm.Conv(out, 2, (1, 1, 1), activation_func='lin', name='head'), 's1')


def _s3(nm):
    inp = nm.Input((1, 1, 5, 18, 20), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 4, (1, 3, 3), (1, 2, 2), name='stem')
    a = nm.UpConv(c0, 4, (1, 2, 2), name='a')
    c1 = nm.Conv(a, 4, (1, 3, 3), (1, 2, 2), name='mid')
    b = nm.UpConv(c1, 4, (1, 2, 2), name='b', identity_init=False, w=a.w, b=a.b)
    return _finish(nm, inp, nm.Conv(b, 2, (1, 1, 1), activation_func='lin', name='head'), 's3')


def _s4(nm):
    inp = nm.Input((1, 1, 5, 18, 20), 'b,f,z,x,y', name='raw')
    a = nm.Conv(inp, 4, (1, 3, 3), name='a')                      # fused first layer
    c1 = nm.Conv(a, 1, (1, 3, 3), name='mid')
    b = nm.Conv(c1, 4, (1, 3, 3), name='b', w=a.w, b=a.b)         # the same filters as a GEMM
    return _finish(nm, inp, nm.Conv(b, 2, (1, 1, 1), activation_func='lin', name='head'), 's4')


def _s5(nm):
    inp = nm.Input((1, 1, 5, 14, 16), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 4, (1, 3, 3), name='stem')
    a = nm.Conv(c0, 4, (1, 1, 1), name='a')
    b = nm.Conv(a, 4, (1, 1, 1), name='b', w=a.w, b=a.b)          # the tail's 1x1x1 relu conv
    return _finish(nm, inp, nm.Conv(b, 2, (1, 1, 1), activation_func='lin', name='head'), 's5')


def _s6(nm):
    inp = nm.Input((1, 1, 5, 14, 16), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 4, (1, 3, 3), (1, 2, 2), name='stem')
    c1 = nm.Conv(c0, 8, (1, 3, 3), name='trunk')
    a = nm.Conv(c1, 3, (1, 1, 1), activation_func='lin', name='a')
    b = nm.Conv(c1, 3, (1, 1, 1), activation_func='lin', name='b', w=a.w, b=a.b)
    sms = [nm.Softmax(a, name='probs0'), nm.Softmax(b, name='probs1')]
    target = nm.Input_like(sms[0], override_f=2, name='target')
    parts = nm.split(target, 'f', n_out=2)
    nlls = [nm.MultinoulliNLL(s, t, target_is_sparse=True, name='nll%d' % k)
            for k, (s, t) in enumerate(zip(sms, parts))]
    loss = nm.AggregateLoss(nlls, mixing_weights=[1.5, 0.5], name='loss')
    pred = nm.Concat(sms, name='pred')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=pred)
    model.set_opt_meta_params('Adam', ADAM)
    model._classes = (3, 3)
    return model


def _s7(nm):
    inp = nm.Input((2, 1, 10, 10), 'b,f,x,y', name='raw')
    c0 = nm.Conv(inp, 4, (3, 3), (2, 2), name='stem')
    d0 = nm.Perceptron(c0, 8, flatten=True, name='dot0')
    a = nm.Perceptron(d0, 8, name='a')
    b = nm.Perceptron(a, 8, name='b', w=a.w, b=a.b)
    return _finish(nm, inp, nm.Perceptron(b, 3, activation_func='lin', name='head'), 's7')


def _s8(nm):
    inp = nm.Input((2, 1, 5, 18, 20), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 4, (1, 3, 3), name='stem')
    a = nm.Conv(c0, 4, (1, 3, 3), batch_normalisation='train', name='a')
    b = nm.Conv(a, 4, (1, 3, 3), (1, 2, 2), batch_normalisation='train', name='b',
                gamma=a.gamma, b=a.b)
    return _finish(nm, inp, nm.Conv(b, 2, (1, 1, 1), activation_func='lin', name='head'), 's8')


def _s9(nm):
    inp = nm.Input((1, 1, 5, 16, 18), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 4, (1, 3, 3), name='stem')
    a = nm.Conv(c0, 4, (1, 3, 3), name='a')
    b = nm.Conv(a, 4, (1, 3, 3), conv_mode='same', name='b', w=a.w)
    return _finish(nm, inp, nm.Conv(b, 2, (1, 1, 1), activation_func='lin', name='head'), 's9')


# name -> (builder, seed, keys the node 'b' takes from the node 'a')
NETS = {
    'S1': (_s1, 21, ('w', 'b')),
    'S2': (lambda nm: _s1(nm, same_sig=True), 42, ('w', 'b')),
    'S3': (_s3, 53, ('w', 'b')),
    'S4': (_s4, 14, ('w', 'b')),
    'S5': (_s5, 15, ('w', 'b')),
    'S6': (_s6, 16, ('w', 'b')),
    'S7': (_s7, 27, ('w', 'b')),
    'S8': (_s8, 18, ('gamma', 'b')),
    'S9': (_s9, 19, ('w',)),
}


def build(name):
    """a fresh model of net ``name``; same seed, same initial values every time"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    fn, seed, keys = NETS[name]
    np.random.seed(seed)
    m = fn(nm)
    rng = np.random.RandomState(seed + 100)
    for p in m.trainable_params:
        v = p.get_value()
        # every value away from its initial pattern (constant biases, the identity of an UpConv):
        # the contributions of the two users then differ element by element
        p.set_value((v + 0.1 * rng.standard_normal(v.shape) * max(float(np.abs(v).max()), 0.1))
                    .astype(np.float32))
    a, b = m.nodes['a'], m.nodes['b']
    for k in keys:
        assert getattr(b, k) is getattr(a, k)
    return m


def batch_for(m, seed):
    rng = np.random.RandomState(seed)
    x = rng.rand(*m.input_node.shape.shape).astype(np.float32)
    t = np.empty(m.target_node.shape.shape, np.float32)
    for k, c in enumerate(m._classes):
        tk = rng.randint(0, c, t[:, k].shape).astype(np.float32)
        tk[rng.rand(*tk.shape) < 0.08 + 0.2 * k] = -1             # unlabelled positions
        t[:, k] = tk
    return x, t


_REF = {}


def batch(r):
    """writable copies of a reference's input and target"""
    return r['x'].copy(), r['t'].copy()


def reference(name):
    """the reference numbers of net ``name``, computed once per process and shared read-only:
    loss / prediction / gradients at the initial values, the loss of each of N_STEPS Adam steps,
    the parameters after every step, prediction and gradients at the final values; and the two
    contributions to every shared gradient from the untied twin"""
    if name in _REF:
        return _REF[name]
    m = build(name)
    x, t = batch_for(m, NETS[name][1] + 200)
    ref = SRef(m)
    r = dict(x=x, t=t)
    r['loss0'], r['pred0'] = ref.loss_and_grads(x, t)
    r['grads0'] = [g.copy() for g in ref.grads()]
    twin = SRef(m, untied=True)
    r['twin_loss0'] = twin.loss_and_grads(x, t)[0]
    r['contrib'] = [(r['grads0'][[id(q) for q in m.trainable_params].index(k)], ga, gb)
                    for k, (ga, gb) in twin.contributions().items()]
    r['losses'], r['params'] = [], []
    for _ in range(N_STEPS):
        loss, _ = ref.loss_and_grads(x, t)
        ref.adam(**ADAM)
        r['losses'].append(loss)
        r['params'].append([ref.p(p).detach().numpy().copy() for p in m.trainable_params])
    r['loss_end'], r['pred_end'] = ref.loss_and_grads(x, t)
    r['grads_end'] = [g.copy() for g in ref.grads()]
    for v in r.values():
        for a in (v if isinstance(v, list) else [v]):
            for q in (a if isinstance(a, tuple) else (a,)):
                if isinstance(q, np.ndarray):
                    q.setflags(write=False)
    _REF[name] = r
    return r
