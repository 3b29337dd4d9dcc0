"""Nets in which one node's output feeds several consumers (their gradients are summed on the way
back) and their float64 reference, shared by tests/test_wiring_host.py and test_wiring_gpu.py.

``WRef`` is ``Ref`` of tests/test_conv_modes_host.py with the node kinds these nets add -- Pool in
every mode (``pool_ref`` of tests/test_pool_modes_host.py), LRN (``lrn_ref`` of
tests/test_lrn_host.py), Perceptron, SplitPart and an AggregateLoss of several sparse NLL terms (as
``SRef`` of tests/shared_param_cases.py restates them) -- and an EDGE SWITCH: ``edge=(parent name,
consumer name, slot, scale)`` hands that one consumer (its ``slot``-th parent) a ``v * 1.0`` copy
whose gradient is scaled on the way back: 0 drops that edge's contribution to the parent's
gradient, 2 doubles it; the forward numbers are unchanged.

Where the order can change a net comes in two orders (``flip``, the nets of ``FLIPPED``): the same graph with the parents of its merge node
swapped, so that ``Plan._bwd_nodes()`` -- ``plan.nodes`` reversed, and ``plan.nodes`` follows the
parents depth first -- reaches the consumers of the fan-out node in the other order, and the
first writer of its gradient becomes a later one."""
import numpy as np
import torch
import torch.nn.functional as F

from shared_param_cases import BF16_LOSS, BF16_GRAD        # noqa: F401  (the bf16 bounds of that suite)
from test_conv_modes_host import Ref, conv_ref
from test_lrn_host import lrn_ref
from test_pool_modes_host import pool_ref

ADAM = dict(lr=5e-4, mom=0.9, beta2=0.999, wd=0.5e-4)       # tests/test_model_gpu.py
TOL = 1e-4                                                  # tests/test_model_gpu.py:17
N_STEPS = 4


class WRef(Ref):
    def __init__(self, model, edge=None):
        Ref.__init__(self, model)
        self.edge = edge

    def take(self, val, parent, node, slot=0):
        """the value ``node`` reads from its ``slot``-th parent (through the edge switch)"""
        v = val[parent]
        e = self.edge
        if e is not None and (parent.name, node.name, slot) == tuple(e[:3]):
            scale = float(e[3])
            v = v * 1.0
            if v.requires_grad:
                v.register_hook(lambda g: g * scale)
            self.edge_seen = True
        return v

    def forward(self, x, t=None, upto=None):
        m = self.model
        self.min_pre = np.inf
        self.edge_seen = False
        val = {}
        for node in m.nodes.values():
            kind = type(node).__name__
            par = node.parent
            pars = list(par) if isinstance(par, (list, tuple)) else ([] if par is None else [par])
            if node is m.input_node:
                val[node] = torch.tensor(np.asarray(x, np.float64))
            elif node is m.target_node:
                if t is not None:
                    val[node] = torch.tensor(np.asarray(t, np.float64))
            elif any(q not in val for q in pars):
                continue                                     # (behind the target: no target given)
            elif kind in ('Conv', 'UpConv', 'Perceptron'):
                h, w, b = self.take(val, par, node), self.p(node.w), self.p(node.b)
                assert not node.batch_normalisation
                if kind == 'Perceptron':
                    y = (h.flatten(1) if node.flatten else h) @ w
                elif kind == 'UpConv':
                    y = F.conv_transpose3d(h, w.permute(1, 0, 2, 3, 4), stride=tuple(node.pool_shape))
                else:
                    y = conv_ref(h, w, node.conv_mode)
                    if any(q != 1 for q in node.pool_shape):
                        y = (F.max_pool3d if h.dim() == 5 else F.max_pool2d)(y, tuple(node.pool_shape))
                val[node] = self.act(node, y + b.view((1, -1) + (1,) * (y.dim() - 2)))
            elif kind == 'Pool':
                h = self.take(val, par, node)
                if node.mode == 'max':
                    assert tuple(node.pool_stride) == tuple(node.pool_shape)
                    val[node] = (F.max_pool3d if h.dim() == 5 else F.max_pool2d)(h, tuple(node.pool_shape))
                else:
                    val[node] = pool_ref(h, node.pool_shape, node.pool_stride, node.mode)
            elif kind == 'LRN':
                val[node] = lrn_ref(self.take(val, par, node), node.filter_shape, node.mode,
                                    self.p(node.alpha), self.p(node.k), self.p(node.beta))
            elif kind == 'Crop':
                val[node] = self.take(val, par, node)[node._slicer()]
            elif kind == 'Pad':
                pz, px, py = node.pad
                val[node] = F.pad(self.take(val, par, node), [py, py, px, px, pz, pz],
                                  value=float(node.value))
            elif kind == 'SplitPart':
                val[node] = val[par][:, node.lo:node.hi]
            elif kind == 'Concat':
                val[node] = torch.cat([self.take(val, q, node, i) for i, q in enumerate(par)], dim=1)
            elif kind == 'Add':
                val[node] = self.take(val, par[0], node, 0) + self.take(val, par[1], node, 1)
            elif kind == 'Softmax':
                val[node] = torch.softmax(self.take(val, par, node), dim=1)
            elif kind == 'MultinoulliNLL':
                pr, tg = val[par[0]], val[par[1]]
                C = pr.shape[1]
                classes = torch.arange(C, dtype=tg.dtype).view((1, C) + (1,) * (pr.dim() - 2))
                onehot = (tg == classes).to(pr.dtype)
                nll = -(onehot * torch.log(pr + 1e-5)) * pr.numel() / (onehot.sum() + 1e-5) / C
                val[node] = nll.sum(dim=1, keepdim=True)
            elif kind == 'AggregateLoss':
                if len(pars) == 1:
                    val[node] = val[pars[0]].mean()
                else:                      # weighted mean of the terms (loss.py, AggregateLoss)
                    w = node.mixing_weights.get_value().astype(np.float64)
                    val[node] = sum(float(w[k]) * val[q].mean() for k, q in enumerate(pars)) / len(pars)
            elif kind in ('Errors', '_Errors', 'Classification'):
                continue
            else:
                raise NotImplementedError(kind)
            if upto is not None and node is upto:
                return val[node]
        assert self.edge is None or self.edge_seen, "no such edge: %s" % (self.edge,)
        return (val.get(m.loss_node), val[m.prediction_node])


def fanouts(model):
    """[(node, [(consumer, slot), ...])] of every node whose output gradient has several writers:
    two or more reads by nodes on the loss path, and a trainable parameter upstream"""
    anc = model.loss_node.all_parents
    out = []
    for node in model.nodes.values():
        if node.name not in anc or node.is_source or not node.all_trainable_params:
            continue
        edges = []
        for c in node.children.values():
            if anc.get(c.name) is not c:
                continue
            ps = list(c.parent) if isinstance(c.parent, (list, tuple)) else [c.parent]
            edges += [(c, i) for i, q in enumerate(ps) if q is node]
        if len(edges) > 1:
            out.append((node, edges))
    return out


def writer_kind(c):
    """the kind of launch with which consumer ``c`` writes its parent's output gradient, as far as
    the graph alone tells (the GPU tests refine Conv by route and split-K parts)"""
    kind = type(c).__name__
    if kind == 'Conv':
        return 'conv_valid' if c._valid_mode() else 'conv_same'
    if kind == 'Pool':
        return 'maxpool' if c.mode == 'max' else 'avgpool'
    return kind.lower()


def writers(model, order):
    """{fan-out node name: [(consumer name, slot, kind), ...]} in the order in which ``order`` -- the
    nodes as the backward pass visits them -- reaches the consumers (a node given twice to one
    consumer: its parents in their order, as Add and Concat walk them)"""
    pos = dict((id(n), i) for i, n in enumerate(order))
    out = {}
    for node, edges in fanouts(model):
        es = sorted(edges, key=lambda e: (pos[id(e[0])], e[1]))
        out[node.name] = [(c.name, i, writer_kind(c)) for c, i in es]
    return out


def backward_order(model):
    """the rule of Plan._bwd_nodes on the graph alone: the loss node's ancestors, reversed"""
    return list(reversed(list(model.loss_node.all_parents.values())))


# (net, flip) -> {fan-out node: the consumer that writes its gradient FIRST}
FIRST = {
    ('residual', False): {'a': 'd'}, ('residual', True): {'a': 's'},
    ('unet_add', False): {'c1': 'crop'}, ('unet_add', True): {'c1': 'down'},
    ('unet_cat', False): {'c1': 'crop'}, ('unet_cat', True): {'c1': 'down'},
    ('head_kid', False): {'a': 'v'}, ('head_kid', True): {'a': 'u'},
    ('tail_shaped', False): {'b': 'side'}, ('tail_shaped', True): {'b': 't1'},
    ('tail_kid', False): {}, ('tail_plain', False): {},
    ('fan_same_avg', False): {'a': 'w_avgpool'}, ('fan_same_avg', True): {'a': 'w_same'},
    ('fan_up_lrn', False): {'a': 'w_lrn'}, ('fan_up_lrn', True): {'a': 'w_upconv'},
    ('fan_pad_max', False): {'a': 'w_maxpool'}, ('fan_pad_max', True): {'a': 'w_pad'},
    ('fan_crop_valid', False): {'a': 'w_valid'}, ('fan_crop_valid', True): {'a': 'w_crop'},
    ('fan_framed', False): {'a': 'w_pad'}, ('fan_framed', True): {'a': 'w_same'},
    ('cat_copy', False): {'a': 'd'}, ('cat_copy', True): {'a': 'cat'},
    ('twice', False): {'a': 's', 'cr': 'cat'},
    ('dense', False): {'a': 'p2'}, ('dense', True): {'a': 'p1'},
    ('two_valid', False): {'a': 'v'}, ('two_valid', True): {'a': 'u'},
    ('pred_trunk', False): {'a': 'v'}, ('pred_trunk', True): {'a': 'u'},
    ('mh_fused', False): {'a': 'head1'},          # (one launch writes for both heads)
    ('mh_third', False): {'a': 'side'}, ('mh_third', True): {'a': 'head0'},
}
# the writer kinds the graph alone tells apart; every one first and later somewhere in CASES
GRAPH_KINDS = ('conv_valid', 'conv_same', 'upconv', 'maxpool', 'avgpool', 'lrn', 'perceptron',
               'crop', 'pad', 'concat', 'add')


# ---- the nets ----------------------------------------------------------------------------------------
def _finish(nm, inp, logits, pred=None, debug=None):
    probs = nm.Softmax(logits, name='probs')
    target = nm.Input_like(probs, override_f=1, name='target')
    loss = nm.AggregateLoss(nm.MultinoulliNLL(probs, target, target_is_sparse=True), name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss,
                          prediction_node=probs if pred is None else pred, debug_outputs=debug)
    model.set_opt_meta_params('Adam', ADAM)
    model._classes = (logits.n_f,)
    return model


def _head(nm, x, n=2):
    return nm.Conv(x, n, (1, 1, 1), activation_func='lin', name='head')


def _add(nm, u, v, flip, name='merge'):
    return nm.Add(v, u, name=name) if flip else nm.Add(u, v, name=name)


def _residual(nm, flip):
    """`a` has three writers: the valid conv d, the Add s and the 'same' conv b"""
    inp = nm.Input((2, 1, 5, 14, 14), 'b,f,z,x,y', name='raw')
    a = nm.Conv(inp, 5, (1, 3, 3), name='a')
    b = nm.Conv(a, 5, (1, 3, 3), conv_mode='same', name='b')
    s = nm.Add(a, b, name='s')
    c = nm.Conv(s, 6, (3, 3, 3), name='c')
    d = nm.Conv(a, 6, (3, 3, 3), name='d')
    return _finish(nm, inp, _head(nm, _add(nm, c, d, flip)))


def _unet_add(nm, flip, mode='add'):
    """U-Net skip merged by Add (or, unet_cat, by a Concat that hands its parents slices of its own
    buffers): c1 -> max Pool and c1 -> Crop; the merge feeds a 'same' conv"""
    inp = nm.Input((2, 1, 6, 20, 20), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 6, (1, 3, 3), name='c0')
    c1 = nm.Conv(c0, 6, (3, 3, 3), name='c1')
    if flip:
        skip = nm.Crop(c1, (0, 2, 2), name='skip')
    low = nm.Conv(nm.Pool(c1, (1, 2, 2), name='down'), 8, (1, 3, 3), name='low')
    if flip:
        up = nm.UpConv(low, 6, (1, 2, 2), name='up')
        mg = nm.Add(skip, up, name='merge') if mode == 'add' else nm.Concat((skip, up), name='merge')
    else:
        mg = nm.UpConvMerge(c1, low, 6, merge_mode=mode, name='merge')
    post = nm.Conv(mg, 5, (1, 3, 3), conv_mode='same', name='post')
    return _finish(nm, inp, _head(nm, post))


def _head_kid(nm, flip):
    """the logits conv has a second child (off the loss path; an extra output of the training
    plans): not the form of a fused head (Conv._head_form, one child) -- the logits are made by the
    ordinary launches and the NLL writes their gradient"""
    inp = nm.Input((2, 1, 4, 12, 12), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 4, (1, 3, 3), name='c0')
    a = nm.Conv(c0, 6, (1, 3, 3), name='a')
    u = nm.Conv(a, 6, (1, 3, 3), name='u')
    v = nm.Conv(a, 6, (1, 3, 3), activation_func='tanh', name='v')
    head = _head(nm, _add(nm, u, v, flip))
    aux = nm.Conv(head, 3, (1, 1, 1), name='aux')
    return _finish(nm, inp, head, debug=[aux])


def _tail_shaped(nm, flip, form='fan'):
    """form 'fan': b feeds the (1,1,1) relu conv t1 and a tanh conv, added; 'kid': t1 -> head as in
    a tail, but t1 has a second child; 'plain': the tail itself (control)"""
    inp = nm.Input((1, 1, 4, 14, 14), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 8, (1, 3, 3), name='c0')
    b = nm.Conv(c0, 8, (2, 3, 3), name='b')
    t1 = nm.Conv(b, 12, (1, 1, 1), name='t1')
    if form == 'fan':
        side = nm.Conv(b, 12, (1, 1, 1), activation_func='tanh', name='side')
        return _finish(nm, inp, _head(nm, _add(nm, t1, side, flip)))
    head = _head(nm, t1)
    if form == 'kid':
        nm.Conv(t1, 3, (1, 1, 1), name='aux')             # (off the loss path)
    return _finish(nm, inp, head)


# one consumer branch of the fan-out node `a` (N, 6, 4, 10, 10), ending at (N, 6, 4, 8, 8); the
# FIRST node of each is the writer of a's gradient
def _branch(nm, kind, a):
    if kind == 'valid':
        return nm.Conv(a, 6, (1, 3, 3), name='w_valid')
    if kind == 'same':
        return nm.Crop(nm.Conv(a, 6, (1, 3, 3), conv_mode='same', name='w_same'), (0, 1, 1))
    if kind == 'upconv':
        u = nm.UpConv(a, 6, (1, 2, 2), identity_init=False, name='w_upconv')
        return nm.Crop(nm.Pool(u, (1, 2, 2), mode='average'), (0, 1, 1))
    if kind == 'maxpool':
        u = nm.UpConv(nm.Pool(a, (1, 2, 2), name='w_maxpool'), 6, (1, 2, 2), identity_init=False)
        return nm.Crop(u, (0, 1, 1))
    if kind == 'avgpool':
        return nm.Pool(a, (1, 3, 3), stride=(1, 1, 1), mode='average', name='w_avgpool')
    if kind == 'lrn':
        return nm.Crop(nm.LRN(a, (1, 3, 3), alpha=0.5, k=1.5, name='w_lrn'), (0, 1, 1))
    if kind == 'crop':
        return nm.Crop(a, (0, 1, 1), name='w_crop')
    if kind == 'pad':
        return nm.Crop(nm.Pad(a, (0, 1, 1), value=0.25, name='w_pad'), (0, 2, 2))
    raise ValueError(kind)


def _fan(nm, flip, kinds):
    inp = nm.Input((2, 1, 4, 14, 14), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 4, (1, 3, 3), name='c0')
    a = nm.Conv(c0, 6, (1, 3, 3), name='a')
    out = None
    for i, k in enumerate(kinds):      # ((u + v) + w) + ...; flipped: ... + (w + (v + u))
        b = _branch(nm, k, a)
        out = b if out is None else _add(nm, out, b, flip, name='merge%d' % i)
    post = nm.Conv(out, 6, (1, 3, 3), name='post')
    return _finish(nm, inp, _head(nm, post))


def _cat_copy(nm, flip):
    """a is a direct parent of a Concat (a copied slice: a has other children) and of two convs"""
    inp = nm.Input((2, 1, 4, 14, 14), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 4, (1, 3, 3), name='c0')
    a = nm.Conv(c0, 5, (1, 3, 3), name='a')
    b = nm.Conv(a, 3, (1, 3, 3), conv_mode='same', name='b')
    cat = nm.Concat((b, a) if flip else (a, b), name='cat')
    c = nm.Conv(cat, 6, (1, 3, 3), name='c')
    d = nm.Conv(a, 6, (1, 3, 3), name='d')
    return _finish(nm, inp, _head(nm, _add(nm, c, d, flip)))


def _twice(nm, flip):
    """one parent given twice: Add(a, a), then a Crop given twice to a Concat (which must not
    take the crop's gradient for a slice of its own: Concat._plan_alloc, `sole`)"""
    inp = nm.Input((2, 1, 4, 12, 12), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 4, (1, 3, 3), name='c0')
    a = nm.Conv(c0, 4, (1, 3, 3), name='a')
    s = nm.Add(a, a, name='s')
    cr = nm.Crop(s, (0, 1, 1), name='cr')
    cat = nm.Concat((cr, cr), name='cat')
    c = nm.Conv(cat, 6, (1, 3, 3), name='c')
    return _finish(nm, inp, _head(nm, c))


def _dense(nm, flip):
    """a conv output read by two Perceptrons (each flattens it)"""
    inp = nm.Input((2, 1, 3, 9, 9), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 3, (1, 3, 3), name='c0')
    a = nm.Conv(c0, 4, (1, 3, 3), (1, 1, 1), name='a')
    p1 = nm.Perceptron(a, 8, flatten=True, name='p1')
    p2 = nm.Perceptron(a, 8, flatten=True, activation_func='tanh', name='p2')
    out = nm.Perceptron(_add(nm, p1, p2, flip), 3, activation_func='lin', name='head')
    return _finish(nm, inp, out)


def _two_valid(nm, flip):
    """Conv -> two valid Convs: the split-K case and the second bf16 net"""
    inp = nm.Input((1, 1, 5, 16, 16), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 8, (1, 3, 3), name='c0')
    a = nm.Conv(c0, 12, (1, 3, 3), name='a')
    u = nm.Conv(a, 8, (3, 3, 3), name='u')               # (3 depth taps: K chunks to split)
    v = nm.Conv(a, 8, (3, 3, 3), activation_func='lin', name='v')
    return _finish(nm, inp, _head(nm, _add(nm, u, v, flip)))


def _pred_trunk(nm, flip):
    """the fused head's trunk is the model's prediction output and has a second, Softmax-free
    consumer; a (upstream) is read by the trunk and by that consumer's sibling on the loss path"""
    inp = nm.Input((2, 1, 4, 12, 12), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 4, (1, 3, 3), name='c0')
    a = nm.Conv(c0, 6, (1, 3, 3), name='a')
    u = nm.Conv(a, 6, (1, 1, 1), name='u')
    v = nm.Conv(a, 6, (1, 1, 1), activation_func='tanh', name='v')
    trunk = _add(nm, u, v, flip, name='trunk')
    head = _head(nm, trunk)
    aux = nm.Conv(trunk, 3, (1, 1, 1), name='aux')        # (off the loss path; an extra output
    return _finish(nm, inp, head, pred=trunk, debug=[aux])   # of the training plans)


def _multihead(nm, flip, third=False):
    """two softmax heads on one trunk (the fused multi-head launches); the trunk is also read by
    the Conv `side`: off the loss path, or (``third``) under a third head -- the heads then run as
    ordinary launches and the trunk's gradient has three writers"""
    inp = nm.Input((2, 1, 4, 12, 12), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 4, (1, 3, 3), name='c0')
    trunk = nm.Conv(c0, 8, (1, 3, 3), name='a')
    side = nm.Conv(trunk, 6, (1, 1, 1), name='side')
    h = [nm.Conv(trunk, 3, (1, 1, 1), activation_func='lin', name='head0'),
         nm.Conv(trunk, 2, (1, 1, 1), activation_func='lin', name='head1')]
    if third:
        h.append(nm.Conv(side, 2, (1, 1, 1), activation_func='lin', name='head2'))
    if flip:
        h = h[::-1]
    sms = [nm.Softmax(q, name='probs%d' % k) for k, q in enumerate(h)]
    target = nm.Input_like(sms[0], override_f=len(h), name='target')
    parts = nm.split(target, 'f', n_out=len(h))
    nlls = [nm.MultinoulliNLL(s, t, target_is_sparse=True, name='nll%d' % k)
            for k, (s, t) in enumerate(zip(sms, parts))]
    loss = nm.AggregateLoss(nlls, mixing_weights=[1.5, 0.5, 1.0][:len(h)], name='loss')
    pred = nm.Concat(sms, name='pred')
    model = nm.model_manager.getmodel()
    # (`side` without a head of its own: an extra output of the training plans, so that they hold it)
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=pred,
                          debug_outputs=None if third else [side])
    model.set_opt_meta_params('Adam', ADAM)
    model._classes = tuple(q.n_f for q in h)
    return model


# name -> (builder(nm, flip), seed); a seed was moved on where the reference met a kinked unit
# within MIN_PRE of zero (Ref.loss_and_grads refuses such a case)
NETS = {
    'residual': (_residual, 31),
    'unet_add': (_unet_add, 32),
    'unet_cat': (lambda nm, flip: _unet_add(nm, flip, 'concat'), 164),
    'head_kid': (_head_kid, 49),
    'tail_shaped': (_tail_shaped, 33),
    'tail_kid': (lambda nm, flip: _tail_shaped(nm, flip, 'kid'), 134),
    'tail_plain': (lambda nm, flip: _tail_shaped(nm, flip, 'plain'), 35),
    'fan_same_avg': (lambda nm, flip: _fan(nm, flip, ('same', 'avgpool')), 152),
    'fan_up_lrn': (lambda nm, flip: _fan(nm, flip, ('upconv', 'lrn')), 37),
    'fan_pad_max': (lambda nm, flip: _fan(nm, flip, ('pad', 'maxpool')), 38),
    'fan_crop_valid': (lambda nm, flip: _fan(nm, flip, ('crop', 'valid')), 139),
    # `a` lives inside the framed image of its 'same' consumer: every other consumer reads the
    # interior view, forward and backward
    'fan_framed': (lambda nm, flip: _fan(nm, flip, ('same', 'lrn', 'upconv', 'maxpool', 'pad')), 47),
    'cat_copy': (_cat_copy, 40),
    'twice': (_twice, 41),
    'dense': (_dense, 42),
    'two_valid': (_two_valid, 143),
    'pred_trunk': (_pred_trunk, 44),
    'mh_fused': (_multihead, 145),
    'mh_third': (lambda nm, flip: _multihead(nm, flip, third=True), 46),
}
# nets whose second order is a different plan (the others have one order, or none to swap)
FLIPPED = ('residual', 'unet_add', 'unet_cat', 'head_kid', 'tail_shaped', 'fan_same_avg', 'fan_up_lrn', 'fan_pad_max',
           'fan_crop_valid', 'fan_framed', 'cat_copy', 'dense', 'two_valid', 'pred_trunk', 'mh_third')
CASES = [(n, False) for n in sorted(NETS)] + [(n, True) for n in FLIPPED]
CASE_IDS = ["%s%s" % (n, '-flip' if f else '') for n, f in CASES]


def build(name, flip=False):
    """a fresh model of net ``name``; same seed, same initial values every time (and in both orders:
    the parameters are drawn per node, in the order of creation, which ``flip`` leaves alone except
    in unet_add and the multi-head nets)"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    fn, seed = NETS[name]
    np.random.seed(seed)
    m = fn(nm, flip)
    rng = np.random.RandomState(seed + 100)
    for p in [p for n in m.nodes.values() for p in n.params.values() if p.apply_train]:
        v = p.get_value()
        # every value away from its initial pattern (constant biases); in the order of creation
        p.set_value((v + 0.1 * rng.standard_normal(v.shape) * max(float(np.abs(v).max()), 0.1))
                    .astype(np.float32))
    return m


def batch_for(m, seed):
    rng = np.random.RandomState(seed)
    x = rng.rand(*m.input_node.shape.shape).astype(np.float32)
    t = np.empty(m.target_node.shape.shape, np.float32)
    for k, c in enumerate(m._classes):
        tk = rng.randint(0, c, t[:, k].shape).astype(np.float32)
        tk[rng.rand(*tk.shape) < 0.08 + 0.1 * k] = -1             # unlabelled positions
        t[:, k] = tk
    return x, t


_REF = {}


def batch(r):
    """writable copies of a reference's input and target"""
    return r['x'].copy(), r['t'].copy()


def reference(name, flip=False):
    """the reference numbers of a net, computed once per process and shared read-only: loss /
    prediction / gradients at the initial values, the loss of each of N_STEPS Adam steps, the
    parameters after every step, loss / prediction / gradients at the final values"""
    key = (name, bool(flip))
    if key in _REF:
        return _REF[key]
    m = build(name, flip)
    x, t = batch_for(m, NETS[name][1] + 200)
    ref = WRef(m)
    r = dict(x=x, t=t)
    r['loss0'], r['pred0'] = ref.loss_and_grads(x, t)
    r['grads0'] = [g.copy() for g in ref.grads()]
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
            for q in (a if isinstance(a, list) else [a]):
                if isinstance(q, np.ndarray):
                    q.setflags(write=False)
    _REF[key] = r
    return r
