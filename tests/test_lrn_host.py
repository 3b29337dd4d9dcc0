"""LRN node (local response normalisation, neural.py:2043-2181 of the reference), host side (no
GPU): the float64 restatement that tests/test_lrn_gpu.py compares every number against
(``lrn_ref``: avg_pool3d over the zero-framed squares for the spatial mode, a clamped index gather for the
channel mode, autograd for the backward; ``LrnRef`` for whole graphs -- never the kernels), pinned
here against a literal NumPy loop of the definition; the hand-derived backward formula the kernels
implement against autograd; that a window off by one moves the restatement far beyond the op
tolerance; constructor checks and bookkeeping of the node; the save -> modelload round trip; the
two prediction-time refusals."""
import functools
import itertools
import json
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_conv_modes_host import Ref, conv_ref
from test_pool_modes_host import pool_ref

TOL = 2e-5                                  # the op tolerance of tests/test_lrn_gpu.py
# the op tests: x = 2 randn, g = randn, and parameters far from the defaults (with alpha = 1e-4 the
# output differs from x by 1e-3 at most and no window error would show)
ALPHA, K, BETA = 0.7, 1.5, 0.75
OP_SHAPES = [(2, 3, 4, 5, 8), (1, 2, 3, 5, 7), (2, 5, 1, 3, 13), (1, 1, 1, 1, 3), (3, 7, 1, 1, 1),
             (1, 1, 5, 33, 34)]
OP_CONFIGS = [('spatial', (1, 3, 3)), ('spatial', (3, 3, 3)), ('spatial', (1, 5, 5)),
              ('channel', 3), ('channel', 5)]
OP_IDS = ["%s_%s" % (m, "".join(map(str, f)) if isinstance(f, tuple) else f) for m, f in OP_CONFIGS]


# ---- the float64 restatement ---------------------------------------------------------------------
def lrn_ref(x, filter_shape, mode, alpha, k, beta, with_q=False):
    """x: float64 torch tensor (n, c, *spatial) with 2 or 3 spatial axes; alpha / k / beta floats or
    0-d tensors.  out = x / (k + alpha * m) ** beta"""
    sq = x * x
    if mode == 'spatial':
        f = tuple(int(v) for v in filter_shape)
        assert len(f) == x.dim() - 2 and all(v % 2 == 1 for v in f)
        f3 = (1,) * (3 - len(f)) + f
        s5 = sq if x.dim() == 5 else sq.unsqueeze(2)
        # avg_pool3d over the explicitly zero-framed squares: what padding=f//2 with
        # count_include_pad=True computes, also where the window exceeds the axis (there
        # avg_pool3d refuses its own padding)
        h = [v // 2 for v in f3]
        m = F.avg_pool3d(F.pad(s5, [h[2], h[2], h[1], h[1], h[0], h[0]]), f3, stride=1)
        m = m if x.dim() == 5 else m.squeeze(2)
    else:
        assert mode == 'channel'
        f = int(filter_shape)
        assert f % 2 == 1
        C = x.shape[1]
        idx = torch.arange(C)
        m = sum(sq[:, torch.clamp(idx + o, 0, C - 1)] for o in range(-(f // 2), f // 2 + 1)) / f
    q = k + alpha * m
    out = x / q ** beta
    return (out, q) if with_q else out


def lrn_ref_fwd_bwd(x, g, filter_shape, mode, alpha=ALPHA, k=K, beta=BETA):
    """(out, q, dx) of numpy x and output gradient g through lrn_ref and torch autograd, float64"""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    out, q = lrn_ref(xt, filter_shape, mode, alpha, k, beta, with_q=True)
    out.backward(torch.tensor(np.asarray(g, np.float64)))
    return out.detach().numpy(), q.detach().numpy(), xt.grad.numpy()


def numpy_loop(x, filter_shape, mode, alpha, k, beta):
    """the definition by explicit loops over elements and window offsets (shares no code with
    torch): (out, q), x of shape (n, c, d, h, w)"""
    x = np.asarray(x, np.float64)
    N, C, D, H, W = x.shape
    q = np.zeros(x.shape)
    for n, c, z, y, w in itertools.product(range(N), range(C), range(D), range(H), range(W)):
        s = 0.0
        if mode == 'spatial':
            fz, fy, fx = filter_shape
            for oz in range(-(fz // 2), fz // 2 + 1):
                for oy in range(-(fy // 2), fy // 2 + 1):
                    for ox in range(-(fx // 2), fx // 2 + 1):
                        a, b, d = z + oz, y + oy, w + ox
                        if 0 <= a < D and 0 <= b < H and 0 <= d < W:
                            s += x[n, c, a, b, d] ** 2
            s /= fz * fy * fx
        else:
            for o in range(-(filter_shape // 2), filter_shape // 2 + 1):
                s += x[n, min(max(c + o, 0), C - 1), z, y, w] ** 2
            s /= filter_shape
        q[n, c, z, y, w] = k + alpha * s
    return x / q ** beta, q


def channel_mult(C, f):
    """mult[i, j] = the number of o in [-f//2, f//2] with clamp(j + o, 0, C - 1) == i"""
    mult = np.zeros((C, C))
    for j in range(C):
        for o in range(-(f // 2), f // 2 + 1):
            mult[min(max(j + o, 0), C - 1), j] += 1
    return mult


def lrn_bwd_formula(x, g, filter_shape, mode, alpha, k, beta):
    """the backward the kernels implement, written out by hand (float64 NumPy):
    t = g x q^(-beta-1);  dx_i = g_i q_i^(-beta) - (2 alpha beta / N) x_i sum_j mult(i, j) t_j"""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    _, q = [np.asarray(a) for a in lrn_ref_fwd_bwd(x, g, filter_shape, mode, alpha, k, beta)[:2]]
    t = g * x * q ** (-beta - 1)
    if mode == 'spatial':
        f = tuple(filter_shape)
        n_win = float(np.prod(f))
        h = [v // 2 for v in f]
        tp = np.pad(t, [(0, 0), (0, 0)] + [(v, v) for v in h])           # t = 0 outside
        S = np.zeros(x.shape)
        D, H, W = x.shape[2:]
        for oz, oy, ox in itertools.product(range(f[0]), range(f[1]), range(f[2])):
            S += tp[:, :, oz:oz + D, oy:oy + H, ox:ox + W]
    else:
        n_win = float(filter_shape)
        S = np.einsum('ij,njzyx->nizyx', channel_mult(x.shape[1], filter_shape), t)
    return g * q ** (-beta) - (2 * alpha * beta / n_win) * x * S


def lrn_shrunk(x, filter_shape, mode, alpha, k, beta):
    """the restatement with every window one short at its upper end (offsets [-f//2, f//2 - 1] along
    each windowed axis, divisor unchanged): the mistake a wrong loop bound makes"""
    sq = x * x
    if mode == 'spatial':
        f = tuple(filter_shape)
        h = [v // 2 for v in f]
        sp = F.pad(sq, [h[2], h[2], h[1], h[1], h[0], h[0]])
        D, H, W = x.shape[2:]
        m = 0
        for oz, oy, ox in itertools.product(*[range(v if v == 1 else v - 1) for v in f]):
            m = m + sp[:, :, oz:oz + D, oy:oy + H, ox:ox + W]
        m = m / float(np.prod(f))
    else:
        f = int(filter_shape)
        C = x.shape[1]
        idx = torch.arange(C)
        m = sum(sq[:, torch.clamp(idx + o, 0, C - 1)] for o in range(-(f // 2), f // 2)) / f
    return x / (k + alpha * m) ** beta


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@functools.lru_cache(maxsize=None)
def op_case(shape, mode, filter_shape):
    """(x, g, reference out, q, dx) of one op-test configuration: made once, shared, read-only"""
    rng = np.random.RandomState(zlib.crc32(repr((shape, mode, filter_shape)).encode()))
    x = (2 * rng.randn(*shape)).astype(np.float32)
    g = rng.randn(*shape).astype(np.float32)
    out, q, dx = lrn_ref_fwd_bwd(x, g, filter_shape, mode)
    for a in (x, g, out, q, dx):
        a.setflags(write=False)
    return x, g, out, q, dx


# ---- 1. the restatement ----------------------------------------------------------------------------
TINY = [('spatial', (1, 3, 3), (1, 2, 2, 4, 5)), ('spatial', (3, 3, 3), (1, 1, 3, 3, 4)),
        ('spatial', (1, 5, 5), (1, 1, 1, 3, 4)),                  # the window exceeds both axes
        ('channel', 3, (2, 1, 1, 2, 3)), ('channel', 3, (1, 2, 2, 2, 3)), ('channel', 3, (1, 5, 1, 2, 3)),
        ('channel', 5, (2, 2, 1, 1, 3))]


@pytest.mark.parametrize("mode,f,shape", TINY, ids=["%s_%s_C%d" % (m, f, s[1]) for m, f, s in TINY])
def test_restatement_equals_the_numpy_loop_and_the_hand_derived_backward(mode, f, shape):
    rng = np.random.RandomState(5)
    x, g = 2 * rng.randn(*shape), rng.randn(*shape)
    for alpha, k, beta in ((ALPHA, K, BETA), (1e-4, 1.0, 0.75), (2.0, 0.5, 1.25)):
        out, q, dx = lrn_ref_fwd_bwd(x, g, f, mode, alpha, k, beta)
        want_out, want_q = numpy_loop(x, f, mode, alpha, k, beta)
        assert np.abs(out - want_out).max() < 1e-12
        assert np.abs(q - want_q).max() < 1e-12
        assert np.abs(dx - lrn_bwd_formula(x, g, f, mode, alpha, k, beta)).max() < 1e-10


def test_channel_multiplicities_at_the_replicated_edges():
    assert np.array_equal(channel_mult(1, 3), [[3]])
    assert np.array_equal(channel_mult(2, 3), [[2, 1], [1, 2]])
    assert np.array_equal(channel_mult(2, 5), [[3, 2], [2, 3]])
    m = channel_mult(5, 3)
    assert m[0, 0] == 2 and m[4, 4] == 2 and m[0, 1] == 1 and m[2, 2] == 1 and m[0, 2] == 0
    for C, f in ((1, 3), (2, 3), (5, 3), (2, 5), (7, 5)):
        assert np.all(channel_mult(C, f).sum(axis=0) == f)        # every offset lands somewhere


def test_2d_inputs_are_the_3d_restatement_with_a_unit_z_axis():
    rng = np.random.RandomState(6)
    x = torch.tensor(rng.randn(2, 3, 6, 7))
    a = lrn_ref(x, (3, 5), 'spatial', ALPHA, K, BETA)
    b = lrn_ref(x.unsqueeze(2), (1, 3, 5), 'spatial', ALPHA, K, BETA).squeeze(2)
    assert torch.equal(a, b)


@pytest.mark.parametrize("mode,f", OP_CONFIGS, ids=OP_IDS)
def test_a_window_one_short_moves_the_restatement_far_beyond_the_op_tolerance(mode, f):
    """at every shape of the op tests that has room for one whole window along a windowed axis.
    Where the window exceeds every axis it walks along, nearly every sum is the whole row whatever
    the bounds are: on (3, 7, 1, 1, 1) a spatial window reaches nothing but the element itself
    (no difference at all), on the three elements of (1, 1, 1, 1, 3) a (1, 5, 5) window loses one
    term of one sum (1.6e-3 / 5.0e-3, printed below) -- those shapes test the borders, not this."""
    done = 0
    for shape in OP_SHAPES:
        x, g, out, q, dx = op_case(shape, mode, f)
        xt = torch.tensor(x.astype(np.float64), requires_grad=True)
        bad = lrn_shrunk(xt, f, mode, ALPHA, K, BETA)
        bad.backward(torch.tensor(g.astype(np.float64)))
        e_f, e_b = rel(bad.detach().numpy(), out), rel(xt.grad.numpy(), dx)
        print(mode, f, shape, "forward %.3g backward %.3g" % (e_f, e_b))
        if mode == 'spatial' and all(e < w or w == 1 for e, w in zip(shape[2:], f)):
            continue
        assert e_f > 100 * TOL and e_b > 100 * TOL, (shape, e_f, e_b)
        done += 1
    assert done >= 4


# ---- 2. the node -----------------------------------------------------------------------------------
def _nm():
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    return nm


def test_constructor_errors():
    nm = _nm()
    inp = nm.Input((1, 4, 6, 12, 12), 'b,f,z,x,y', name='raw')
    with pytest.raises(ValueError, match="in \\+ 1"):
        nm.LRN(inp, (1, 2, 3))                                    # even extent
    with pytest.raises(ValueError):
        nm.LRN(inp, (1, 0, 3))
    with pytest.raises(ValueError):
        nm.LRN(inp, (1, 3.0, 3))
    with pytest.raises(ValueError, match="filter_shape dimensionality \\(2\\) and the number of "
                                         "spatial dimensions in the input \\(3\\)differ"):
        nm.LRN(inp, (3, 3))                                       # wrong tuple length
    with pytest.raises(ValueError):
        nm.LRN(inp, 3)                                            # spatial wants a tuple
    for bad in (4, 0, -1, 3.0, (3,), None):
        with pytest.raises(ValueError):
            nm.LRN(inp, bad, mode='channel')                      # even / non-int channel window
    with pytest.raises(ValueError, match="Unknow mode across"):
        nm.LRN(inp, (1, 3, 3), mode='across')
    flat = nm.Input((2, 8), 'b,f', name='flat')
    with pytest.raises(NotImplementedError):
        nm.LRN(flat, 3, mode='channel')
    odd = nm.Input((1, 6, 4, 12, 12), 'b,z,f,x,y', name='odd')
    with pytest.raises(NotImplementedError):
        nm.LRN(odd, (1, 3, 3))
    with pytest.raises(NotImplementedError):
        nm.LRN(odd, 3, mode='channel')
    one_d = nm.Input((1, 4, 12), 'b,f,x', name='one_d')
    with pytest.raises(NotImplementedError):
        nm.LRN(one_d, (3,))
    with pytest.raises(NotImplementedError):
        nm.LRN(one_d, 3, mode='channel')
    # what is accepted: an extent beyond its axis, unit windows, both 2-D orders
    assert nm.LRN(inp, (7, 13, 1)).filter_shape == (7, 13, 1)
    assert nm.LRN(inp, (1, 1, 1)).filter_shape == (1, 1, 1)
    assert nm.LRN(inp, np.int64(9), mode='channel').filter_shape == 9
    for tags in ('b,f,x,y', 'b,f,y,x'):
        img = nm.Input((2, 3, 12, 14), tags, name='img')
        assert nm.LRN(img, (3, 5))._f3 == (1, 3, 5)
        assert nm.LRN(img, 3, mode='channel')._f3 == (3, 1, 1)


@pytest.mark.parametrize("mode,f", [('spatial', (1, 3, 5)), ('channel', 5)])
def test_bookkeeping_is_the_parents(mode, f):
    nm = _nm()
    inp = nm.Input((2, 1, 6, 22, 22), 'b,f,z,x,y', name='raw')
    par = nm.Conv(inp, 6, (1, 3, 3), (1, 2, 2))
    node = nm.LRN(par, f, mode=mode, alpha=0.3, k=2, beta=0.5)
    assert tuple(node.shape.shape) == tuple(par.shape.shape) == (2, 6, 6, 10, 10)
    assert tuple(node.shape.tags) == tuple(par.shape.tags)
    assert tuple(int(v) for v in node.shape.strides) == tuple(int(v) for v in par.shape.strides) == (1, 2, 2)
    assert tuple(node.shape.fov) == tuple(par.shape.fov)
    assert tuple(node.shape.offsets) == tuple(par.shape.offsets)
    assert list(node.params) == ['alpha', 'beta', 'k']                    # no average_filter
    for key, v in (('alpha', 0.3), ('beta', 0.5), ('k', 2.0)):
        p = node.params[key]
        assert p is getattr(node, key)
        assert not p.apply_train and p.name == key + "_noTrain" and p.shape == ()
        assert p.get_value() == np.float32(v) and p.get_value().dtype == np.float32
    assert node.param_count == 0
    assert node.computational_cost == 2 * 6 * 6 * 10 * 10 * (15 if mode == 'spatial' else 5)
    assert not any(k.startswith(node.name) for k in node.all_trainable_params)
    dflt = nm.LRN(par, f, mode=mode, name='dflt')
    assert [float(dflt.params[k].get_value()) for k in ('alpha', 'k', 'beta')] == \
        [float(np.float32(1e-4)), 1.0, 0.75]


def test_lrn_is_exported():
    from elektronn2_amd import backend, neuromancer as nm
    from elektronn2_amd.neuromancer import neural
    assert 'LRN' in neural.__all__ and nm.LRN is neural.LRN
    assert {'e2_lrn_fwd', 'e2_lrn_bwd'} <= set(backend.EXPORTED_SYMBOLS)
    assert backend.LRN_MODE == {'spatial': 0, 'channel': 1}


# ---- 3. whole graphs -------------------------------------------------------------------------------
class LrnRef(Ref):
    """``Ref`` of tests/test_conv_modes_host.py with an LRN branch (parameters read from the node:
    ``set_params`` follows a ``set_value``), Pool in every mode, the Perceptron of the 2-D net, and
    the value of every node kept (``self.val``; the parents of LRN nodes retain their gradient)."""

    def set_params(self, node):
        for p in node.params.values():
            self.P[id(p)] = torch.tensor(p.get_value().astype(np.float64), requires_grad=bool(p.apply_train))

    def forward(self, x, t=None, upto=None):
        m = self.model
        self.min_pre = np.inf
        val = self.val = {}
        lrn_parents = set(id(n.parent) for n in m.nodes.values() if type(n).__name__ == 'LRN')
        for node in m.nodes.values():
            kind = type(node).__name__
            par = node.parent
            if node is m.input_node:
                val[node] = torch.tensor(np.asarray(x, np.float64))
            elif node is m.target_node:
                if t is None:
                    continue
                val[node] = torch.tensor(np.asarray(t, np.float64))
            elif kind in ('Conv', 'UpConv'):
                h, w, b = val[par], self.p(node.w), self.p(node.b)
                nd = h.dim() - 2
                if kind == 'UpConv':
                    y = F.conv_transpose3d(h, w.permute(1, 0, 2, 3, 4), stride=tuple(node.pool_shape))
                else:
                    y = conv_ref(h, w, node.conv_mode)
                    if any(q != 1 for q in node.pool_shape):
                        y = (F.max_pool3d if nd == 3 else F.max_pool2d)(y, tuple(node.pool_shape))
                if node.batch_normalisation == 'train':
                    y = self.bn(y, self.p(node.gamma), b, [i for i in range(y.dim()) if i != 1])
                else:
                    assert not node.batch_normalisation
                    y = y + b.view((1, -1) + (1,) * nd)
                val[node] = self.act(node, y)
            elif kind == 'LRN':
                val[node] = lrn_ref(val[par], node.filter_shape, node.mode, self.p(node.alpha),
                                    self.p(node.k), self.p(node.beta))
            elif kind == 'Perceptron':
                h = val[par].flatten(1) if node.flatten else val[par]
                assert not node.batch_normalisation
                val[node] = self.act(node, h @ self.p(node.w) + self.p(node.b))
            elif kind == 'Pool':
                h = val[par]
                if node.mode == 'max':
                    val[node] = (F.max_pool3d if h.dim() == 5 else F.max_pool2d)(h, tuple(node.pool_shape))
                else:
                    val[node] = pool_ref(h, node.pool_shape, node.pool_stride, node.mode)
            elif kind == 'Crop':
                val[node] = val[par][node._slicer()]
            elif kind == 'Concat':
                val[node] = torch.cat([val[q] for q in par], dim=1)
            elif kind == 'Softmax':
                val[node] = torch.softmax(val[par], dim=1)
            elif kind == 'MultinoulliNLL':
                if t is None:
                    continue
                pr, tg = val[par[0]], val[par[1]]
                C = pr.shape[1]
                classes = torch.arange(C, dtype=tg.dtype).view((1, C) + (1,) * (pr.dim() - 2))
                onehot = (tg == classes).to(pr.dtype)
                nll = -(onehot * torch.log(pr + 1e-5)) * pr.numel() / (onehot.sum() + 1e-5) / C
                val[node] = nll.sum(dim=1, keepdim=True)
            elif kind == 'AggregateLoss':
                if t is None:
                    continue
                val[node] = val[par[0] if isinstance(par, (list, tuple)) else par].mean()
            elif kind == 'Errors':
                continue
            else:
                raise NotImplementedError(kind)
            if id(node) in lrn_parents and val[node].requires_grad:
                val[node].retain_grad()
            if upto is not None and node is upto:
                return val[node]
        return (val.get(m.loss_node), val[m.prediction_node])

    def lrn_parent_grads(self):
        """{LRN node: d loss / d (its parent's output)} of the last loss_and_grads"""
        return dict((n, self.val[n.parent].grad.numpy()) for n in self.model.nodes.values()
                    if type(n).__name__ == 'LRN')


ADAM = dict(lr=5e-4, mom=0.9, beta2=0.999, wd=0.5e-4)
LRN_KW = dict(alpha=ALPHA, k=K, beta=BETA)


def _finish(nm, inp, logits):
    probs = nm.Softmax(logits)
    target = nm.Input_like(probs, override_f=1, name='target')
    loss = nm.AggregateLoss(nm.MultinoulliNLL(probs, target, target_is_sparse=True), name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=probs,
                          prediction_ext=[loss, probs])
    model.set_opt_meta_params('Adam', ADAM)
    return model


def net_chain(batch=2, seed=71, lrn=True, sp=(6, 22, 22), mode1='channel'):
    """(a) relu Conv -> LRN spatial (1,3,3) -> relu Conv with pooling -> LRN channel 3 -> relu Conv
    -> (1,1,1) 'lin' Conv -> Softmax / NLL; ``lrn=False``: the same net without the two nodes"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 1) + tuple(sp), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 6, (1, 3, 3), name='c0')                             # (6, 20, 20)
    if lrn:
        out = nm.LRN(out, (1, 3, 3), name='lrn_s', **LRN_KW)
    out = nm.Conv(out, 8, (1, 3, 3), (1, 2, 2), name='c1')                  # (6, 9, 9)
    if lrn:
        out = nm.LRN(out, 3 if mode1 == 'channel' else (1, 3, 3), mode=mode1, name='lrn_c', **LRN_KW)
    out = nm.Conv(out, 8, (3, 3, 3), name='c2')                             # (4, 7, 7)
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin', name='head')
    return _finish(nm, inp, out)


def net_unet(batch=1, seed=72):
    """(b) the U-Net of tests/test_activations_gpu.py (relu throughout) with a channel LRN on the
    skip branch that feeds the merge: its output reaches the Concat's buffer through the Crop view,
    and its parent feeds the LRN and the Pool -- two writers of one gradient"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 1, 6, 20, 20), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 8, (1, 3, 3))
    c1 = nm.Conv(c0, 8, (1, 3, 3), name='enc')
    skip = nm.LRN(c1, 3, mode='channel', name='lrn_skip', **LRN_KW)
    p1 = nm.Pool(c1, (1, 2, 2))
    c2 = nm.Conv(p1, 16, (3, 3, 3))
    c3 = nm.Conv(c2, 16, (3, 3, 3))
    mrg = nm.UpConvMerge(skip, c3, 24)
    c4 = nm.Conv(mrg, 8, (1, 3, 3))
    out = nm.Conv(c4, 2, (1, 1, 1), activation_func='lin')
    return _finish(nm, inp, out)


def net_2d(batch=2, seed=73, tags='b,f,y,x'):
    """(c) 2-D convs and Perceptrons in the style of config 1, a spatial (3,3) LRN behind a Conv with
    train-mode batch normalisation"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 1, 26, 26), tags, name='raw')
    out = nm.Conv(inp, 12, (3, 3), (2, 2), batch_normalisation='train')     # (12, 12)
    out = nm.LRN(out, (3, 3), name='lrn_s', **LRN_KW)
    out = nm.Conv(out, 16, (3, 3), (2, 2))                                  # (5, 5)
    out = nm.Perceptron(out, 32, flatten=True)
    out = nm.Perceptron(out, 10, activation_func='lin')
    return _finish(nm, inp, out)


# name, constructor, classes, seed of the batch per batch size (chosen on the float64 reference
# alone: MIN_PRE of test_conv_modes_host.py holds over every evaluation the GPU tests make)
NETS = [("chain", net_chain, 2, {1: 62, 2: 62}), ("unet", net_unet, 2, {1: 66, 2: 81}),
        ("2d", net_2d, 10, {1: 61, 2: 63})]
NET_CASES = [(name, make, ncls, b, seeds[b]) for name, make, ncls, seeds in NETS for b in (1, 2)]
NET_IDS = ["%s_b%d" % (c[0], c[3]) for c in NET_CASES]


def batch_for(model, seed, n_class=2):
    rng = np.random.RandomState(seed)
    x = rng.rand(*model.input_node.shape.shape).astype(np.float32)
    t = rng.randint(0, n_class, model.target_node.shape.shape).astype(np.float32)
    if t.ndim == 5:
        t.flat[::17] = -1                          # unlabelled voxels
    return x, t


def lrn_nodes(m):
    return [n for n in m.nodes.values() if type(n).__name__ == 'LRN']


@pytest.mark.parametrize("name,make,ncls,batch,data_seed", NET_CASES, ids=NET_IDS)
def test_restated_nets_run_on_the_cpu(name, make, ncls, batch, data_seed):
    """every evaluation the GPU tests make (the first call and three Adam steps) passes MIN_PRE;
    every parameter and every LRN parent receives a gradient; alpha, k, beta receive none"""
    m = make(batch=batch)
    x, t = batch_for(m, data_seed, ncls)
    ref = LrnRef(m)
    for step in range(4):
        loss, probs = ref.loss_and_grads(x, t)            # asserts MIN_PRE
        assert np.isfinite(loss)
        assert all(np.abs(g).max() > 0 for g in ref.grads())
        for node, g in ref.lrn_parent_grads().items():
            assert g.shape == tuple(node.parent.shape.shape) and np.abs(g).max() > 0
            assert all(ref.p(p).grad is None for p in node.params.values())
        ref.adam(**ADAM)
    assert len(lrn_nodes(m)) == (2 if name == 'chain' else 1)


def sharpen(model, factor=40.0):
    """scale the head's weights: at initialisation the logits are nearly 0 and the loss nearly ln 2
    whatever the layers below compute; with a sharper head the loss itself depends on them"""
    w = model.nodes['head'].w
    w.set_value(w.get_value() * np.float32(factor))


def test_the_lrn_nodes_matter_to_the_nets():
    """net (a), on the reference alone: the first conv's weight gradient with and without the nodes
    differs by far more than the step tolerance, and so does the loss under a sharpened head when
    alpha, k, beta change -- what the GPU test of parameters read in place relies on"""
    a, b = net_chain(), net_chain(lrn=False)
    x, t = batch_for(a, 62)
    ra, rb = LrnRef(a), LrnRef(b)
    ra.loss_and_grads(x, t); rb.loss_and_grads(x, t)
    assert rel(ra.p(a.nodes['c0'].w).grad.numpy(), rb.p(b.nodes['c0'].w).grad.numpy()) > 1e-2
    sharpen(a)
    ra = LrnRef(a)
    before = ra.loss_and_grads(x, t)[0]
    for node, (al, k, be) in zip(lrn_nodes(a), NEW_PARAMS):
        node.alpha.set_value(al); node.k.set_value(k); node.beta.set_value(be)
        ra.set_params(node)
    after = ra.loss_and_grads(x, t)[0]
    assert abs(after - before) / abs(before) > 100 * 1e-4, (before, after)


# (alpha, k, beta) the GPU test sets on the two LRN nodes of net (a) under a captured step
NEW_PARAMS = [(2.0, 0.8, 1.1), (0.2, 2.5, 0.4)]


# ---- 4. save / modelload and the prediction-time rewrites ------------------------------------------
def test_graph_descriptors_round_trip(tmp_path):
    nm = _nm()
    m = net_chain()
    m.nodes['lrn_s'].beta.set_value(0.6)
    f = str(tmp_path / "lrn.mdl")
    m.save(f)
    descr = json.loads(str(np.load(f, allow_pickle=False)["meta/graph"]))["nodes"]
    assert sum(1 for n in descr if n[1] == 'LRN') == 2

    def lrns(model):
        return [(n.name, n.mode, n.filter_shape, type(n.filter_shape), tuple(n.shape.shape),
                 [float(n.params[k].get_value()) for k in ('alpha', 'k', 'beta')])
                for n in lrn_nodes(model)]
    want = lrns(m)
    assert [w[1:4] for w in want] == [('spatial', (1, 3, 3), tuple), ('channel', 3, int)]
    assert want[0][5] == [float(np.float32(ALPHA)), K, float(np.float32(0.6))]
    m2 = nm.modelload(f, name='again')
    assert lrns(m2) == want
    m3 = nm.modelload(f, name='batch5', imposed_batch_size=5)
    assert [g[:4] + g[5:] for g in lrns(m3)] == [w[:4] + w[5:] for w in want]
    assert [g[4][0] for g in lrns(m3)] == [5, 5]


def test_prediction_time_rewrites_refuse_the_spatial_mode_and_name_the_node(tmp_path):
    nm = _nm()
    m = net_chain(batch=None)
    f = str(tmp_path / "lrn.mdl")
    m.save(f)
    with pytest.raises(NotImplementedError, match="lrn_s"):
        m.prediction_node.predict_dense(np.zeros((1, 8, 30, 30), np.float32))
    with pytest.raises(NotImplementedError, match="lrn_s"):
        nm.modelload(f, name='mfp', override_mfp_to_active=True)
    # the channel mode is pointwise in space: both rewrites go through it
    nm.model_manager.reset()
    np.random.seed(3)
    inp = nm.Input((1, 1, 6, 22, 22), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 6, (1, 3, 3), (1, 2, 2))
    out = nm.LRN(out, 3, mode='channel', name='lrn_c', **LRN_KW)
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin')
    mc = _finish(nm, inp, out)
    f2 = str(tmp_path / "lrn_c.mdl")
    mc.save(f2)
    dense = nm.modelload(f2, name='mfp_c', override_mfp_to_active=True)
    assert [n.mode for n in lrn_nodes(dense)] == ['channel']
    assert any(type(n).__name__ == 'FragmentsToDense' for n in dense.nodes.values())
