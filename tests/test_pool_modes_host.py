"""Pool modes 'average' / 'average_inc_pad' / 'average_exc_pad' / 'sum' with a stride of their own
and 2-D Pool nodes, host side (no GPU): the float64 restatement that tests/test_pool_modes_gpu.py
compares every number against (``pool_ref`` and ``PoolRef``; never the kernels), pinned here against
an explicit NumPy sliding-window loop; shape / stride / fov / offset bookkeeping of the Pool node
(neural.py:1528-1559 of the reference); every rejected argument; the save -> modelload round trip."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_conv_modes_host import Ref, conv_ref

# (pool | stride): plain, no z pooling, overlap, dense overlap, gaps, a window wider than a quad,
# z-only overlap, subsampling, copy
WINDOWS = [((2, 2, 2), (2, 2, 2)), ((1, 2, 2), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)),
           ((2, 3, 3), (1, 1, 1)), ((1, 2, 2), (1, 3, 3)), ((1, 1, 5), (1, 1, 2)),
           ((2, 1, 1), (1, 1, 1)), ((1, 1, 1), (2, 2, 2)), ((1, 1, 1), (1, 1, 1))]
WINDOW_IDS = ["%s_%s" % ("".join(map(str, p)), "".join(map(str, s))) for p, s in WINDOWS]
INPUTS = [(2, 3, 4, 5, 8), (1, 2, 3, 7, 9), (1, 1, 2, 3, 19), (1, 1, 5, 33, 34), (3, 7, 1, 1, 1)]
LINEAR_MODES = ('average', 'average_inc_pad', 'average_exc_pad', 'sum')
ALL_MODES = ('max',) + LINEAR_MODES


# ---- the float64 restatement ---------------------------------------------------------------------
def pool_ref(x, pool, stride, mode):
    """x: float64 torch tensor (n, c, *spatial), 2 or 3 spatial axes; pad 0, extent
    floor((in - p) / s) + 1; mode 'avg' / 'sum' (or a Pool node's mode string)"""
    nd = x.dim() - 2
    pool, stride = tuple(int(v) for v in pool), tuple(int(v) for v in stride)
    y = (F.avg_pool3d if nd == 3 else F.avg_pool2d)(x, pool, stride)
    if mode == 'sum':
        y = y * float(np.prod(pool))
    else:
        assert mode in ('avg', 'average', 'average_inc_pad', 'average_exc_pad'), mode
    return y


def pool_ref_fwd_bwd(x, dout, pool, stride, mode):
    """(out, dx) of numpy x and dout through pool_ref and torch autograd, float64"""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    out = pool_ref(xt, pool, stride, mode)
    out.backward(torch.tensor(np.asarray(dout, np.float64)))
    return out.detach().numpy(), xt.grad.numpy()


def out_extent(sp, pool, stride):
    return tuple((i - p) // s + 1 for i, p, s in zip(sp, pool, stride))


def numpy_loop(x, dout, pool, stride, mode):
    """the same by explicit loops over outputs and window offsets (shares no code with torch);
    also returns the mask of input elements that no window covers"""
    x = np.asarray(x, np.float64)
    n, c = x.shape[:2]
    osp = out_extent(x.shape[2:], pool, stride)
    scale = 1.0 if mode == 'sum' else 1.0 / float(pool[0] * pool[1] * pool[2])
    out = np.zeros((n, c) + osp)
    dx = np.zeros(x.shape)
    covered = np.zeros(x.shape[2:], bool)
    for oz in range(osp[0]):
        for ox in range(osp[1]):
            for oy in range(osp[2]):
                for dz in range(pool[0]):
                    for dx_ in range(pool[1]):
                        for dy in range(pool[2]):
                            z, a, b = oz * stride[0] + dz, ox * stride[1] + dx_, oy * stride[2] + dy
                            out[:, :, oz, ox, oy] += x[:, :, z, a, b]
                            if dout is not None:
                                dx[:, :, z, a, b] += scale * dout[:, :, oz, ox, oy]
                            covered[z, a, b] = True
    return out * scale, dx, ~covered


class PoolRef(Ref):
    """``Ref`` of tests/test_conv_modes_host.py with a Pool branch that honours ``mode`` and
    ``stride`` (and 2-D parents), the Perceptron of the 2-D net, and the value of every node kept
    (``self.val``; the parents of Pool nodes retain their gradient)."""

    def forward(self, x, t=None, upto=None):
        m = self.model
        self.min_pre = np.inf
        val = self.val = {}
        pool_parents = set(id(n.parent) for n in m.nodes.values() if type(n).__name__ == 'Pool')
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
                assert not node.batch_normalisation
                val[node] = self.act(node, y + b.view((1, -1) + (1,) * nd))
            elif kind == 'Perceptron':
                h = val[par].flatten(1) if node.flatten else val[par]
                assert not node.batch_normalisation
                val[node] = self.act(node, h @ self.p(node.w) + self.p(node.b))
            elif kind == 'Pool':
                h = val[par]
                if node.mode == 'max':
                    assert tuple(node.pool_stride) == tuple(node.pool_shape)
                    val[node] = (F.max_pool3d if h.dim() == 5 else F.max_pool2d)(h, tuple(node.pool_shape))
                else:
                    val[node] = pool_ref(h, node.pool_shape, node.pool_stride, node.mode)
            elif kind == 'Crop':
                val[node] = val[par][node._slicer()]
            elif kind == 'Concat':
                val[node] = torch.cat([val[q] for q in par], dim=1)
            elif kind == 'Add':
                val[node] = val[par[0]] + val[par[1]]
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
            if id(node) in pool_parents and val[node].requires_grad:
                val[node].retain_grad()
            if upto is not None and node is upto:
                return val[node]
        return (val.get(m.loss_node), val[m.prediction_node])

    def pool_parent_grads(self):
        """{Pool node: d loss / d (its parent's output)} of the last loss_and_grads"""
        return dict((n, self.val[n.parent].grad.numpy()) for n in self.model.nodes.values()
                    if type(n).__name__ == 'Pool')


# ---- the nets of tests/test_pool_modes_gpu.py (built without a GPU) --------------------------------
ADAM = dict(lr=5e-4, mom=0.9, beta2=0.999, wd=0.5e-4)


def _finish(nm, inp, logits):
    probs = nm.Softmax(logits)
    target = nm.Input_like(probs, override_f=1, name='target')
    loss = nm.AggregateLoss(nm.MultinoulliNLL(probs, target, target_is_sparse=True), name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=probs,
                          prediction_ext=[loss, probs])
    model.set_opt_meta_params('Adam', ADAM)
    return model


def net_chain(batch=2, seed=81, second=((1, 2, 2), (1, 1, 1), 'sum'), sp=(6, 22, 22)):
    """relu Conv -> Pool (2,2,2) 'average' -> tanh Conv -> Pool ``second`` -> lin Conv -> Softmax"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 1) + tuple(sp), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 4, (1, 3, 3))                                        # (6, 20, 20)
    out = nm.Pool(out, (2, 2, 2), mode='average', name='pool_a')            # (3, 10, 10)
    out = nm.Conv(out, 6, (1, 3, 3), activation_func='tanh')                # (3, 8, 8)
    out = nm.Pool(out, second[0], stride=second[1], mode=second[2], name='pool_b')
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin')
    return _finish(nm, inp, out)


def net_gaps(batch=2, seed=82):
    """the second Pool leaves gaps: (1,2,2) every (1,3,3), under the alias-free name"""
    return net_chain(batch, seed, second=((1, 2, 2), (1, 3, 3), 'average_exc_pad'))   # (3, 3, 3)


def net_skip(batch=2, seed=83):
    """an encoder Conv that feeds an average Pool AND the merge that brings the pooled branch back
    (its gradient has two writers); a 'same' Conv directly behind the Pool"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 1, 3, 22, 22), 'b,f,z,x,y', name='raw')
    c1 = nm.Conv(inp, 4, (1, 3, 3), name='enc')                             # (3, 20, 20)
    p1 = nm.Pool(c1, (1, 2, 2), mode='average', name='pool_a')              # (3, 10, 10)
    c2 = nm.Conv(p1, 6, (1, 3, 3), conv_mode='same', activation_func='tanh', name='same')
    c3 = nm.Conv(c2, 6, (1, 3, 3), name='low')                              # (3, 8, 8)
    mrg = nm.UpConvMerge(c1, c3, 4)                                         # (3, 16, 16)
    out = nm.Conv(mrg, 2, (1, 1, 1), activation_func='lin')
    return _finish(nm, inp, out)


def net_2d(batch=4, seed=84, tags='b,f,x,y'):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 1, 14, 14), tags, name='raw')
    out = nm.Conv(inp, 4, (3, 3))                                           # (12, 12)
    out = nm.Pool(out, (2, 2), mode='average', name='pool_a')               # (6, 6)
    out = nm.Conv(out, 6, (3, 3))                                           # (4, 4)
    out = nm.Pool(out, (2, 2), name='pool_b')                               # (2, 2), max
    out = nm.Perceptron(out, 10, 'lin', flatten=True)
    return _finish(nm, inp, out)


# name, constructor, classes, seed of the batch (chosen on the float64 reference alone: MIN_PRE of
# test_conv_modes_host.py holds over every evaluation the GPU tests make)
NETS = [("chain", net_chain, 2, 91), ("gaps", net_gaps, 2, 92), ("skip", net_skip, 2, 93),
        ("2d", net_2d, 10, 94)]


def batch_for(model, seed, n_class=2):
    rng = np.random.RandomState(seed)
    x = rng.rand(*model.input_node.shape.shape).astype(np.float32)
    t = rng.randint(0, n_class, model.target_node.shape.shape).astype(np.float32)
    if t.ndim == 5:
        t.flat[::17] = -1                          # unlabelled voxels
    return x, t


# ---- 1. the restatement against the NumPy loop -----------------------------------------------------
@pytest.mark.parametrize("mode", ['avg', 'sum'])
@pytest.mark.parametrize("win", WINDOWS, ids=WINDOW_IDS)
def test_restatement_equals_the_numpy_loop(win, mode):
    pool, stride = win
    rng = np.random.RandomState(7)
    done = 0
    for shape in INPUTS[:3] + [(1, 1, 3, 9, 11), (3, 7, 1, 1, 1)]:
        if any(p > i for p, i in zip(pool, shape[2:])):
            continue
        x = rng.randn(*shape)
        dout = rng.randn(*(shape[:2] + out_extent(shape[2:], pool, stride)))
        got_o, got_dx = pool_ref_fwd_bwd(x, dout, pool, stride, mode)
        want_o, want_dx, uncovered = numpy_loop(x, dout, pool, stride, mode)
        assert got_o.shape == want_o.shape, (shape, win)
        assert np.abs(got_o - want_o).max() < 1e-12
        assert np.abs(got_dx - want_dx).max() < 1e-12
        assert np.all(got_dx[:, :, uncovered] == 0)
        # what the windows of this pair leave out
        left_out = any((i - p) % s or (s > p and o > 1)
                       for i, p, s, o in zip(shape[2:], pool, stride, want_o.shape[2:]))
        assert bool(uncovered.any()) == left_out, (shape, win)
        done += 1
    assert done >= 1


# ---- 2. bookkeeping --------------------------------------------------------------------------------
def _nm():
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    return nm


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("win", WINDOWS, ids=WINDOW_IDS)
def test_shape_strides_fov_and_offsets(win, mode):
    """neural.py:1528-1559: extent (in - p + s - 1) // s + 1 where (in - p + s) % s == 0, fov grows
    by (p - 1) * the parent's stride, strides multiply by the pool STRIDE, offsets = fov // 2"""
    pool, stride = win
    nm = _nm()
    if mode == 'max' and pool != stride:
        inp = nm.Input((1, 2, 12, 12, 12), 'b,f,z,x,y', name='raw')
        with pytest.raises(NotImplementedError, match="Stride!=Pool"):
            nm.Pool(inp, pool, stride=stride, mode=mode)
        return
    # behind a pooled Conv: parent strides (1, 2, 2), fov (1, 4, 4)
    sp = tuple(p + 3 * s for p, s in zip(pool, stride))                     # three strides + a window
    inp = nm.Input((2, 1) + (sp[0], 2 * sp[1] + 2, 2 * sp[2] + 2), 'b,f,z,x,y', name='raw')
    par = nm.Conv(inp, 3, (1, 3, 3), (1, 2, 2))
    assert tuple(par.shape.spatial_shape) == sp
    pstr, pfov = (1, 2, 2), (1, 4, 4)
    assert tuple(int(v) for v in par.shape.strides) == pstr and tuple(par.shape.fov) == pfov
    node = nm.Pool(par, pool, stride=stride, mode=mode)
    assert node.mode == ('average_inc_pad' if mode == 'average' else mode)
    assert node.pool_shape == pool and node.pool_stride == stride
    assert tuple(node.shape.spatial_shape) == (4, 4, 4) == out_extent(sp, pool, stride)
    assert node.shape['f'] == 3 and node.shape['b'] == 2
    assert tuple(int(v) for v in node.shape.strides) == tuple(a * b for a, b in zip(pstr, stride))
    fov = tuple(f + (p - 1) * s for f, p, s in zip(pfov, pool, pstr))
    assert tuple(int(v) for v in node.shape.fov) == fov
    assert tuple(int(v) for v in node.shape.offsets) == tuple(f // 2 for f in fov)
    # stride None means the pool
    dflt = nm.Pool(par, pool, mode=mode, name='dflt') if all((i - p) % p == 0 for i, p in zip(sp, pool)) else None
    if dflt is not None:
        assert dflt.pool_stride == pool


def test_average_is_stored_as_average_inc_pad():
    nm = _nm()
    inp = nm.Input((1, 2, 4, 8, 8), 'b,f,z,x,y', name='raw')
    assert nm.Pool(inp, (1, 2, 2), mode='average').mode == 'average_inc_pad'
    assert nm.Pool(inp, (1, 2, 2), mode='average_exc_pad').mode == 'average_exc_pad'
    assert nm.Pool(inp, (1, 2, 2), mode='sum').mode == 'sum'
    assert nm.Pool(inp, (1, 2, 2)).mode == 'max'


@pytest.mark.parametrize("tags", ['b,f,x,y', 'b,f,y,x'])
@pytest.mark.parametrize("mode", ALL_MODES)
def test_2d_parents(tags, mode):
    nm = _nm()
    inp = nm.Input((3, 2, 12, 14), tags, name='raw')
    node = nm.Pool(inp, (3, 2), mode=mode)
    assert tuple(node.shape.spatial_shape) == (4, 7) and tuple(node.shape.tags) == tuple(tags.split(','))
    assert tuple(int(v) for v in node.shape.strides) == (3, 2)
    assert node.pool_shape == (3, 2) and node.pool_stride == (3, 2)
    if mode != 'max':
        over = nm.Pool(inp, (4, 2), stride=(2, 3), mode=mode, name='over')
        assert tuple(over.shape.spatial_shape) == (5, 5)
        assert tuple(int(v) for v in over.shape.strides) == (2, 3)
    else:
        with pytest.raises(NotImplementedError):
            nm.Pool(inp, (3, 2), stride=(2, 3))


def test_rejections():
    nm = _nm()
    inp = nm.Input((1, 2, 6, 12, 12), 'b,f,z,x,y', name='raw')
    with pytest.raises(ValueError) as e:
        nm.Pool(inp, (1, 2, 2), mode='median')
    for name in ALL_MODES:
        assert name in str(e.value)
    with pytest.raises(NotImplementedError):
        nm.Pool(inp, (1, 2, 2), stride=(1, 1, 1))                 # max with a stride of its own
    with pytest.raises(NotImplementedError):
        nm.Pool(inp, (1, 2, 2), stride=(1, 1, 1), mode='max')
    for mode in ALL_MODES:
        with pytest.raises(NotImplementedError):
            nm.Pool(inp, (1, 2, 2), mfp=True, mode=mode)
        with pytest.raises(NotImplementedError):
            nm.Pool(inp, (2, 2), mode=mode)                       # wrong tuple length
    with pytest.raises(ValueError):
        nm.Pool(inp, (1, 2, 2), stride=(2, 2), mode='sum')        # stride / pool lengths differ
    with pytest.raises(ValueError):
        nm.Pool(inp, (1, 2, 2), stride=(1, 0, 1), mode='sum')
    inp2 = nm.Input((1, 2, 12, 12), 'b,f,x,y', name='raw2')
    with pytest.raises(NotImplementedError):
        nm.Pool(inp2, (1, 2, 2), mode='average')
    inp1 = nm.Input((1, 2, 12), 'b,f,x', name='raw1')
    with pytest.raises(NotImplementedError):
        nm.Pool(inp1, (2,), mode='average')                       # 1-D parent
    with pytest.raises(ValueError, match="Cannot downsample"):
        nm.Pool(inp, (1, 2, 2), stride=(1, 3, 3), mode='average')  # (12 - 2) % 3
    with pytest.raises(ValueError, match="Cannot downsample"):
        nm.Pool(inp, (1, 5, 5), mode='sum')
    nm.Pool(inp, (1, 3, 3), stride=(1, 3, 3), mode='sum')


# ---- 3. save / modelload ---------------------------------------------------------------------------
def test_graph_descriptors_round_trip(tmp_path):
    nm = _nm()
    np.random.seed(5)
    m = net_chain()
    f = str(tmp_path / "pool.mdl")
    m.save(f)
    descr = json.loads(str(np.load(f, allow_pickle=False)["meta/graph"]))["nodes"]
    assert sum(1 for n in descr if n[1] == 'Pool') == 2

    def pools(model):
        return [(n.name, n.mode, n.pool_shape, n.pool_stride, tuple(n.shape.shape),
                 tuple(int(v) for v in n.shape.strides), tuple(int(v) for v in n.shape.fov))
                for n in model.nodes.values() if type(n).__name__ == 'Pool']
    want = pools(m)
    assert [w[1:4] for w in want] == [('average_inc_pad', (2, 2, 2), (2, 2, 2)),
                                      ('sum', (1, 2, 2), (1, 1, 1))]
    m2 = nm.modelload(f, name='again')
    assert pools(m2) == want
    for a, b in zip(m.trainable_params, m2.trainable_params):
        assert np.array_equal(a.get_value(), b.get_value())
    m3 = nm.modelload(f, name='batch5', imposed_batch_size=5)
    got = pools(m3)
    assert [g[:4] + g[5:] for g in got] == [w[:4] + w[5:] for w in want]
    assert [g[4] for g in got] == [(5,) + w[4][1:] for w in want]
    assert m3.input_node.shape['b'] == 5
    # a linear Pool has no max-fragment-pooling form: the rewrite names the node
    with pytest.raises(NotImplementedError, match="pool_a"):
        nm.modelload(f, name='mfp', override_mfp_to_active=True)


def test_new_symbols_are_exported():
    from elektronn2_amd import backend
    assert {'e2_pool3d_lin_fwd', 'e2_pool3d_lin_bwd'} <= set(backend.EXPORTED_SYMBOLS)
    assert backend.POOL_MODE == {'avg': 1, 'sum': 2}


# ---- 4. the reference side of the GPU tests on its own ---------------------------------------------
@pytest.mark.parametrize("name,make,ncls,data_seed", NETS, ids=[n[0] for n in NETS])
def test_restated_nets_run_on_the_cpu(name, make, ncls, data_seed):
    """every evaluation the GPU tests make (the first call and three Adam steps) passes MIN_PRE;
    every parameter and every Pool parent receives a gradient"""
    m = make()
    x, t = batch_for(m, data_seed, ncls)
    ref = PoolRef(m)
    for step in range(4):
        loss, probs = ref.loss_and_grads(x, t)            # asserts MIN_PRE
        assert np.isfinite(loss)
        assert all(np.abs(g).max() > 0 for g in ref.grads())
        for node, g in ref.pool_parent_grads().items():
            assert g.shape == tuple(node.parent.shape.shape) and np.abs(g).max() > 0
        ref.adam(**ADAM)
