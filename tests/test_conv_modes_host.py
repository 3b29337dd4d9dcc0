"""Conv border modes 'same' / 'full' and the Pad node, host side (no GPU): the float64 restatement
that tests/test_conv_modes_gpu.py compares every number against (``conv_ref`` and ``Ref``; never the
kernels), pinned here against scipy.signal.convolve; shape / stride / fov / cost bookkeeping of the
three modes (neural.py:725-778 of the reference) and of Pad (neural.py:1259-1279); every rejected
argument; the same-mode U-Net of nets.py; the save -> modelload round trip and the patch-size
solver."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_activations_host import act_torch, CANON, KINKED

MODES = ('valid', 'same', 'full')


# ---- the float64 restatement ---------------------------------------------------------------------
def frame_of(mode, filter_shape):
    """zero frame per axis: 0 ('valid'), f // 2 ('same'), f - 1 ('full')  (computations.py:287-291,
    320-326)"""
    if mode == 'valid':
        return tuple(0 for _ in filter_shape)
    return tuple((int(f) // 2 if mode == 'same' else int(f) - 1) for f in filter_shape)


def conv_ref(x, w, mode):
    """true convolution (filters flipped) of the zero-framed input, float64 torch-CPU;
    x (n, ci, *sp), w (co, ci, *k), 2 or 3 spatial axes"""
    nd = x.dim() - 2
    q = frame_of(mode, w.shape[2:])
    pad = []
    for v in reversed(q):              # F.pad takes the LAST axis first
        pad += [v, v]
    xp = F.pad(x, pad)
    return (F.conv3d if nd == 3 else F.conv2d)(xp, w.flip(*range(2, 2 + nd)))


MIN_PRE = 1e-6     # (tests/test_activations_gpu.py: a kinked unit this close to zero is ill-posed)


class Ref(object):
    """float64 torch-CPU restatement of a model's graph: conv (any border mode) -> pool -> (batch
    norm) + bias -> activation per Conv node, UpConv, Pool, Crop, Pad, Concat, Add, Softmax,
    MultinoulliNLL (sparse targets), AggregateLoss; autograd differentiates it; ``adam`` restates
    optimiser.py:273-334."""

    def __init__(self, model):
        self.model = model
        self.t = 0
        self.min_pre = np.inf
        self.P, self.m, self.s = {}, {}, {}
        for node in model.nodes.values():
            for p in node.params.values():
                if id(p) not in self.P:
                    self.P[id(p)] = torch.tensor(p.get_value().astype(np.float64),
                                                 requires_grad=bool(p.apply_train))

    def p(self, param):
        return self.P[id(param)]

    def act(self, node, v):
        if CANON[node.activation_func] in KINKED:
            self.min_pre = min(self.min_pre, float(v.detach().abs().min()))
        return act_torch(node.activation_func, v)

    @staticmethod
    def bn(y, g, b, red):
        bsh = [1] * y.dim()
        bsh[1] = -1
        mean = y.mean(dim=red)
        std = torch.sqrt(((y - mean.view(bsh)) ** 2).mean(dim=red)) + 1e-6
        return (g / std).view(bsh) * y + (b - g * mean / std).view(bsh)

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
                if t is None:
                    continue
                val[node] = torch.tensor(np.asarray(t, np.float64))
            elif kind in ('Conv', 'UpConv'):
                h, w, b = val[par], self.p(node.w), self.p(node.b)
                nd = h.dim() - 2
                bsh = (1, -1) + (1,) * nd
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
                    y = y + b.view(bsh)
                val[node] = self.act(node, y)
            elif kind == 'Pool':
                val[node] = F.max_pool3d(val[par], tuple(node.pool_shape))
            elif kind == 'Crop':
                val[node] = val[par][node._slicer()]
            elif kind == 'Pad':
                pz, px, py = node.pad
                val[node] = F.pad(val[par], [py, py, px, px, pz, pz], value=float(node.value))
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
            if upto is not None and node is upto:
                return val[node]
        return (val.get(m.loss_node), val[m.prediction_node])

    def loss_and_grads(self, x, t):
        for v in self.P.values():
            v.grad = None
        loss, probs = self.forward(x, t)
        assert self.min_pre >= MIN_PRE, "ill-posed case: a kinked unit at %.1e" % (self.min_pre,)
        loss.backward()
        return float(loss.detach()), probs.detach().numpy()

    def predict(self, x):
        with torch.no_grad():
            return self.forward(x)[1].numpy()

    def grads(self):
        """in the order of Model.gradients"""
        return [self.p(p).grad.numpy() for p in self.model.trainable_params]

    @torch.no_grad()
    def adam(self, lr, mom, beta2, wd):
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


# ---- 1. the restatement against scipy --------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_restatement_equals_scipy_convolve(mode):
    from scipy.signal import convolve
    rng = np.random.RandomState(5)
    worst = 0.0
    for sp, k in (((4, 9, 10), (3, 3, 3)), ((3, 8, 9), (1, 5, 5)), ((5, 7, 6), (3, 1, 1)),
                  ((4, 8, 9), (2, 4, 4)), ((9, 11), (3, 3)), ((8, 9), (5, 3))):
        if mode == 'same' and any(f % 2 == 0 for f in k):
            continue
        x = rng.randn(2, 3, *sp)
        w = rng.randn(4, 3, *k)
        got = conv_ref(torch.tensor(x), torch.tensor(w), mode).numpy()
        for n in range(2):
            for co in range(4):
                want = sum(convolve(x[n, ci], w[co, ci], mode=mode) for ci in range(3))
                assert got[n, co].shape == want.shape, (mode, sp, k)
                worst = max(worst, float(np.abs(got[n, co] - want).max()))
    print("conv_ref vs scipy.signal.convolve, mode %s: largest difference %.2e" % (mode, worst))
    assert worst < 1e-12


# ---- 2. bookkeeping and rejections -----------------------------------------------------------------
def _nm():
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    return nm


def _border(mode, f):
    return {'valid': 1 - f, 'same': 0, 'full': f - 1}[mode]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dims", [3, 2])
def test_shapes_strides_fov_and_cost(mode, dims):
    nm = _nm()
    if dims == 3:
        sp, k, p, tags = (9, 22, 25), (3, 3, 5), (1, 2, 1), 'b,f,z,x,y'
        if mode == 'full':
            sp = (9, 20, 25)              # (20 + 2) % 2 == 0
    else:
        sp, k, p, tags = (20, 21), (3, 5), (2, 1), 'b,f,y,x'
    inp = nm.Input((2, 3) + sp, tags, name='raw')
    c = nm.Conv(inp, 5, k, p, conv_mode=mode)
    want = tuple((s + _border(mode, f)) // q for s, f, q in zip(sp, k, p))
    assert tuple(c.shape.spatial_shape) == want
    assert c.shape['f'] == 5 and c.shape['b'] == 2
    assert tuple(int(v) for v in c.shape.strides) == tuple(p)
    assert tuple(int(v) for v in c.shape.fov) == tuple(1 + (f + q - 2) for f, q in zip(k, p))
    npos = int(np.prod([s + (1 - f if mode == 'valid' else f - 1) for s, f in zip(sp, k)]))
    assert c.computational_cost == 5 * 3 * int(np.prod(k)) * npos * 2
    # a second layer: fov grows by (f + p - 2) * stride whatever the mode
    c2 = nm.Conv(c, 4, tuple(3 for _ in k), conv_mode='same')
    assert tuple(c2.shape.spatial_shape) == want
    assert tuple(int(v) for v in c2.shape.fov) == tuple(1 + (f + q - 2) + 2 * q for f, q in zip(k, p))
    c3 = nm.Conv(c, 4, tuple(3 for _ in k), conv_mode='same', invalidate_fov=True)
    assert tuple(int(v) for v in c3.shape.fov) == tuple(-1 for _ in k)


def test_rejected_arguments():
    nm = _nm()
    inp = nm.Input((1, 2, 6, 12, 12), 'b,f,z,x,y', name='raw')
    with pytest.raises(ValueError, match="Cannot pool spatial axis"):
        nm.Conv(inp, 4, (1, 3, 3), (1, 1, 5), conv_mode='same')
    with pytest.raises(ValueError, match="Cannot pool spatial axis"):
        nm.Conv(inp, 4, (1, 3, 3), (1, 1, 4), conv_mode='full')           # 14 % 4
    with pytest.raises(ValueError, match='For "same"-mode convolution, filter shapes must be odd'):
        nm.Conv(inp, 4, (2, 3, 3), conv_mode='same')
    with pytest.raises(ValueError, match="conv_mode"):
        nm.Conv(inp, 4, (1, 3, 3), conv_mode='reflect')
    with pytest.raises(NotImplementedError, match="same"):
        nm.Conv(inp, 4, (1, 3, 3), (1, 2, 2), conv_mode='same', mfp=True)
    with pytest.raises(NotImplementedError, match="full"):
        nm.Conv(inp, 4, (1, 3, 3), (1, 2, 2), conv_mode='full', mfp=True)
    # behind a max-fragment-pooling layer (fragments on the batch axis) a frame is not the border
    inp1 = nm.Input((1, 1, 6, 14, 14), 'b,f,z,x,y', name='raw_mfp')
    frag = nm.Conv(inp1, 4, (1, 2, 2), (1, 2, 2), mfp=True)
    with pytest.raises(NotImplementedError, match="max-fragment"):
        nm.Conv(frag, 4, (1, 3, 3), conv_mode='same')
    nm.Conv(frag, 4, (1, 1, 1), conv_mode='same')                         # (the valid conv)
    # all filter extents 1: any mode is the valid conv, internally too
    c = nm.Conv(inp, 4, (1, 1, 1), conv_mode='full')
    assert c._valid_mode() and tuple(c._q3) == (0, 0, 0)
    assert tuple(c.shape.spatial_shape) == (6, 12, 12)
    c = nm.Conv(inp, 4, (1, 3, 3), conv_mode='same')
    assert not c._valid_mode() and tuple(c._q3) == (0, 1, 1)
    c = nm.Conv(inp, 4, (2, 4, 4), conv_mode='full')
    assert tuple(c._q3) == (1, 3, 3) and tuple(c.shape.spatial_shape) == (7, 15, 15)
    # UpConv stays 'valid' (neural.py:969-970)
    u = nm.UpConv(inp, 4, (1, 2, 2))
    assert u.conv_mode == 'valid' and u._valid_mode()


def test_pad_node_bookkeeping_and_rejections():
    nm = _nm()
    inp = nm.Input((1, 2, 6, 12, 13), 'b,f,z,x,y', name='raw')
    c = nm.Conv(inp, 4, (1, 3, 3), (1, 2, 1))
    pd = nm.Pad(c, (1, 0, 2), value=1.5)
    assert tuple(pd.shape.spatial_shape) == (8, 5, 15)
    assert pd.shape['f'] == 4
    assert tuple(int(v) for v in pd.shape.strides) == tuple(int(v) for v in c.shape.strides)
    assert tuple(int(v) for v in pd.shape.fov) == tuple(int(v) for v in c.shape.fov)
    assert pd.computational_cost == 0
    assert pd.value == 1.5 and tuple(pd.pad) == (1, 0, 2)
    assert nm.Pad is not None and 'Pad' in dir(nm)
    for bad in ((1, 2), (1, -1, 0), (1, 1.5, 1), 3, (1, 1, 1, 1), ('a', 1, 1)):
        with pytest.raises(ValueError):
            nm.Pad(c, bad)
    inp2 = nm.Input((1, 1, 12, 12), 'b,f,y,x', name='raw2d')
    with pytest.raises(NotImplementedError, match='only implemented for "b,f,z,x,y"'):
        nm.Pad(inp2, (1, 1, 1))


# ---- 3. the same-mode U-Net ------------------------------------------------------------------------
def test_unet3d_lite_same_maps_a_patch_to_a_prediction_of_its_size():
    from elektronn2_amd import nets, neuromancer as nm
    nm.model_manager.reset()
    m = nets.unet3d_lite((None, 1, 22, 136, 136), conv_mode='same')
    assert tuple(m.prediction_node.shape.spatial_shape) == (22, 136, 136)
    assert tuple(int(v) for v in m.prediction_node.shape.strides) == (1, 1, 1)
    assert tuple(m.target_node.shape.spatial_shape) == (22, 136, 136)
    assert tuple(int(v) for v in m.prediction_node.shape.fov) == (0, 0, 0)
    assert tuple(int(v) for v in m.prediction_node.shape.offsets) == (0, 0, 0)
    assert not any(type(n).__name__ == 'Crop' for n in m.nodes.values())
    assert all(n.conv_mode == 'same' for n in m.nodes.values() if type(n).__name__ == 'Conv')
    # the defaults are untouched
    nm.model_manager.reset()
    m = nets.unet3d_lite((None, 1, 22, 140, 140))
    assert all(n.conv_mode == 'valid' for n in m.nodes.values() if type(n).__name__ == 'Conv')
    assert tuple(m.prediction_node.shape.spatial_shape) != (22, 140, 140)
    nm.model_manager.reset()
    m = nets.unet3d((None, 1, 24, 24, 24), conv_mode='same')
    assert tuple(m.prediction_node.shape.spatial_shape) == (24, 24, 24)


# ---- 4. save / modelload ---------------------------------------------------------------------------
def _same_pad_net(nm, sp=(6, 18, 18)):
    inp = nm.Input((1, 1) + sp, 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 4, (1, 3, 3), (1, 2, 2), conv_mode='same')
    out = nm.Pad(out, (0, 1, 1), value=0.25)
    out = nm.Conv(out, 6, (1, 3, 3))
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin', conv_mode='same')
    probs = nm.Softmax(out)
    target = nm.Input_like(probs, override_f=1, name='target')
    loss = nm.AggregateLoss(nm.MultinoulliNLL(probs, target, target_is_sparse=True), name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=probs)
    return model


def test_graph_descriptors_round_trip_and_the_solver_takes_same_convs(tmp_path):
    nm = _nm()
    m = _same_pad_net(nm)
    assert tuple(m.prediction_node.shape.spatial_shape) == (6, 9, 9)
    f = str(tmp_path / "same.mdl")
    m.save(f)
    m2 = nm.modelload(f, name='again')
    kinds = [(type(n).__name__, getattr(n, 'conv_mode', None)) for n in m2.nodes.values()]
    assert kinds == [(type(n).__name__, getattr(n, 'conv_mode', None)) for n in m.nodes.values()]
    pads = [n for n in m2.nodes.values() if type(n).__name__ == 'Pad']
    assert len(pads) == 1 and tuple(pads[0].pad) == (0, 1, 1) and pads[0].value == 0.25
    assert tuple(m2.prediction_node.shape.spatial_shape) == (6, 9, 9)
    for a, b in zip(m.trainable_params, m2.trainable_params):
        assert np.array_equal(a.get_value(), b.get_value())
    # the solver: 'same' (1,3,3) pool (1,2,2) -> needs even x / y; Pad grows by 2; valid 3x3 shrinks
    from elektronn2_amd.neuromancer import model as model_mod
    z = np.load(f, allow_pickle=False)
    import json
    nodes = json.loads(str(z["meta/graph"]))["nodes"]
    filters, pools, mfps = model_mod.kernel_lists_from_node_descr(nodes)
    assert filters == [(1, 1, 1), (1, -1, -1), (1, 3, 3), (1, 1, 1)]
    assert pools == [(1, 2, 2), (1, 1, 1), (1, 1, 1), (1, 1, 1)]
    m3 = nm.modelload(f, name='imposed', imposed_patch_size=(5, 27, 31))
    assert tuple(m3.input_node.shape.spatial_shape) == (5, 26, 30)
    assert tuple(m3.prediction_node.shape.spatial_shape) == (5, 13, 15)
    # a 'full' conv: effective extent 2 - f (or NotImplementedError); here the solver takes it
    nm.model_manager.reset()
    inp = nm.Input((1, 1, 4, 10, 10), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 3, (1, 3, 3), (1, 2, 2), conv_mode='full')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, prediction_node=out)
    f2 = str(tmp_path / "full.mdl")
    model.save(f2)
    m4 = nm.modelload(f2, name='full_imposed', imposed_patch_size=(4, 13, 9))
    assert tuple(m4.input_node.shape.spatial_shape) == (4, 12, 8)
    assert tuple(m4.prediction_node.shape.spatial_shape) == (4, 7, 5)


def test_prediction_time_rewrites_are_rejected_without_a_gpu(tmp_path):
    nm = _nm()
    m = _same_pad_net(nm)
    with pytest.raises(NotImplementedError, match="same"):
        m.predict_dense(np.zeros((1, 6, 30, 30), np.float32))
    f = str(tmp_path / "same.mdl")
    m.save(f)
    with pytest.raises(NotImplementedError, match="same"):
        nm.modelload(f, name='mfp', override_mfp_to_active=True)
    nm.model_manager.reset()
    inp = nm.Input((1, 1, 6, 18, 18), 'b,f,z,x,y', name='raw')
    out = nm.Conv(nm.Pad(inp, (0, 1, 1)), 2, (1, 3, 3))
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, prediction_node=out)
    with pytest.raises(NotImplementedError, match="Pad"):
        model.predict_dense(np.zeros((1, 6, 30, 30), np.float32))


def test_restated_graph_runs_on_the_cpu():
    """the reference side of the GPU tests on its own: a same-mode net with a Pad and batch size 2"""
    nm = _nm()
    np.random.seed(3)
    m = _same_pad_net(nm)
    rng = np.random.RandomState(4)
    x = rng.rand(1, 1, 6, 18, 18).astype(np.float32)
    t = rng.randint(0, 2, (1, 1, 6, 9, 9)).astype(np.float32)
    ref = Ref(m)
    loss, probs = ref.loss_and_grads(x, t)
    assert np.isfinite(loss) and probs.shape == (1, 2, 6, 9, 9)
    assert all(np.abs(g).max() > 0 for g in ref.grads())
