"""SobelizedLoss on the GPU (csrc/loss_sobel.hip; loss.py:1373-1439) against tests/test_sobel_loss_host.py's
float64 DENSE convolution + ABS row + autograd on the float32 inputs the kernels saw, at the project's own bounds.
CONDITION on the op tests' inputs, asserted on the reference: every d = S t - S p is 0 exactly or >= 1e-3 away from 0 and the margin."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from elektronn2_amd import backend
from test_activations_gpu import ADAM
from test_loss_nodes_gpu import Watched
from test_regression_loss_gpu import RefL, TOL, TOL_LOSS, TOL_STEP, rel, dev, t64, close, _done, _trunk
from test_regression_loss_host import ref_squared, ref_aggregate, is_masked
from test_sobel_loss_host import ref_sobel

pytestmark, f32 = pytest.mark.gpu, np.float32
# tile 4 x 8 x 32 (1 x 8 x 32 for dim 2): extents below the halo reach, a unit axis, batch / features > 1; 2-D calls;
# one more than the tile on every axis (every seam); 1080 tiles > the cap of 1024 work-groups (grid-stride path)
SHAPES = [((1, 1, 1, 1, 1), 3), ((1, 1, 2, 2, 2), 3), ((2, 3, 3, 1, 2), 3), ((1, 2, 1, 5, 7), 2),
          ((1, 2, 5, 9, 33), 3), ((1, 2, 1, 9, 33), 2), ((2, 3, 9, 73, 161), 3)]
MARGIN = {3: float(f32(0.1)), 2: float(f32(0.25))}    # |d| in {0} + {.09, .12, .16 (dim 2: .3, .4)} x {.5, 1, 2}
SC, WGT = float(f32(0.7)), 0.7
_REF = {}


def inputs(shape, dim, seed):
    """t random; p = t but for spikes THREE apart on every filtered axis: no d sees two, most see none (equal data)"""
    rng = np.random.RandomState(seed)
    t = (rng.randn(*shape) * 1.5).astype(f32)
    e = np.zeros(shape, f32)
    for n in range(shape[0]):
        for f in range(shape[1]):
            oz, oy, ox = rng.randint(0, 3, 3) % np.minimum(shape[2:], 3)      # (a spike also in a short axis)
            sub = e[n, f, oz::3, oy::3, ox::3] if dim == 3 else e[n, f, :, oy::3, ox::3]
            sub[...] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], sub.shape)
    return (t - e).astype(f32), t


def case(shape, dim, opt):
    """(p, t, L, n_lab, d(WGT L)/dp, a start for the accumulating backward), made once"""
    if (shape, opt) not in _REF:
        p, t = inputs(shape, dim, 500 + int(np.dot(shape, [1, 7, 49, 343, 2401])))
        m = MARGIN[dim] if 'm' in opt else None
        tp = t64(p, True)
        out, d, ts = ref_sobel(tp, t64(t), dim, m, SC if 's' in opt else None)
        nz = d[d != 0].abs()
        assert nz.numel() == 0 or nz.min() >= 1e-3
        assert m is None or nz.numel() == 0 or (nz - m).abs().min() >= 1e-3
        L = out.mean()
        g = torch.autograd.grad(WGT * L, [tp])[0].numpy()
        g0 = (np.random.RandomState(7).randn(*shape) * (np.abs(g).max() or 1.0)).astype(f32)
        _REF[shape, opt] = (p, t, float(L.detach()), int((~is_masked(ts)).sum()), g, g0)
    return _REF[shape, opt]


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("opt", ["", "m", "s", "ms"])
@pytest.mark.parametrize("shape,dim", SHAPES, ids=["x".join(map(str, s)) for s, _ in SHAPES])
def test_fwd_mix_bwd_through_the_c_abi(ctx, shape, dim, opt, acc):
    p, t, L, n_lab, g, g0 = case(shape, dim, opt)
    term = backend.loss_term('abs', margin=dev([MARGIN[dim]]) if 'm' in opt else None,
                             scale_correction=dev([SC]) if 's' in opt else None)
    w = Watched("mixed")
    pv, tv = w.place(shape, p, read_only=True), w.place(shape, t, read_only=True)
    rows = ctx.sobel_partials(pv)
    slab = torch.full((4 * rows + 8,), float('nan'), device='cuda')
    ctx.sobel_abs_fwd(term, dim, pv, tv, slab[:4 * rows])
    assert torch.isnan(slab[4 * rows:]).all() and not torch.isnan(slab[:4 * rows]).any()
    coef, tl, cnt = (torch.full((8,), -3.0, device='cuda') for _ in range(3))
    out = torch.full((1,), -3.0, device='cuda')
    ctx.loss_mix([term], [slab[:4 * rows]], [dim * p.size], dev([WGT]), coef, tl, cnt, out)
    assert close(tl[0].item(), L, TOL_LOSS) and close(out.item(), WGT * L, TOL_LOSS), (tl[0].item(), L)
    assert cnt[0].item() == n_lab == dim * p.size
    dv = w.place(shape, g0)
    ctx.sobel_abs_bwd(term, dim, pv, tv, coef[0:1], dv, accumulate=acc)
    got, base = dv.cpu().numpy(), (g0 if acc else np.zeros_like(g0))
    assert np.all(np.isfinite(got)) and rel(got, base.astype(np.float64) + g) < TOL
    w.check()


# ---- nodes --------------------------------------------------------------------------------------------------
class RefS(RefL):
    """RefL with 2-D Convs and the Sobel term; ``margin_gap``: the least distance of its |d| from 0 and the margin"""

    def forward(self, feed, seed=0, counter=0):
        m = self.model
        self.min_pre, self.n_kinked, self.max_sig_pre, self.margin_gap, self.terms = np.inf, 0, 0.0, np.inf, {}
        val = {}
        for node in m.nodes.values():
            kind, par = type(node).__name__, node.parent
            if kind == 'Input':
                val[node] = t64(feed[node.name])
            elif kind == 'Conv':
                w, b = self.p(node.w), self.p(node.b)
                nd = w.dim() - 2
                y = (F.conv3d if nd == 3 else F.conv2d)(val[par], w.flip(*range(2, 2 + nd)))
                val[node] = self.act(node, y + b.view((1, -1) + (1,) * nd))
            elif kind == 'SquaredLoss':
                val[node] = ref_squared(val[par[0]], val[par[1]])
            elif kind == 'SobelAbsLoss':
                mg = float(f32(node.margin.get_value()))
                lift = (lambda a: a) if node.dim == 3 else (lambda a: a[:, :, None])
                val[node], d, ts = ref_sobel(lift(val[par[0]]), lift(val[par[1]]), node.dim, mg)
                self.margin_gap = float(torch.minimum(d.abs(), (d.abs() - mg).abs()).min())
                self.terms[node.name] = (float(val[node].detach().mean()), int((~is_masked(ts)).sum()))
            elif kind == 'AggregateLoss':
                val[node] = ref_aggregate([val[q] for q in par], node.mixing_weights.get_value().astype(np.float64))
        return val[m.loss_node], val[m.prediction_node]


def net(dims, seed=91, margin=0.05):
    from elektronn2_amd import neuromancer as nm
    if dims == 3:
        inp, out = _trunk(nm, 1, seed)
    else:
        nm.model_manager.reset()
        np.random.seed(seed)
        inp = nm.Input((2, 1, 18, 18), 'b,f,x,y', name='raw')
        out = nm.Conv(nm.Conv(inp, 6, (3, 3)), 8, (3, 3), activation_func='tanh')
    head = nm.Conv(out, 2, (1,) * dims, activation_func='lin', name='head')
    t = nm.Input_like(head, name='target')
    sob = nm.SobelizedLoss(head, t, loss_kwargs=dict(margin=margin, name='sobel'))
    loss = nm.AggregateLoss([nm.SquaredLoss(head, t), sob], mixing_weights=[1.0, 0.5], name='loss')
    return _done(nm, inp, loss, head)


@pytest.mark.parametrize("dims", [3, 2])
def test_step_against_float64_and_replay(dims, tmp_path):
    """loss, term, every gradient, Adam; a new margin reaches the captured step; save / modelload"""
    from elektronn2_amd.neuromancer.model import modelload
    m = net(dims)
    rng = np.random.RandomState(83)
    args = [rng.rand(*m.nodes['raw'].shape.shape).astype(f32), rng.randn(*m.nodes['target'].shape.shape).astype(f32)]
    feed = dict(raw=args[0], target=args[1])
    for call, mg in enumerate((0.05, 0.05, 0.05, 0.4)):      # eager, capture, replay, replay with a new margin
        m.nodes['sobel'].params['margin'].set_value(f32(mg))
        ref = RefS(m)
        lref, _ = ref.loss_and_grads(feed)
        assert close(float(m.loss(*args)), lref, TOL_STEP)
        for nme, g, w in zip(m.loss_node.all_trainable_params.keys(), m.gradients(*args), ref.grads()):
            assert np.abs(w).max() > 0 and rel(g, w) < TOL_STEP, (mg, nme, rel(g, w))
        (L, n_lab), sob = ref.terms['sobel'], m.nodes['sobel']
        assert close(sob.term_value, L, TOL_LOSS) and sob.n_labelled == n_lab == dims * args[1].size
        if call >= 2:
            graphs = [list(fn.func._graphs) for fn in (m._grad_func, m.loss_node._output_func)]
            assert all(graphs) and (call == 2 or graphs == plans)          # no new capture
            plans = graphs
    f = str(tmp_path / "sobel.mdl")
    m.save(f)
    ref.loss_and_grads(feed)
    ref.adam(**ADAM)
    m.trainingstep(*args, optimiser='Adam')
    for nme, p in m.loss_node.all_trainable_params.items():
        assert rel(p.get_value(), ref.p(p).detach().numpy()) < TOL_STEP, nme
    c = modelload(f)
    assert type(c.nodes['sobel']).__name__ == 'SobelAbsLoss' and float(c.nodes['sobel'].margin.get_value()) == f32(0.4)
    assert close(float(c.loss(*args)), lref, TOL_STEP)


def test_a_trainable_target_is_refused():
    from elektronn2_amd import neuromancer as nm
    inp, out = _trunk(nm, 1, 92)
    a, b = (nm.Conv(out, 2, (1, 1, 1), activation_func='lin', name=k) for k in 'ab')
    loss = nm.AggregateLoss(nm.SobelizedLoss(a, b, loss_kwargs=dict(name='sobel')), name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=None, loss_node=loss, prediction_node=a)
    with pytest.raises(NotImplementedError, match="sobel"):
        model.gradients(np.random.RandomState(1).rand(1, 1, 5, 18, 18).astype(f32))
