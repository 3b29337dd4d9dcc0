"""GaussianRV and its AEVB prior on the GPU (csrc/gauss_rv.hip, various.py:32-151).

The reference of every comparison is the float64 restatement of tests/test_gauss_rv_host.py and
float64 torch-CPU autograd of the nets with eps taken from it -- never the kernels.  Bounds: the
device noise at NOISE_TOL (four times the largest error measured over the 2^20
elements of the statistics case; a wrong word pairing, counter or stream gives errors of order 1);
ops at the project's op bound 2e-5 (tests/test_ops_gpu.py:16); loss and gradients of a step at the
whole-step bound 1e-4 (tests/test_model_gpu.py:17), in bf16 mode at tests/shared_param_cases.py's."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from shared_param_cases import BF16_LOSS, BF16_GRAD
from test_conv_modes_host import Ref, conv_ref
from test_dropout_gpu import dev, rel, state_tensor
from test_gauss_rv_host import restated_normals, restated, STAT, STAT_N

pytestmark = pytest.mark.gpu
NOISE_TOL = 4 * 5.785e-7    # measured: 5.785e-7 (printed by the statistics test below)
TOL, TOL_STEP = 2e-5, 1e-4
SEED, COUNTER, STREAM = (9 << 32) + 77, 41, 6
LR = 0.05                   # SGD without momentum or decay: p' = p - LR g
SHAPES = [(1, 1, 1, 1, 1), (2, 3, 1, 1, 7), (1, 2, 3, 5, 9), (1, 4, 2, 8, 16)]


# ---- layouts: k views of one logical shape inside NaN-filled storage -> [(storage, view)] ----------
def _dense(shape, k):
    return [(t, t) for t in (torch.full(shape, np.nan, device='cuda') for _ in range(k))]


def _halves(shape, k):
    """consecutive pairs are the two channel halves of one (n, 2F, ...) buffer (here with one more
    channel either side of them)"""
    n, c = shape[:2]
    ts = [torch.full((n, 2 * c + 2) + shape[2:], np.nan, device='cuda') for _ in range((k + 1) // 2)]
    return [(ts[i // 2], ts[i // 2][:, 1 + (i % 2) * c:1 + (i % 2 + 1) * c]) for i in range(k)]


def _misaligned(shape, k):
    """a dense view whose base lies one element behind a 16-byte boundary"""
    ts = [torch.full((int(np.prod(shape)) + 8,), np.nan, device='cuda') for _ in range(k)]
    return [(t, t[1:1 + int(np.prod(shape))].view(shape)) for t in ts]


def _around(views):
    """per storage, the bits outside every view that lies in it (NaN-safe)"""
    marks = {}
    for store, v in views:
        mark = marks.setdefault(id(store), (store, torch.zeros_like(store, dtype=torch.bool)))[1]
        mark.as_strided(v.shape, v.stride(), v.storage_offset()).fill_(True)
    return [store.view(torch.int32)[~mark].clone() for store, mark in marks.values()]


@pytest.mark.parametrize("layout", [_dense, _halves, _misaligned], ids=lambda f: f.__name__[1:])
def test_ops_through_the_c_abi(ctx, layout):
    rng = np.random.RandomState(3)
    st, coef = state_tensor(SEED, COUNTER), dev([0.37])
    for shape in SHAPES:
        eps = restated_normals(int(np.prod(shape)), SEED, COUNTER, STREAM).reshape(shape)
        mu, ls, g, pm, ps = ((rng.randn(*shape) * 0.7).astype(np.float32).astype(np.float64) for _ in range(5))
        want = restated(mu, ls, eps, g, 0.37)
        views = layout(shape, 6)
        vm, vl, vo, vg, dm, dl = (v for _, v in views)
        vm.zero_(); vl.zero_()                                      # the noise itself
        ctx.gaussrv_fwd(vm, vl, vo, st, STREAM)
        assert np.abs(vo.cpu().numpy() - eps).max() < NOISE_TOL, shape
        vm.copy_(dev(mu)); vl.copy_(dev(ls)); vg.copy_(dev(g))
        before = _around(views)
        ctx.gaussrv_fwd(vm, vl, vo, st, STREAM)
        assert rel(vo.cpu().numpy(), want['z']) < TOL, shape
        dense = torch.empty(shape, device='cuda')
        ctx.gaussrv_fwd(dev(mu), dev(ls), dense, st, STREAM)
        assert torch.equal(dense, vo), shape                        # j is logical: bit-equal
        # backward: each accumulate value on prefilled gradients, each gradient view NULL in turn
        for am, al in ((False, False), (True, False), (False, True), (True, True)):
            for bwd, ref in ((lambda a, b: ctx.gaussrv_bwd(vg, vl, a, b, st, STREAM, acc_mu=am, acc_sig=al), want['rv_bwd']),
                             (lambda a, b: ctx.aevb_prior_bwd(vm, vl, coef, a, b, acc_mu=am, acc_sig=al), want['prior_bwd'])):
                dm.copy_(dev(pm)); dl.copy_(dev(ps))
                bwd(dm, dl)
                both = dm.clone(), dl.clone()
                assert rel(both[0].cpu().numpy(), ref[0] + am * pm) < TOL, (shape, am, al)
                assert rel(both[1].cpu().numpy(), ref[1] + al * ps) < TOL, (shape, am, al)
                dm.copy_(dev(pm)); dl.copy_(dev(ps))
                bwd(dm, None)
                bwd(None, dl)
                assert torch.equal(dm, both[0]) and torch.equal(dl, both[1]), (shape, am, al)
        # the prior's slab: total against the restatement, two runs bit-equal
        slabs = [torch.full((ctx.loss_partials(vm), 4), np.nan, device='cuda') for _ in range(2)]
        for s in slabs:
            ctx.aevb_prior_fwd(vm, vl, s.view(-1))
        tot = slabs[0].double().sum(0).cpu().numpy()
        assert torch.equal(slabs[0], slabs[1]) and tuple(tot[1:]) == (np.prod(shape), 0, 0)
        assert abs(tot[0] - want['prior'].sum()) < TOL * max(want['prior'].sum(), 1.0), shape
        for now, b in zip(_around(views), before):
            assert torch.equal(now, b), shape                       # no bit changed around the views


def test_noise_statistics_and_tolerance_at_2_to_the_20(ctx):
    z = torch.zeros((1, 1, 1, 1024, STAT_N // 1024), device='cuda')
    out = torch.empty_like(z)
    ctx.gaussrv_fwd(z, z.clone(), out, state_tensor(STAT['seed'], STAT['counter']), STAT['stream'])
    got = out.cpu().numpy().astype(np.float64).reshape(-1)
    err = np.abs(got - restated_normals(STAT_N, **STAT)).max()
    print("largest |eps_dev - eps_64| over 2^20 elements: %.3e" % err)
    assert NOISE_TOL <= 1e-4 and err < NOISE_TOL
    assert abs(got.mean()) < 5.0 / np.sqrt(STAT_N) and abs(got.var() - 1.0) < 5.0 * np.sqrt(2.0 / STAT_N)


def test_refusals(ctx):
    from elektronn2_amd import backend
    a, b, c = (torch.zeros((1, 2, 1, 3, 4), device='cuda') for _ in range(3))
    small, st, coef = torch.zeros((1, 2, 1, 3, 3), device='cuda'), state_tensor(1, 1), dev([1.0])
    slab = torch.zeros(4 * ctx.loss_partials(a), device='cuda')
    for call, msg in ((lambda: ctx.gaussrv_fwd(a, small, c, st, 0), "different sizes"),
                      (lambda: ctx.gaussrv_bwd(a, b, small, None, st, 0), "different sizes"),
                      (lambda: ctx.aevb_prior_fwd(a, small, slab), "different sizes"),
                      (lambda: ctx.aevb_prior_bwd(a, b, coef, None, small), "different sizes"),
                      (lambda: ctx.gaussrv_fwd(a, b, c, None, 0), "null state"),
                      (lambda: ctx.gaussrv_bwd(a, b, c, None, None, 0), "null state"),
                      (lambda: ctx.gaussrv_bwd(a, b, None, None, st, 0), "no gradient view"),
                      (lambda: ctx.aevb_prior_bwd(a, b, coef, None, None), "no gradient view"),
                      (lambda: ctx.gaussrv_fwd(a, b, a, st, 0), "alias")):
        with pytest.raises(backend.E2Error, match=msg):
            call()
    # a channel of 2^31 elements: descriptors only, refused on the host before anything is launched
    huge = [C.byref(backend.Tensor5(t.data_ptr(), 1, 1, 2048, 1024, 1024, 0, 0, 0, 0)) for t in (a, b, c)]
    assert backend.lib().e2_gaussrv_fwd(ctx.h, *huge, C.c_void_p(st.data_ptr()), 0) != 0
    assert b"2^31" in backend.lib().e2_last_error()


# ---- one VAE, end to end ---------------------------------------------------------------------------
class VaeRef(Ref):
    """``Ref`` with the node kinds of the two nets below; eps of a GaussianRV from the restatement.
    (loss, gradients, parameters) in float64 for the noise of ``counter``"""

    def step(self, x, t, counter):
        m, val = self.model, {}
        for node in m.nodes.values():
            kind, par = type(node).__name__, node.parent
            if kind == 'Input':
                val[node] = torch.tensor(np.asarray(x if node is m.input_node else t, np.float64))
            elif kind in ('Conv', 'UpConv', 'Perceptron'):
                h, w, b = val[par], self.p(node.w), self.p(node.b)
                if kind == 'Perceptron':
                    y = (h.flatten(1) if node.flatten else h) @ w
                elif kind == 'UpConv':
                    y = F.conv_transpose3d(h, w.permute(1, 0, 2, 3, 4), stride=tuple(node.pool_shape))
                else:
                    y = conv_ref(h, w, node.conv_mode)
                    if any(q != 1 for q in node.pool_shape):
                        y = (F.max_pool3d if h.dim() == 5 else F.max_pool2d)(y, tuple(node.pool_shape))
                val[node] = self.act(node, y + b.view((1, -1) + (1,) * (y.dim() - 2)))
            elif kind == 'SplitPart':
                val[node] = val[par][:, node.lo:node.hi]
            elif kind == 'GaussianRV':
                eps = restated_normals(val[par[0]].numel(), SEED, counter, 0).reshape(tuple(val[par[0]].shape))
                val[node] = val[par[0]] + torch.exp(val[par[1]]) * torch.tensor(eps)
            elif kind == 'GaussianAEVBPrior':
                mu, ls = val[par[0]], val[par[1]]
                val[node] = 0.5 * (mu ** 2 + torch.exp(2 * ls) - 1 - 2 * ls)
            elif kind == 'SquaredLoss':
                d = val[par[1]] - val[par[0]]
                val[node] = 0.5 * d * d * d.numel() / (d.numel() + 1.0)      # (nothing is masked)
            elif kind == 'AggregateLoss':
                w = node.mixing_weights.get_value().astype(np.float64)
                val[node] = sum(float(w[k]) * val[q].mean() for k, q in enumerate(par)) / len(par)
        ps = [self.p(p) for p in m.trainable_params]
        gs = torch.autograd.grad(val[m.loss_node], ps)
        return float(val[m.loss_node].detach()), [g.numpy() for g in gs], [p.detach().numpy() for p in ps]


def _vae(kind):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(31)
    if kind == 'conv_split':
        inp = target = nm.Input((2, 1, 4, 20, 20), 'b,f,z,x,y', name='raw')
        enc = nm.Conv(inp, 4, (1, 3, 3), (1, 2, 2), name='enc')
        mu, ls = nm.split(nm.Conv(enc, 6, (1, 1, 1), activation_func='lin', name='both'), 'f', n_out=2)
        z = nm.GaussianRV(mu, ls, name='z')
        recon = nm.Conv(nm.UpConv(z, 4, (1, 2, 2), name='up'), 1, (1, 3, 3), conv_mode='full',
                        activation_func='lin', name='recon')
    else:
        inp = nm.Input((2, 1, 12, 12), 'b,f,y,x', name='raw')
        trunk = nm.Perceptron(nm.Conv(inp, 4, (3, 3), (2, 2), name='enc'), 12, flatten=True, name='trunk')
        z = nm.GaussianRV(nm.Perceptron(trunk, 5, activation_func='lin', name='mu'),
                          nm.Perceptron(trunk, 5, activation_func='lin', name='ls'), name='z')
        recon = nm.Perceptron(z, 7, activation_func='lin', name='recon')
        target = nm.Input_like(recon, name='target')
    loss = nm.AggregateLoss([nm.SquaredLoss(recon, target), z.make_priorlayer()],
                            mixing_weights=[1.0, 0.3], name='loss')
    m = nm.model_manager.getmodel()
    m.designate_nodes(input_node=inp, target_node=None if target is inp else target, loss_node=loss,
                      prediction_node=recon)
    m.set_opt_meta_params('SGD', dict(lr=LR, mom=0.0, wd=0.0))
    rng = np.random.RandomState(32)
    return m, [rng.rand(*n.shape.shape).astype(np.float32) for n in loss.input_nodes]


def _check_step(m, args, tol_loss, tol_grad):
    """loss and every parameter gradient of the eager plans; then SGD steps (eager, captured,
    replayed twice) whose loss and gradient g = (p - p') / LR follow the counter: new noise in every
    replay, the same in the forward and the backward of one"""
    m.set_dropout_seed(SEED, COUNTER)
    loss = float(m.loss(*args))
    m.set_dropout_seed(SEED, COUNTER)
    grads = m.gradients(*args)
    rl, rg, _ = VaeRef(m).step(args[0], args[-1], COUNTER)
    print("loss %.6f ref %.6f" % (loss, rl))
    assert abs(loss - rl) < tol_loss * abs(rl)
    for p, g, r in zip(m.trainable_params, grads, rg):
        assert rel(g, r) < tol_grad, p.name
    losses = []
    for i in range(4):
        rl, rg, rp = VaeRef(m).step(args[0], args[-1], COUNTER + 1 + i)
        losses.append(float(m.trainingstep(*args, optimiser='SGD')[0]))
        assert abs(losses[-1] - rl) < tol_loss * abs(rl), i
        for p, r, old in zip(m.trainable_params, rg, rp):
            g = (old - p.get_value().astype(np.float64)) / LR        # (p' carries one f32 rounding)
            assert np.abs(g - r).max() < tol_grad * np.abs(r).max() + 2.0 ** -23 * np.abs(old).max() / LR, (i, p.name)
    assert len(set(losses)) == 4 and m.dropout_state()['counter'] == COUNTER + 5


@pytest.mark.parametrize("kind,mode", [('conv_split', 'f32'), ('dense_heads', 'f32'), ('conv_split', 'bf16')])
def test_vae_step_against_float64_autograd(kind, mode):
    import elektronn2_amd
    elektronn2_amd.set_mfma_dtype(mode)
    try:
        _check_step(*_vae(kind), **(dict(tol_loss=TOL_STEP, tol_grad=TOL_STEP) if mode == 'f32' else
                                    dict(tol_loss=BF16_LOSS, tol_grad=BF16_GRAD)))
    finally:
        elektronn2_amd.set_mfma_dtype('f32')


def test_checkpoint_round_trip(tmp_path):
    from elektronn2_amd import neuromancer as nm
    m, args = _vae('conv_split')
    m.set_dropout_seed(SEED, COUNTER)
    want = m.loss(*args)
    m.save(str(tmp_path / "vae.mdl"))
    m2 = nm.modelload(str(tmp_path / "vae.mdl"))
    assert [type(n).__name__ for n in m2.nodes.values()] == [type(n).__name__ for n in m.nodes.values()]
    m2.set_dropout_seed(SEED, COUNTER)
    assert m2.loss(*args) == want
