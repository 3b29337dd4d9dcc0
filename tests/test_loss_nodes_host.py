"""EuclideanDistance / RampLoss / BetaNLL / OneHot, host side (no GPU).

``ref_fdist`` / ``ref_ramp`` / ``ref_beta`` / ``ref_onehot`` restate the reference's lines
(loss.py:96-138, 890-950, 1104-1151, 1154-1212) in float64 torch; autograd of them is the reference
of every GPU comparison (tests/test_loss_nodes_gpu.py).  Here each is pinned to a plain NumPy loop
over the reference's expressions, ``ref_beta`` also to torch.distributions.Beta where EPS does not
matter; float32 restatements of what the kernels compute (``k32_*``, the digamma series among
them) meet the float64 reference at the project's bound for ops, and four WRONG float32 variants
miss it.  Then the nodes are constructed without a device and the C ABI is checked for the new
entries.

Two stated departures from the reference's gradient (include/e2hip.h): where the distance is 0, and
where its forward replaced a NaN, EVERY feature's gradient is an exact 0 (T.grad: 0/0).  ``ref_fdist``
is written so that autograd gives exactly that."""
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5
TOL = 2e-5          # ops: of the reference's largest magnitude (tests/test_regression_loss_gpu.py:24)


@pytest.fixture(autouse=True, scope="module")
def the_nodes_under_test():
    """every test of this module is about these nodes, the ones that pin the references alone
    included: without the nodes none of them has anything to say (imported here, not at module
    level, as the other host modules do: collection must not need the built library)"""
    from elektronn2_amd.neuromancer.loss import EuclideanDistance, RampLoss, BetaNLL, OneHot
    return EuclideanDistance, RampLoss, BetaNLL, OneHot


# ---- the float64 restatement -------------------------------------------------------------------------
def ref_fdist(pred, target):
    """loss.py:1143-1146: the L2 norm of target - pred over 'f' (axis 1, kept as one feature), NaN
    as 0.  Positions whose norm is 0 or NaN take no part in the gradient (the stated departure)."""
    d = target - pred
    ss0 = (d.detach() ** 2).sum(dim=1, keepdim=True)
    ok = ss0 > 0                                            # False for 0 and for NaN
    dz = torch.where(ok, d, torch.zeros_like(d))
    ss = (dz * dz).sum(dim=1, keepdim=True)
    return torch.where(ok, torch.sqrt(torch.where(ok, ss, torch.ones_like(ss))), torch.zeros_like(ss))


def ref_ramp(d_low, d_big, margin):
    """loss.py:1200-1206: r = d_low - d_big + margin, r < 0 -> 0, then NaN -> 0, mean over 'f'"""
    r = d_low - d_big + margin
    r = torch.where(r < 0, torch.zeros_like(r), r)
    r = torch.where(torch.isnan(r), torch.zeros_like(r), r)
    return r.mean(dim=1, keepdim=True)


def ref_beta(mode, conc, target):
    """loss.py:936-950"""
    a = mode * (conc - 2) + 1
    b = (1 - mode) * (conc - 2) + 1
    p = torch.lgamma(a + b) - torch.lgamma(a) - torch.lgamma(b) \
        + (a - 1) * torch.log(target + EPS) + (b - 1) * torch.log(1 - target + EPS)
    return -p + torch.nn.functional.softplus(-conc)


def ref_onehot(target, n_class):
    """loss.py:127-132: T.eq(target, arange(n_class)) along 'f' as float"""
    classes = torch.arange(n_class, dtype=target.dtype).view((1, n_class) + (1,) * (target.dim() - 2))
    return (target == classes).to(target.dtype)


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float32).astype(np.float64), requires_grad=grad)


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---- float32 restatements of what the kernels compute ----------------------------------------------------
f32 = np.float32


def k32_fdist(p, t, dout, wrong=None):
    """(out, dpred, dtarget) in float32, csrc/loss_map.hip's expressions"""
    p, t, dout = f32(p), f32(t), f32(dout)
    d = t - p
    ss = np.zeros(p[:, :1].shape, f32)
    for f in range(p.shape[1]):
        ss = ss + d[:, f:f + 1] * d[:, f:f + 1]
    with np.errstate(invalid='ignore', divide='ignore'):
        out = np.sqrt(ss)
        out = np.where(np.isnan(out), f32(0), out).astype(f32)
        dp = np.where(out > 0, (-d / out) * dout, f32(0)).astype(f32)
    return out, dp, (dp if wrong == 'dtarget_sign' else -dp)


def k32_ramp(lo, big, m, dout, wrong=None):
    """(out, dd_low, dd_big) in float32"""
    lo, big, m, dout = f32(lo), f32(big), f32(m), f32(dout)
    F = f32(lo.shape[1])
    with np.errstate(invalid='ignore'):
        r = (lo - big) + m
        pos = (r > 0) if wrong == 'slope_at_zero' else (r >= 0)
        val = np.where(r >= 0, r, f32(0)).astype(f32)
    acc = np.zeros(lo[:, :1].shape, f32)
    for f in range(lo.shape[1]):
        acc = acc + val[:, f:f + 1]
    den = f32(1) if wrong == 'sum_not_mean' else F
    g = np.where(pos, dout / den, f32(0)).astype(f32)
    return (acc / den).astype(f32), g, -g


def k32_digamma(x):
    """the series of csrc/loss_elem.hip's digammaf, operation by operation in float32"""
    x = np.array(x, f32)
    r = np.zeros_like(x)
    for _ in range(6):
        low = x < 6
        r = np.where(low, r - f32(1) / x, r).astype(f32)
        x = np.where(low, x + f32(1), x).astype(f32)
    i1 = f32(1) / x
    i2 = i1 * i1
    ser = i2 * (f32(1 / 12) - i2 * (f32(1 / 120) - i2 * (f32(1 / 252) - i2 * f32(1 / 240))))
    return (r + (np.log(x) - f32(0.5) * i1 - ser)).astype(f32)


def k32_beta(m, c, x, wrong=None):
    """(l, dl/dm, dl/dc) in float32; lgamma through torch float32"""
    m, c, x = f32(m), f32(c), f32(x)
    lg = lambda v: torch.lgamma(torch.from_numpy(np.ascontiguousarray(v, f32))).numpy()
    a = m * (c - f32(2)) + f32(1)
    b = (f32(1) - m) * (c - f32(2)) + f32(1)
    lx, l1x = np.log(x + f32(EPS)), np.log(f32(1) - x + f32(EPS))
    p = lg(a + b) - lg(a) - lg(b) + (a - f32(1)) * lx + (b - f32(1)) * l1x
    l = -p + np.log1p(np.exp(-c))
    pa, pb = k32_digamma(a), k32_digamma(b)
    gm = (c - f32(2)) * ((pa - pb) - lx + l1x)
    wb = m if wrong == 'psi_b_weight' else (f32(1) - m)
    with np.errstate(over='ignore'):                        # (exp(c) = inf: sigmoid(-c) = 0)
        sg = f32(1) / (f32(1) + np.exp(c))
    gc = -k32_digamma(a + b) + m * (pa - lx) + wb * pb - (f32(1) - m) * l1x - sg
    return l.astype(f32), gm.astype(f32), gc.astype(f32)


# ---- inputs ------------------------------------------------------------------------------------------------
def fdist_inputs(rng, shape):
    return rng.randn(*shape).astype(f32), (rng.randn(*shape) * 1.5).astype(f32)


def ramp_inputs(rng, shape, margin):
    """d_low, d_big with |r| >= 2e-3 CONSTRUCTED (r = d_low - d_big + margin)"""
    big = np.abs(rng.randn(*shape)) + 0.1
    r = (2e-3 + rng.rand(*shape) * 0.8) * np.where(rng.rand(*shape) < 0.5, 1.0, -1.0)
    lo = big - margin + r
    return lo.astype(f32), big.astype(f32)


def ramp_gap(lo, big, margin):
    r = lo.astype(np.float64) - big.astype(np.float64) + float(f32(margin))
    return np.abs(r[np.isfinite(r) & (r != 0)]).min()


def beta_inputs(rng, shape):
    """m in [0.02, 0.98], c in [2.1, 500] (log-uniform), x uniform with 10 % hard 0 / 1 labels"""
    n = int(np.prod(shape))
    m = rng.uniform(0.02, 0.98, shape)
    c = np.exp(rng.uniform(np.log(2.1), np.log(500.0), shape))
    x = rng.uniform(0, 1, shape)
    x.flat[rng.permutation(n)[: n // 10]] = rng.randint(0, 2, n // 10)
    return m.astype(f32), np.clip(c, 2.1, 500).astype(f32), x.astype(f32)


def grads_of(out, dout, leaves):
    return [g.numpy() for g in torch.autograd.grad((out * t64(dout)).sum(), leaves)]


# ---- 1. the restatements against plain loops ---------------------------------------------------------------
def test_ref_fdist_and_ref_ramp_against_numpy_loops():
    rng = np.random.RandomState(1)
    shape = (2, 3, 2, 3, 5)
    p, t = fdist_inputs(rng, shape)
    p[0, :, 0, 0, 0] = t[0, :, 0, 0, 0]                     # distance 0
    p[1, 1, 1, 2, 3] = np.nan                               # a NaN in one feature
    out = ref_fdist(t64(p), t64(t)).numpy()
    lo, big = ramp_inputs(rng, shape, 0.5)
    lo[0, 0, 0, 0, 0] = big[0, 0, 0, 0, 0] - f32(0.5)       # r == 0 (dyadic margin: exact)
    lo[1, 2, 1, 1, 1] = np.nan
    rout = ref_ramp(t64(lo), t64(big), 0.5).numpy()
    N, F, D, H, W = shape
    for n in range(N):
        for z in range(D):
            for y in range(H):
                for x in range(W):
                    diff = t[n, :, z, y, x].astype(np.float64) - p[n, :, z, y, x].astype(np.float64)
                    v = np.sqrt((diff ** 2).sum())          # diff.norm(2, axis=f)
                    if np.isnan(v):
                        v = 0.0
                    assert abs(out[n, 0, z, y, x] - v) <= 1e-12 * max(v, 1.0)
                    r = lo[n, :, z, y, x].astype(np.float64) - big[n, :, z, y, x].astype(np.float64) + 0.5
                    with np.errstate(invalid='ignore'):
                        r[r < 0] = 0.0
                    r[np.isnan(r)] = 0.0
                    assert abs(rout[n, 0, z, y, x] - r.mean()) <= 1e-12
    assert out[0, 0, 0, 0, 0] == 0 and out[1, 0, 1, 2, 3] == 0


def test_ref_fdist_gradient_is_the_quotient_and_zero_where_stated():
    rng = np.random.RandomState(2)
    shape = (1, 3, 1, 2, 6)
    p, t = fdist_inputs(rng, shape)
    p[0, :, 0, 0, 0] = t[0, :, 0, 0, 0]
    p[0, 2, 0, 1, 4] = np.nan
    dout = rng.randn(1, 1, 1, 2, 6).astype(f32).astype(np.float64)
    tp, tt = t64(p, True), t64(t, True)
    out = ref_fdist(tp, tt)
    gp, gt = grads_of(out, dout, [tp, tt])
    assert np.all(np.isfinite(gp)) and np.all(np.isfinite(gt))
    assert np.all(gp[0, :, 0, 0, 0] == 0) and np.all(gp[0, :, 0, 1, 4] == 0)
    assert np.array_equal(gt, -gp)
    o = out.detach().numpy()
    with np.errstate(invalid='ignore', divide='ignore'):
        want = -(t.astype(np.float64) - p.astype(np.float64)) / o * dout
    ok = np.broadcast_to(o > 0, shape)
    assert np.abs(gp[ok] - want[ok]).max() <= 1e-12
    # the ramp: slope 1/F at r == 0, 0 where r < 0 or NaN
    lo = np.array([0.25, 1.0, -1.0, np.nan], f32).reshape(1, 4, 1, 1, 1)
    big = np.array([0.75, 0.5, 0.0, 0.0], f32).reshape(1, 4, 1, 1, 1)
    tl, tb = t64(lo, True), t64(big, True)
    gl, gb = grads_of(ref_ramp(tl, tb, 0.5), np.ones((1, 1, 1, 1, 1)), [tl, tb])
    assert gl.ravel().tolist() == [0.25, 0.25, 0.0, 0.0] and np.array_equal(gb, -gl)


def test_ref_beta_against_a_numpy_loop_and_the_beta_density():
    import math
    rng = np.random.RandomState(3)
    m, c, x = beta_inputs(rng, (1, 2, 1, 3, 7))
    out = ref_beta(t64(m), t64(c), t64(x)).numpy()
    for i in range(m.size):
        mm, cc, xx = float(m.flat[i]), float(c.flat[i]), float(x.flat[i])
        a, b = mm * (cc - 2) + 1, (1 - mm) * (cc - 2) + 1
        p = math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + (a - 1) * math.log(xx + EPS) \
            + (b - 1) * math.log(1 - xx + EPS)
        want = -p + math.log1p(math.exp(-cc))
        assert abs(out.flat[i] - want) <= 1e-10 * max(abs(want), 1.0)
    # where EPS does not matter (x well inside (0, 1), moderate c): -log Beta(a, b).pdf(x) + softplus(-c)
    xs = t64(rng.uniform(0.2, 0.8, m.shape))
    cs = t64(rng.uniform(2.5, 20.0, m.shape))
    a, b = t64(m) * (cs - 2) + 1, (1 - t64(m)) * (cs - 2) + 1
    dens = -torch.distributions.Beta(a, b).log_prob(xs) + torch.nn.functional.softplus(-cs)
    assert float((ref_beta(t64(m), cs, xs) - dens).abs().max()) <= 2e-3      # (EPS / 0.2 * (c - 2))
    ours = ref_beta(t64(m), cs, xs)
    assert rel(ours.numpy(), dens.numpy()) < 1e-3


def test_ref_onehot_against_a_numpy_loop():
    t = np.array([0, 1, 2, 3, -1, 2.5, np.nan, 4, 1, 0], f32).reshape(1, 1, 1, 2, 5)
    out = ref_onehot(t64(t), 4).numpy()
    assert out.shape == (1, 4, 1, 2, 5)
    for i in range(10):
        for k in range(4):
            assert out.reshape(4, 10)[k, i] == (1.0 if t.flat[i] == k else 0.0)
    assert out.reshape(4, 10)[:, 4:8].sum() == 0            # -1, 2.5, NaN, n_class: zero columns


# ---- 2. float32 restatements of the kernels, and wrong variants --------------------------------------------
def _fdist_case(rng):
    shape = (2, 5, 2, 3, 7)
    p, t = fdist_inputs(rng, shape)
    dout = rng.randn(2, 1, 2, 3, 7).astype(f32)
    tp, tt = t64(p, True), t64(t, True)
    out = ref_fdist(tp, tt)
    return p, t, dout, out.detach().numpy(), grads_of(out, dout, [tp, tt])


def _ramp_case(rng, with_zero=True):
    shape = (2, 3, 2, 3, 7)
    lo, big = ramp_inputs(rng, shape, 0.5)
    if with_zero:
        lo[:, 0, :, :, 0] = big[:, 0, :, :, 0] - f32(0.5)   # planted r == 0
    dout = rng.randn(2, 1, 2, 3, 7).astype(f32)
    tl, tb = t64(lo, True), t64(big, True)
    out = ref_ramp(tl, tb, 0.5)
    return lo, big, dout, out.detach().numpy(), grads_of(out, dout, [tl, tb])


def _beta_case(rng):
    m, c, x = beta_inputs(rng, (2, 3, 2, 5, 9))
    tm, tc = t64(m, True), t64(c, True)
    out = ref_beta(tm, tc, t64(x))
    return m, c, x, out.detach().numpy(), [g.numpy() for g in torch.autograd.grad(out.sum(), [tm, tc])]


def test_float32_restatements_meet_the_bound():
    rng = np.random.RandomState(4)
    p, t, dout, out, (gp, gt) = _fdist_case(rng)
    o32, dp32, dt32 = k32_fdist(p, t, dout)
    assert rel(o32, out) < TOL and rel(dp32, gp) < TOL and rel(dt32, gt) < TOL
    lo, big, dout, out, (gl, gb) = _ramp_case(rng)
    assert ramp_gap(lo, big, 0.5) >= 1e-3
    o32, dl32, db32 = k32_ramp(lo, big, 0.5, dout)
    assert rel(o32, out) < TOL and rel(dl32, gl) < TOL and rel(db32, gb) < TOL
    m, c, x, out, (gm, gc) = _beta_case(rng)
    l32, gm32, gc32 = k32_beta(m, c, x)
    assert rel(l32, out) < TOL and rel(gm32, gm) < TOL and rel(gc32, gc) < TOL
    assert abs(float(l32.astype(np.float64).mean()) - out.mean()) <= 1e-5 * abs(out.mean())


def test_float32_digamma_series_against_float64():
    x = np.concatenate([np.linspace(1.0, 8.0, 3000), np.exp(np.linspace(0.0, np.log(1000.0), 3000)),
                        [1.0, 2.0, 5.999999, 6.0, 1000.0]]).astype(f32)
    want = torch.special.digamma(torch.from_numpy(x.astype(np.float64))).numpy()
    got = k32_digamma(x)
    assert np.all(np.isfinite(got))
    assert rel(got, want) < TOL
    assert np.abs(got - want).max() < 2e-6                  # (a few float32 ulps of psi <= 6.9)
    # a bounded loop: arguments far outside the domain return, whatever they return
    with np.errstate(all='ignore'):
        k32_digamma(np.array([-1e30, -3.5, 0.0, np.nan, np.inf], f32))


@pytest.mark.parametrize("wrong", ["dtarget_sign", "slope_at_zero", "sum_not_mean", "psi_b_weight"])
def test_wrong_float32_variants_miss_the_bound(wrong):
    rng = np.random.RandomState(5)
    if wrong == "dtarget_sign":
        p, t, dout, out, (gp, gt) = _fdist_case(rng)
        errs = [rel(k32_fdist(p, t, dout, wrong)[2], gt)]
    elif wrong in ("slope_at_zero", "sum_not_mean"):
        lo, big, dout, out, (gl, gb) = _ramp_case(rng)
        o32, dl32, db32 = k32_ramp(lo, big, 0.5, dout, wrong)
        errs = [rel(dl32, gl)] + ([rel(o32, out)] if wrong == "sum_not_mean" else [])
    else:
        m, c, x, out, (gm, gc) = _beta_case(rng)
        errs = [rel(k32_beta(m, c, x, wrong)[2], gc)]
    assert all(e > 100 * TOL for e in errs), (wrong, errs)


# ---- 3. node construction without a device -----------------------------------------------------------------
def _heads(tags='b,f,z,x,y'):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    inp = nm.Input((1, 1, 5, 12, 12), 'b,f,z,x,y', name='raw')
    trunk = nm.Conv(inp, 4, (1, 3, 3))
    v = nm.Conv(trunk, 3, (1, 1, 1), activation_func='lin', name='head_v')
    m = nm.Conv(trunk, 2, (1, 1, 1), activation_func='sigmoid', name='head_m')
    c = nm.Conv(trunk, 2, (1, 1, 1), activation_func='soft+', name='head_c')
    return nm, inp, trunk, v, m, c


def test_nodes_have_the_reference_signatures_names_shapes_and_params():
    import inspect
    nm, inp, trunk, v, m, c = _heads()
    tv = nm.Input_like(v, name='tv')
    ed = nm.EuclideanDistance(v, tv)
    assert ed.name == 'se' and not ed.params and list(ed.parent) == [v, tv]
    assert tuple(ed.shape.shape) == (1, 1, 5, 10, 10) and tuple(ed.shape.tags) == tuple(v.shape.tags)
    assert list(ed.shape.fov) == list(v.shape.fov) and list(ed.shape.strides) == list(v.shape.strides)
    ed2 = nm.EuclideanDistance(tv, v, name='far')
    rl = nm.RampLoss(ed, ed2, margin=0.5)
    assert rl.name == 'se1' and set(rl.params) == {'margin'} and rl.d_low is ed and rl.d_big is ed2
    assert float(rl.params['margin'].get_value()) == 0.5 and not rl.params['margin'].apply_train
    assert tuple(rl.shape.shape) == (1, 1, 5, 10, 10)
    assert list(rl.shape.fov) == list(v.shape.fov)
    r0 = nm.RampLoss(v, tv)                                 # margin None: the parameter exists, 0
    assert float(r0.params['margin'].get_value()) == 0.0 and tuple(r0.shape.shape) == (1, 1, 5, 10, 10)
    tm = nm.Input_like(m, name='tm')
    bn = nm.BetaNLL(m, c, tm)
    assert bn.name == 'beta_nll' and list(bn.parent) == [m, c, tm] and not bn.params
    assert tuple(bn.shape.shape) == (1, 2, 5, 10, 10)       # the mode's shape
    ids = nm.Input_like(m, override_f=1, name='ids')
    oh = nm.OneHot(ids, 2)
    assert oh.name == 'onehot' and oh.n_class == 2 and oh.parent is ids
    assert tuple(oh.shape.shape) == (1, 2, 5, 10, 10) and not oh.params
    assert list(oh.shape.fov) == list(ids.shape.fov) and list(oh.shape.strides) == list(ids.shape.strides)
    for n in (ed, rl, bn):
        assert n.term_value is None and n.n_labelled is None    # nothing has run
    agg = nm.AggregateLoss([rl, nm.SquaredLoss(v, tv), bn, nm.BinaryNLL(m, oh), ed],
                           mixing_weights=[1.0, 0.25, 2.0, 0.5, 1.0])
    assert agg.elementwise and not agg.multi_nll and tuple(agg.shape.shape) == (1,)
    assert nm.AggregateLoss(ed2).elementwise
    sig = lambda k: list(inspect.signature(k.__init__).parameters)[1:]
    assert sig(nm.EuclideanDistance) == ['pred', 'target', 'name', 'print_repr']
    assert sig(nm.RampLoss) == ['d_low', 'd_big', 'name', 'print_repr', 'margin']
    assert sig(nm.BetaNLL) == ['mode', 'concentration', 'target', 'name', 'print_repr']
    assert sig(nm.OneHot) == ['target', 'n_class', 'axis', 'name', 'print_repr']


def test_nodes_on_two_dimensional_and_flat_shapes():
    from elektronn2_amd import neuromancer as nm
    for tags, shape, want in (('b,f,x,y', (2, 3, 8, 9), (2, 1, 8, 9)), ('b,f,y,x', (2, 3, 8, 9), (2, 1, 8, 9)),
                              ('b,f', (4, 5), (4, 1))):
        nm.model_manager.reset()
        a, b = nm.Input(shape, tags, name='a'), nm.Input(shape, tags, name='b')
        ed = nm.EuclideanDistance(a, b)
        assert tuple(ed.shape.shape) == want and tuple(ed.shape.tags) == tuple(a.shape.tags)
        assert tuple(nm.RampLoss(a, b, margin=1).shape.shape) == want
        assert tuple(nm.BetaNLL(a, b, a).shape.shape) == shape
        assert tuple(nm.OneHot(ed, 7).shape.shape) == (shape[0], 7) + tuple(shape[2:])


def test_construction_errors_and_the_refusals_that_stay():
    nm, inp, trunk, v, m, c = _heads()
    tv, tm = nm.Input_like(v, name='tv'), nm.Input_like(m, name='tm')
    with pytest.raises(ValueError, match="one shape"):
        nm.EuclideanDistance(v, tm)
    with pytest.raises(ValueError, match="one shape"):
        nm.RampLoss(v, m)
    with pytest.raises(ValueError, match="both parents are the node"):
        nm.EuclideanDistance(v, v)
    with pytest.raises(ValueError, match="both parents are the node"):
        nm.RampLoss(tv, tv)
    with pytest.raises(ValueError, match="concentration must have the prediction's shape"):
        nm.BetaNLL(m, v, tm)
    with pytest.raises(ValueError, match="target must have the prediction's shape"):
        nm.BetaNLL(m, c, tv)
    with pytest.raises(ValueError, match="one feature"):
        nm.OneHot(tv, 3)
    with pytest.raises(NotImplementedError, match="feature axis"):
        nm.OneHot(nm.Input_like(m, override_f=1, name='ids'), 2, axis='z')
    sa = nm.Input((1, 4, 3, 5, 5), 'b,s,f,x,y', name='samples')
    st = nm.Input_like(sa, name='samples_t')
    s1 = nm.Input((1, 4, 1, 5, 5), 'b,s,f,x,y', name='samples_1')
    for make in (lambda: nm.EuclideanDistance(sa, st), lambda: nm.RampLoss(sa, st),
                 lambda: nm.BetaNLL(sa, sa, st), lambda: nm.OneHot(s1, 3)):
        with pytest.raises(NotImplementedError, match="'s' sample axis"):
            make()
    terms = [nm.EuclideanDistance(v, tv) for _ in range(9)]
    with pytest.raises(ValueError, match="at most 8"):
        nm.AggregateLoss(terms)
    assert nm.AggregateLoss(terms[:8]).elementwise
    # ---- every refusal tests/test_regression_loss_host.py pins still raises
    for make in (lambda: nm.BinaryNLL(sa, st), lambda: nm.SquaredLoss(sa, st),
                 lambda: nm.GaussianNLL(sa, sa, st)):
        with pytest.raises(NotImplementedError, match="'s' sample axis"):
            make()
    with pytest.raises(ValueError, match="target must have the prediction's shape"):
        nm.SquaredLoss(v, tm)
    lin2 = nm.Conv(trunk, 2, (1, 1, 1), activation_func='lin')
    probs = nm.Softmax(lin2)
    tc = nm.Input_like(probs, override_f=1, name='tc')
    with pytest.raises(NotImplementedError, match="dense"):
        nm.MultinoulliNLL(probs, tc, target_is_sparse=False)
    with pytest.raises(NotImplementedError, match="dense"):
        nm.MultinoulliNLL(probs, nm.OneHot(tc, 2))          # (OneHot does not open the dense NLL)
    nll = nm.MultinoulliNLL(probs, tc, target_is_sparse=True)
    with pytest.raises(NotImplementedError, match="take no scale"):
        nm.AggregateLoss([nll, terms[0]])
    with pytest.raises(NotImplementedError, match="take no scale"):
        nm.AggregateLoss([nll, nm.BetaNLL(m, c, tm)])
    with pytest.raises(NotImplementedError, match="take no scale"):
        nm.AggregateLoss([nll, nll])
    with pytest.raises(NotImplementedError):
        nm.AggregateLoss([v])
    with pytest.raises(NotImplementedError):
        nm.AggregateLoss([nm.OneHot(tc, 2)])                # not a loss
    with pytest.raises(NotImplementedError, match="activation_func='concentration'"):
        nm.Conv(trunk, 2, (1, 1, 1), activation_func='concentration')
    single = nm.AggregateLoss(nll)
    assert not single.elementwise and list(single.parent) == [nll]


def test_new_nodes_are_exported_and_found_by_modelload():
    from elektronn2_amd import neuromancer as nm
    from elektronn2_amd.neuromancer import loss as loss_mod
    for k in ('EuclideanDistance', 'RampLoss', 'BetaNLL', 'OneHot'):
        assert getattr(nm, k) is getattr(loss_mod, k) and k in loss_mod.__all__
    assert 'BlockedMultinoulliNLL' not in loss_mod.__all__   # (the reference's equals MultinoulliNLL)
    doc = loss_mod.__doc__
    for k in ('EuclideanDistance', 'RampLoss', 'BetaNLL', 'OneHot', 'loss_map.hip'):
        assert k in doc, k


def _triplet_model():
    nm, inp, trunk, v, m, c = _heads()
    tv, tm = nm.Input_like(v, name='tv'), nm.Input_like(m, name='tm')
    ids = nm.Input_like(m, override_f=1, name='ids')
    ed, ed2 = nm.EuclideanDistance(v, tv, name='near'), nm.EuclideanDistance(tv, v, name='far')
    rl = nm.RampLoss(ed, ed2, margin=0.5, name='ramp')
    agg = nm.AggregateLoss([rl, nm.BetaNLL(m, c, tm), nm.BinaryNLL(m, nm.OneHot(ids, 2))],
                           mixing_weights=[1.0, 0.25, 2.0], name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=tv, loss_node=agg, prediction_node=v)
    return model


def test_descriptors_serialise_and_modelload_rebuilds_them(tmp_path):
    from elektronn2_amd.neuromancer.model import modelload
    model = _triplet_model()
    d = json.loads(json.dumps(model.serialise()))
    by = dict((n[0], n) for n in d["nodes"])
    assert by['near'][1] == 'EuclideanDistance' and by['ramp'][1] == 'RampLoss'
    assert by['ramp'][3]['margin'] == 0.5
    assert by['beta_nll'][1] == 'BetaNLL' and by['onehot'][1] == 'OneHot' and by['onehot'][2][1] == 2
    model.nodes['ramp'].params['margin'].set_value(np.float32(0.75))
    f = str(tmp_path / "nodes.mdl")
    model.save(f)
    c = modelload(f)
    assert [type(n).__name__ for n in c.loss_node.parent] == ['RampLoss', 'BetaNLL', 'BinaryNLL']
    assert c.loss_node.elementwise
    assert float(c.nodes['ramp'].params['margin'].get_value()) == 0.75
    assert c.nodes['onehot'].n_class == 2 and type(c.nodes['ramp'].d_low).__name__ == 'EuclideanDistance'
    assert np.array_equal(c.loss_node.params['mixing_weights'].get_value(), np.asarray([1.0, 0.25, 2.0], f32))
    for k, p in model.loss_node.all_trainable_params.items():
        assert np.array_equal(p.get_value(), c.loss_node.all_trainable_params[k].get_value())


def test_a_branch_that_only_borrows_parameters_still_needs_its_gradient():
    """a siamese branch owns no parameter (``w=<other>.w``): its backward launches add to the shared
    gradient slots all the same, so the plan must ask for them"""
    from elektronn2_amd import neuromancer as nm
    from elektronn2_amd.neuromancer.plan import Plan
    nm.model_manager.reset()
    xa, xp = (nm.Input((1, 1, 5, 14, 14), 'b,f,z,x,y', name=k) for k in ('raw', 'pos'))
    c1 = nm.Conv(xa, 4, (1, 3, 3), name='c1')
    ea = nm.Conv(c1, 3, (3, 3, 3), activation_func='tanh', name='emb')
    c1p = nm.Conv(xp, 4, (1, 3, 3), w=c1.w, b=c1.b, name='c1_pos')
    ep = nm.Conv(c1p, 3, (3, 3, 3), activation_func='tanh', w=ea.w, b=ea.b, name='emb_pos')
    # (construction only: a ConstantParam has no slot in the device arena, this plan is never built)
    frozen = nm.Conv(xp, 3, (3, 5, 5), w=[np.zeros((3, 1, 3, 5, 5), f32), 'const'],
                     b=[np.zeros(3, f32), 'const'], name='frozen')
    loss = nm.AggregateLoss([nm.EuclideanDistance(ea, ep, name='near'),
                             nm.EuclideanDistance(ea, frozen, name='fixed')], name='loss')
    assert not ep.params and not c1p.params and not ep.all_trainable_params
    assert ep.borrowed_params == [ea.w, ea.b] and not hasattr(ea, 'borrowed_params')
    plan = Plan(loss.input_nodes, [loss], model=nm.model_manager.getmodel(), step='grad')
    need = dict((n.name, plan.needs_grad(n)) for n in plan.nodes)
    assert need == dict(raw=False, pos=False, c1=True, emb=True, c1_pos=True, emb_pos=True, frozen=False,
                        near=True, fixed=True, loss=True), need
    fwd = Plan(loss.input_nodes, [loss], model=nm.model_manager.getmodel(), step=None)
    assert not any(fwd.needs_grad(n) for n in fwd.nodes)


# ---- 4. C ABI -------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("e2_fdist_fwd", "e2_fdist_bwd", "e2_ramp_fwd", "e2_ramp_bwd", "e2_mean_fwd", "e2_mean_bwd",
               "e2_beta_nll_fwd", "e2_beta_nll_bwd", "e2_onehot")


def test_header_declares_and_backend_binds_the_new_entries():
    from elektronn2_amd import backend
    src = open(os.path.join(ROOT, "include", "e2hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, plain), s
        assert s in backend.EXPORTED_SYMBOLS, s
        assert hasattr(backend.lib(), s)
    for method in ("fdist_fwd", "fdist_bwd", "ramp_fwd", "ramp_bwd", "mean_fwd", "mean_bwd", "beta_nll_fwd",
                   "beta_nll_bwd", "onehot"):
        assert callable(getattr(backend.Context, method))
    # the formula table and the two departures stand in the header
    for text in ("T.grad gives 0/0", "EVERY feature receives an exact 0", "GAUSS_NLL-kind descriptor",
                 "psi(a) - psi(b)", "guard nothing", "slope of the ramp AT r == 0 is 1"):
        assert text in src, text
    # what the existing tests pin is untouched: the enum, the kinds, the descriptor
    assert backend.LOSS == {"squared": 0, "abs": 1, "binary_nll": 2, "gauss_nll": 3}
    assert [f[0] for f in backend.LossTerm._fields_] == ['kind', 'margin', 'scale_correction',
                                                         'subtract_label_entropy', 'sig_is_log']
    mk = open(os.path.join(ROOT, "elektronn2_amd", "csrc", "Makefile")).read()
    assert "loss_map.hip" in mk and "e2map_" in mk
