"""csrc/dense_bn.hip through the C ABI and through the plan: e2_batchnorm_act_fwd / _bwd (every
``batch_normalisation=`` of Conv / UpConv / Perceptron) and e2_dense_fwd / dgrad / wgrad (the
Perceptron), at the shapes, views and corners where they can go wrong.

The reference of every number is float64 and never the code under test: oracle/bn_oracle.py's
closed forms for the ops (pinned against autograd and a plain loop in tests/test_batchnorm_host.py,
which also proves what each planted input is planted for), float64 ``@`` for the dense sums, and
``BnRef`` (torch float64 autograd of the restated graph) for whole steps.

Bounds.  The ones the op test had in tests/test_mnist_gpu.py stay: 1e-5 for ``out`` / ``save``,
2e-5 for the gradients, 1e-6 for ``run_std``, 2e-6 for the dense sums with k <= 57 -- now per
CHANNEL (test_batchnorm_host.chan_err: each channel's largest error over that channel's largest
reference magnitude; against ABS_FLOOR = 1.0, the scale of the inputs, where a channel's reference
is exactly 0), so that no channel hides behind a larger one.  Whole steps: TOL = 1e-4 as in
tests/test_mnist_gpu.py.  Two bounds are computed by the tests and printed, because no fixed one
holds by construction:

  * the offset input x = 30 + 0.25 randn (test_offset_input_holds_the_two_pass_bound): 8 x the
    error against float64 of the float32 two-pass NumPy restatement of the same arithmetic (the
    factor for the other summation order).  tests/test_batchnorm_host.py shows that a one-pass
    E[x^2] - mean^2 misses it (std: 1.2e-7 two-pass, 1e-4 and more one-pass).  Worst channel,
    relative to float64 -- restatement on the CPU / bound = 8 x / kernel on the MI355X:

                   (3, 5, 2, 4, 7)                    (2, 3, 3, 17, 19)
        out        9.87e-06 / 7.89e-05 / 5.93e-06     7.25e-06 / 5.80e-05 / 2.11e-06
        mean       7.46e-08 / 5.97e-07 / 1.16e-07     5.40e-08 / 4.32e-07 / 6.87e-08
        std        1.19e-07 / 9.51e-07 / 1.19e-07     8.70e-08 / 6.96e-07 / 8.70e-08
        run_mean   1.20e-07 / 9.58e-07 / 1.20e-07     4.74e-08 / 3.80e-07 / 4.74e-08
        run_std    8.08e-08 / 6.47e-07 / 8.08e-08     1.13e-07 / 9.07e-07 / 1.13e-07
        dx         1.81e-05 / 1.45e-04 / 3.05e-05     1.34e-05 / 1.07e-04 / 2.14e-05
        dgamma     8.63e-06 / 6.91e-05 / 1.37e-05     7.93e-06 / 6.34e-05 / 1.00e-05
        dbias      1.05e-07 / 8.38e-07 / 7.90e-08     5.97e-08 / 4.78e-07 / 4.27e-08

  * the dense sums with k > 57 (test_dense_fwd_dgrad_wgrad_into_watched_windows): 4 x the error
    against float64 of a float32 restatement in the kernels' order (oracle/bn_oracle.py
    ``dense_f32_sequential``: one accumulator per output, fma term by term, then base + sum).  The
    kernels run exactly that arithmetic: on the MI355X every figure equals the CPU restatement's
    to the digits printed.  whole-tensor error, restatement = kernel / bound = 4 x:

        (n, k, m)        fwd                   dgrad, accumulate off / on                   wgrad, accumulate off / on
        (1, 300, 1)      4.22e-07 (1.69e-06)   3.52e-08 (1.41e-07) / 5.31e-08 (2.12e-07)    3.71e-08 (1.48e-07) / 4.70e-08 (1.88e-07)
        (20, 576, 200)   8.15e-07 (3.26e-06)   6.03e-07 (2.41e-06) / 6.10e-07 (2.44e-06)    1.60e-07 (6.39e-07) / 1.70e-07 (6.80e-07)
        (20, 200, 10)    2.49e-07 (9.96e-07)   9.19e-08 (3.68e-07) / 8.45e-08 (3.38e-07)    1.48e-07 (5.93e-07) / 1.51e-07 (6.03e-07)
        (2, 513, 5)      4.33e-07 (1.73e-06)   1.14e-07 (4.56e-07) / 1.19e-07 (4.74e-07)    5.71e-08 (2.28e-07) / 7.05e-08 (2.82e-07)
"""
import numpy as np
import pytest
import torch

from oracle import bn_oracle as BO
from oracle import e2_oracle as O
from oracle import mnist_oracle as MO
from strided_views import assert_outside_untouched, make_view
from test_activations_host import act_f
from test_batchnorm_host import (BN_KEYS, BN_SHAPES, CORNER_SHAPES, DENSE_LONG_K, DENSE_SHAPES, DENSE_TOL,
                                 DYADIC_CH, NETS, OFFSET_SHAPES, SGD, TOL_GRAD, TOL_OUT, TOL_RUN_STD, BnRef,
                                 all_cases, args_of, bn_case, bn_nodes, bn_ref, chan_err, dense_case,
                                 dense_refs, feed_for, mnist_batches, net_small, params_by_value)

pytestmark = pytest.mark.gpu
TOL = 1e-4
GEOMS = ("frame111", "cslice", "cslice_frame", "planes", "odd_base")


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def dev(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def all_params(m):
    out = {}
    for node in m.nodes.values():
        for k, p in node.params.items():
            if k in ('w', 'b') + BN_KEYS:
                out['%s_%s' % (node.name, k)] = p.get_value()
    return out


# ---- the op the suite had: moved here from tests/test_mnist_gpu.py, every assertion kept ----------
def test_dense_and_batchnorm_ops(ctx):
    rng = np.random.RandomState(5)
    x = rng.randn(20, 57).astype(np.float32)
    w = rng.randn(57, 33).astype(np.float32)
    dy = rng.randn(20, 33).astype(np.float32)
    y = torch.empty(20, 33, device="cuda")
    ctx.dense_fwd(dev(x), dev(w), y)
    assert rel(y.cpu().numpy(), x.astype(np.float64) @ w) < 2e-6
    dx = torch.full((20, 57), float("nan"), device="cuda")
    ctx.dense_dgrad(dev(dy), dev(w), dx)
    assert rel(dx.cpu().numpy(), dy.astype(np.float64) @ w.T) < 2e-6
    ctx.dense_dgrad(dev(dy), dev(w), dx, accumulate=True)
    assert rel(dx.cpu().numpy(), 2 * (dy.astype(np.float64) @ w.T)) < 2e-6
    dw = torch.zeros(57, 33, device="cuda")
    ctx.dense_wgrad(dev(x), dev(dy), dw, accumulate=True)
    ctx.dense_wgrad(dev(x), dev(dy), dw, accumulate=True)
    assert rel(dw.cpu().numpy(), 2 * (x.astype(np.float64).T @ dy)) < 2e-6
    # batch norm + relu, train mode, gradient through the statistics, strided dx view
    for shape in [(20, 12, 1, 12, 12), (3, 5, 2, 4, 7), (20, 200, 1, 1, 1)]:
        xb = rng.randn(*shape).astype(np.float32) * 2 + 0.5
        g = (rng.rand(shape[1]) + 0.5).astype(np.float32)
        b = rng.randn(shape[1]).astype(np.float32) * 0.3
        do = rng.randn(*shape).astype(np.float32)
        X = torch.tensor(xb, dtype=torch.float64, requires_grad=True)
        G = torch.tensor(g, dtype=torch.float64, requires_grad=True)
        B = torch.tensor(b, dtype=torch.float64, requires_grad=True)
        yb, mean, std = MO.batchnorm(X, G, B)
        out_ref = MO.relu(yb)
        (out_ref * torch.tensor(do, dtype=torch.float64)).sum().backward()
        rm = torch.zeros(shape[1], device="cuda"); rs = torch.ones(shape[1], device="cuda")
        out = torch.full(shape, float("nan"), device="cuda")
        save = torch.zeros(2 * shape[1], device="cuda")
        ctx.batchnorm_act_fwd(dev(xb), dev(g), dev(b), rm, rs, True, True, 'relu', out, save)
        assert rel(out.cpu().numpy(), out_ref.detach().numpy()) < 1e-5
        assert rel(save[:shape[1]].cpu().numpy(), mean.detach().numpy()) < 1e-5
        assert rel(save[shape[1]:].cpu().numpy(), std.detach().numpy()) < 1e-5
        assert rel(rm.cpu().numpy(), 0.0005 * mean.detach().numpy()) < 1e-5
        assert rel(rs.cpu().numpy(), 0.9995 + 0.0005 * std.detach().numpy()) < 1e-6
        big = torch.zeros((shape[0], shape[1], shape[2] + 2, shape[3] + 2, shape[4] + 3), device="cuda")
        dxv = big[:, :, 1:-1, 1:-1, 2:-1]
        dg = torch.zeros(shape[1], device="cuda"); db = torch.zeros(shape[1], device="cuda")
        ctx.batchnorm_act_bwd(dev(do), dev(xb), dev(g), dev(b), save, True, 'relu', dxv, dg, db)
        assert rel(dxv.cpu().numpy(), X.grad.numpy()) < 2e-5
        assert rel(dg.cpu().numpy(), G.grad.numpy()) < 2e-5
        assert rel(db.cpu().numpy(), B.grad.numpy()) < 2e-5
        border = big.clone()
        border[:, :, 1:-1, 1:-1, 2:-1] = 0
        assert not border.any()                    # nothing written outside the view
        # predict mode: stored statistics, constants of the gradient
        rm2 = dev(rng.randn(shape[1])); rs2 = dev(rng.rand(shape[1]) + 0.5)
        ctx.batchnorm_act_fwd(dev(xb), dev(g), dev(b), rm2, rs2, False, False, 'lin', out, save)
        ref = (g / rs2.cpu().numpy()).reshape(1, -1, 1, 1, 1) * xb + \
            (b - g * rm2.cpu().numpy() / rs2.cpu().numpy()).reshape(1, -1, 1, 1, 1)
        assert rel(out.cpu().numpy(), ref) < 1e-5


# ---- A. batch norm through the C ABI -------------------------------------------------------------
GRAD_BASE_SEED = 17


def grad_base(C):
    """what dgamma / dbias hold before the backward adds to them: non-zero, O(1)"""
    rng = np.random.RandomState(GRAD_BASE_SEED)
    return (rng.randn(C) + 3).astype(np.float32), (rng.randn(C) - 3).astype(np.float32)


class Launch(object):
    """one forward + backward of a case through the C ABI.  ``views``: which of x / out / dout / dx
    live in a ``make_view`` of ``geom`` inside watched storage (the others are dense tensors; out
    and dx NaN-filled).  ``skip``: which of dgamma / dbias / dx are passed as NULL.  Afterwards:
    out, save, run_mean, run_std, dx, dgamma, dbias as NumPy (None where not produced)."""

    def __init__(self, ctx, shape, kind, act, train, geom=None, views=(), update=None,
                 with_save=True, skip=(), zero_base=False, dout=None):
        c = bn_case(shape, kind)
        C = shape[1]
        self.watched, self.read_only = [], []

        def place(name, data, seed):
            if name in views:
                st, v, _, mask = make_view(shape, geom, seed)
                if data is not None:
                    v.copy_(dev(data))
                (self.watched if data is None else self.read_only).append((name, st, st.clone(), mask))
                return v
            return dev(data) if data is not None else torch.full(shape, float("nan"), device="cuda")
        xv = place('x', c['x'], 1)
        ov = place('out', None, 2)
        gv = place('dout', c['dout'] if dout is None else dout, 3)
        dv = None if 'dx' in skip else place('dx', None, 4)
        g, b = dev(c['gamma']), dev(c['bias'])
        rm, rs = dev(c['run_mean']), dev(c['run_std'])
        update = train if update is None else update
        save = torch.zeros(2 * C, device="cuda") if with_save else None
        ctx.batchnorm_act_fwd(xv, g, b, rm, rs, train, update, act, ov, save)
        # (the backward reads the statistics the forward used: in predict mode the stored ones)
        save_b = save if with_save else torch.cat([rm, rs])
        dg0, db0 = (np.zeros(C, np.float32),) * 2 if zero_base else grad_base(C)
        dg = None if 'dgamma' in skip else dev(dg0)
        db = None if 'dbias' in skip else dev(db0)
        ctx.batchnorm_act_bwd(gv, xv, g, b, save_b, train, act, dv, dg, db)
        torch.cuda.synchronize()
        num = lambda t: None if t is None else t.cpu().numpy()
        self.out, self.save, self.run_mean, self.run_std = num(ov), num(save), num(rm), num(rs)
        self.dx, self.dgamma, self.dbias = num(dv), num(dg), num(db)
        self.inputs_unchanged = same_bits(g, c['gamma']) and same_bits(b, c['bias']) and \
            same_bits(xv, c['x']) and same_bits(gv, c['dout'] if dout is None else dout)

    def check_storage(self):
        for name, st, clone, mask in self.watched:
            assert_outside_untouched(st, clone, mask)
        for name, st, clone, mask in self.read_only:
            assert torch.equal(st.view(torch.int32), clone.view(torch.int32)), name   # only read
        assert self.inputs_unchanged


def errors_of(L, r, shape, kind, train, base=True):
    """quantity -> (per-channel error against the float64 closed forms, fixed bound)"""
    C = shape[1]
    dg0, db0 = grad_base(C) if base else (np.zeros(C), np.zeros(C))
    e = {'out': (chan_err(L.out, r['out']), TOL_OUT)}
    if L.save is not None:
        e['mean'] = (chan_err(L.save[:C], r['mean']), TOL_OUT)
        e['std'] = (chan_err(L.save[C:], r['std']), TOL_OUT)
    if train:
        e['run_mean'] = (chan_err(L.run_mean, r['run_mean']), TOL_OUT)
        e['run_std'] = (chan_err(L.run_std, r['run_std']), TOL_RUN_STD)
    if L.dx is not None:
        e['dx'] = (chan_err(L.dx, r['dx']), TOL_GRAD)
    # what the launch ADDED, against the reference sum (the rounding of base + sum is below)
    if L.dgamma is not None:
        e['dgamma'] = (chan_err(L.dgamma.astype(np.float64) - dg0, r['dgamma']), TOL_GRAD)
    if L.dbias is not None:
        e['dbias'] = (chan_err(L.dbias.astype(np.float64) - db0, r['dbias']), TOL_GRAD)
    return e


_DENSE_LAUNCH = {}


def dense_launch(ctx, shape, kind, act, train):
    """the launch with every tensor dense: made once per case, the bits every other layout must give"""
    key = (shape, kind, act, train)
    if key not in _DENSE_LAUNCH:
        _DENSE_LAUNCH[key] = Launch(ctx, shape, kind, act, train)
    return _DENSE_LAUNCH[key]


PLAIN_AND_CORNERS = [c for c in all_cases() if c[1] != 'offset']


@pytest.mark.parametrize("train", [True, False], ids=["train", "predict"])
@pytest.mark.parametrize("act", ['relu', 'lin'])
@pytest.mark.parametrize("shape,kind", PLAIN_AND_CORNERS, ids=lambda v: str(v).replace(' ', ''))
def test_fwd_and_bwd_against_the_closed_forms(ctx, shape, kind, act, train):
    """every output per channel at the fixed bounds; running statistics from a random start; the
    `+=` into non-zero dgamma / dbias; a second launch gives the same bits; update_running off and
    save == NULL change nothing else"""
    r = bn_ref(shape, kind, act, train)
    c = bn_case(shape, kind)
    C = shape[1]
    L = dense_launch(ctx, shape, kind, act, train)
    errs = errors_of(L, r, shape, kind, train)
    print(shape, kind, act, "train" if train else "predict",
          " ".join("%s %.1e" % (k, v[0]) for k, v in errs.items()))
    for k, (e, bound) in errs.items():
        assert e < bound, (k, e, bound)
    for a in (L.out, L.dx, L.dgamma, L.dbias, L.save):
        assert np.isfinite(a).all()
    L.check_storage()
    if train:
        assert not same_bits(L.run_mean, c['run_mean']) and not same_bits(L.run_std, c['run_std'])
    else:                                   # predict mode never writes the statistics
        assert same_bits(L.run_mean, c['run_mean']) and same_bits(L.run_std, c['run_std'])
        assert same_bits(L.save, np.concatenate([c['run_mean'], c['run_std']]))
    # the += is one read-add-write per channel: base + (the sum a zeroed buffer receives)
    Z = Launch(ctx, shape, kind, act, train, zero_base=True)
    dg0, db0 = grad_base(C)
    assert same_bits(L.dgamma, dg0 + Z.dgamma) and same_bits(L.dbias, db0 + Z.dbias)
    assert not same_bits(L.dbias, Z.dbias)
    # again, with what may be switched off switched off: the same bits everywhere else
    again = Launch(ctx, shape, kind, act, train, update=False, with_save=train)
    for k in ('out', 'dx', 'dgamma', 'dbias'):
        assert same_bits(getattr(again, k), getattr(L, k)), k
    assert same_bits(again.run_mean, c['run_mean']) and same_bits(again.run_std, c['run_std'])
    if train:
        assert same_bits(again.save, L.save)
    else:
        assert again.save is None                   # save == NULL: nothing else changed (above)


@pytest.mark.parametrize("train", [True, False], ids=["train", "predict"])
@pytest.mark.parametrize("skip", ['dgamma', 'dbias', 'dx'])
def test_null_gradient_outputs_leave_the_others_to_the_bit(ctx, skip, train):
    """what a non-trainable gamma (predict mode), a node without bias gradient or a node whose
    parent needs no gradient passes; act = lin in the backward as well as relu"""
    for shape in BN_SHAPES:
        for act in ('relu', 'lin'):
            kind = 'corners' if shape in CORNER_SHAPES else 'plain'
            L = dense_launch(ctx, shape, kind, act, train)
            N = Launch(ctx, shape, kind, act, train, skip=(skip,))
            assert getattr(N, skip) is None
            for k in ('out', 'save', 'dx', 'dgamma', 'dbias'):
                if k != skip:
                    assert same_bits(getattr(N, k), getattr(L, k)), (shape, act, k)


@pytest.mark.parametrize("views", [('x',), ('out',), ('dout',), ('dx',), ('x', 'out', 'dout', 'dx')],
                         ids=["x", "out", "dout", "dx", "all"])
@pytest.mark.parametrize("geom", GEOMS)
def test_strided_views_give_the_dense_bits_and_touch_nothing_else(ctx, geom, views):
    """x, out, dout, dx in turn and together as the views the plan hands over (the interior of a
    zero frame, a channel slice of a concat buffer, both, strided planes, a misaligned base): the
    values against float64, every bit of the dense launch (the summation order is fixed: the layout
    must not change one), and no store outside the views"""
    for shape in BN_SHAPES:
        kind = 'corners' if shape in CORNER_SHAPES else 'plain'
        for act, train in (('relu', True), ('lin', False)):
            r = bn_ref(shape, kind, act, train)
            D = dense_launch(ctx, shape, kind, act, train)
            L = Launch(ctx, shape, kind, act, train, geom=geom, views=views)
            for k, (e, bound) in errors_of(L, r, shape, kind, train).items():
                assert e < bound, (shape, act, k, e, bound)
            for k in ('out', 'save', 'run_mean', 'run_std', 'dx', 'dgamma', 'dbias'):
                assert same_bits(getattr(L, k), getattr(D, k)), (shape, act, k)
            L.check_storage()


@pytest.mark.parametrize("shape", CORNER_SHAPES, ids=lambda v: str(v).replace(' ', ''))
def test_exact_zero_pre_activations_carry_half_the_gradient(ctx, shape):
    """the dyadic-symmetric channel under bias 0 has mean exactly 0, so its planted zeros are
    pre-activations of exactly 0 (tests/test_batchnorm_host.py): relu'(0) = 0.5.
    Train mode: a dout that is non-zero ONLY there, in multiples of 1/4, sums exactly, and dbias of
    that channel is exactly half of its sum.  Predict mode with mean 0, std 1, gamma 1, bias 0:
    dx = dout / 2 at the zeros, dout where x > 0, 0 where x < 0, to the bit."""
    c = bn_case(shape, 'corners')
    zeros = np.zeros(shape, bool)
    zeros[:, DYADIC_CH] = c['x'][:, DYADIC_CH] == 0
    rng = np.random.RandomState(9)
    dout = np.where(zeros, rng.randint(1, 9, shape) / 4.0, 0.0).astype(np.float32)
    L = Launch(ctx, shape, 'corners', 'relu', True, zero_base=True, dout=dout)
    assert L.save[DYADIC_CH] == 0.0                                    # the mean, exactly
    assert np.all(L.out[zeros] == 0.0)
    assert L.dbias[DYADIC_CH] == 0.5 * dout.sum(dtype=np.float64)
    assert np.all(np.delete(L.dbias, DYADIC_CH) == 0.0)
    # predict mode, identity statistics
    C = shape[1]
    x = dev(c['x'])
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    full = (rng.rand(*shape) + 0.5).astype(np.float32)
    out = torch.full(shape, float("nan"), device="cuda")
    dx = torch.full(shape, float("nan"), device="cuda")
    save = torch.full((2 * C,), float("nan"), device="cuda")
    ctx.batchnorm_act_fwd(x, one, zero, zero.clone(), one.clone(), False, False, 'relu', out, save)
    db = torch.zeros(C, device="cuda")
    ctx.batchnorm_act_bwd(dev(full), x, one, zero, save, False, 'relu', dx, None, db)
    want = np.where(c['x'] > 0, full, np.where(c['x'] == 0, np.float32(0.5) * full, np.float32(0)))
    assert same_bits(dx, want.astype(np.float32))
    assert same_bits(out, np.maximum(c['x'], 0))
    assert zeros.sum() >= 2 and np.all(dx.cpu().numpy()[zeros] == 0.5 * full[zeros])


OFFSET_KEYS = ('out', 'mean', 'std', 'run_mean', 'run_std', 'dx', 'dgamma', 'dbias')


@pytest.mark.parametrize("shape", OFFSET_SHAPES, ids=lambda v: str(v).replace(' ', ''))
def test_offset_input_holds_the_two_pass_bound(ctx, shape):
    """x = 30 + 0.25 randn.  The fixed bounds do not hold by construction here (the mean carries
    30 * 2^-24 against a spread of 0.25), so the bound of every quantity is computed: 8 x the error
    against float64 of the float32 two-pass NumPy restatement of the same arithmetic (the factor
    allows for the kernels' summation order).  A one-pass variance is 100 x and more away
    (tests/test_batchnorm_host.py)."""
    c = bn_case(shape, 'offset')
    C = shape[1]
    r = bn_ref(shape, 'offset', 'relu', True)
    f = BO.fwd_bwd(c['x'], c['gamma'], c['bias'], c['dout'], 'relu', dtype=np.float32)
    f['run_mean'], f['run_std'] = BO.running_update(c['run_mean'], c['run_std'], f['mean'], f['std'], np.float32)
    L = Launch(ctx, shape, 'offset', 'relu', True, zero_base=True)
    got = dict(out=L.out, mean=L.save[:C], std=L.save[C:], run_mean=L.run_mean, run_std=L.run_std,
               dx=L.dx, dgamma=L.dgamma, dbias=L.dbias)
    failed = []
    for k in OFFSET_KEYS:
        e_np, e_hip = chan_err(f[k], r[k]), chan_err(got[k], r[k])
        print("%s %-8s float32 two-pass restatement %.2e  bound %.2e  kernel %.2e" % (shape, k, e_np, 8 * e_np, e_hip))
        if not e_hip <= 8 * e_np:
            failed.append((k, e_hip, 8 * e_np))
    assert not failed, failed
    L.check_storage()


def test_bad_batchnorm_arguments_raise(ctx):
    from elektronn2_amd import backend
    sh = (2, 3, 1, 4, 5)
    x, out = torch.zeros(sh, device="cuda"), torch.zeros(sh, device="cuda")
    v = torch.ones(3, device="cuda")
    save = torch.zeros(6, device="cuda")
    other = torch.zeros((2, 3, 1, 4, 6), device="cuda")
    with pytest.raises(backend.E2Error, match="e2_batchnorm_act_fwd"):
        ctx.batchnorm_act_fwd(x, v, v, v, v, True, True, 'relu', other, save)
    with pytest.raises(backend.E2Error, match="e2_batchnorm_act_fwd"):
        ctx.batchnorm_act_fwd(x, v, v, None, None, False, False, 'relu', out, save)   # predict, no statistics
    with pytest.raises(backend.E2Error, match="e2_batchnorm_act_fwd"):
        ctx.batchnorm_act_fwd(x, v, v, v, v, False, True, 'relu', out, save)          # update in predict mode
    with pytest.raises(backend.E2Error, match="e2_batchnorm_act_bwd"):
        ctx.batchnorm_act_bwd(other, x, v, v, save, True, 'relu', out, v, v)
    with pytest.raises(backend.E2Error, match="e2_batchnorm_act_bwd"):
        ctx.batchnorm_act_bwd(x, x, v, v, save, True, 'relu', other, v, v)
    with pytest.raises(backend.E2Error, match="e2_batchnorm_act_bwd"):
        ctx.batchnorm_act_bwd(x, x, v, v, None, True, 'relu', out, v, v)


# ---- B. the Perceptron's sums through the C ABI --------------------------------------------------
def _window(n_el, geom, seed, fill):
    """a flat window of n_el floats inside watched storage, NaN-filled or holding ``fill``"""
    st, v, _, mask = make_view((1, 1, 1, 1, n_el), geom, seed)
    flat = v.reshape(-1)
    assert flat.data_ptr() == v.data_ptr() and flat.is_contiguous()
    if fill is None:
        flat.fill_(float("nan"))
    else:
        flat.copy_(dev(fill).reshape(-1))
    return st, flat, st.clone(), mask


@pytest.mark.parametrize("geom", ["dense", "odd_base"])
@pytest.mark.parametrize("n,k,m", DENSE_SHAPES, ids=lambda v: str(v))
def test_dense_fwd_dgrad_wgrad_into_watched_windows(ctx, n, k, m, geom):
    """y = x w, dx (+)= dy w^T, dw (+)= x^T dy against float64: accumulate=False into NaN, True onto
    random values; no store outside n * m / n * k / k * m.  Bound 2e-6 for k <= 57, else 4 x the
    error of the float32 sequential-fma restatement (printed)."""
    c = dense_case(n, k, m)
    refs = dense_refs(n, k, m)
    x, w, dy = dev(c['x']), dev(c['w']), dev(c['dy'])
    launches = {'fwd': lambda o, acc: ctx.dense_fwd(x, w, o.view(n, m)),
                'dgrad': lambda o, acc: ctx.dense_dgrad(dy, w, o.view(n, k), accumulate=acc),
                'wgrad': lambda o, acc: ctx.dense_wgrad(x, dy, o.view(k, m), accumulate=acc)}
    seed = 0
    for op in ('fwd', 'dgrad', 'wgrad'):
        a, b, base, prod = refs[op]
        for acc in ((False,) if op == 'fwd' else (False, True)):
            seed += 1
            want = prod + base.astype(np.float64) if acc else prod
            st, flat, clone, mask = _window(prod.size, geom, seed, base if acc else None)
            launches[op](flat, acc)
            torch.cuda.synchronize()
            got = flat.cpu().numpy().reshape(prod.shape)
            e = rel(got, want)
            if k <= DENSE_LONG_K:
                bound = DENSE_TOL
            else:
                e_np = rel(BO.dense_f32_sequential(a, b, base if acc else None), want)
                bound = 4 * e_np
                print("(%d, %d, %d) %s accumulate=%s: float32 sequential restatement %.2e  bound %.2e  kernel %.2e"
                      % (n, k, m, op, acc, e_np, bound, e))
            assert np.isfinite(got).all() and e <= bound, (op, acc, e, bound)
            assert_outside_untouched(st, clone, mask)
    assert same_bits(x, c['x']) and same_bits(w, c['w']) and same_bits(dy, c['dy'])


def test_bad_dense_arguments_raise(ctx):
    from elektronn2_amd import backend
    lib = backend.lib()
    import ctypes as C
    t = torch.zeros(64, device="cuda")
    ptr = C.c_void_p(t.data_ptr())
    for n, k, m in ((0, 3, 4), (3, 0, 4), (3, 4, 0), (-1, 3, 4), (3, -2, 4), (3, 4, -5)):
        with pytest.raises(backend.E2Error, match="e2_dense_fwd"):
            backend._chk(lib.e2_dense_fwd(ctx.h, ptr, ptr, ptr, n, k, m), "e2_dense_fwd")
        with pytest.raises(backend.E2Error, match="e2_dense_dgrad"):
            backend._chk(lib.e2_dense_dgrad(ctx.h, ptr, ptr, ptr, n, k, m, 0), "e2_dense_dgrad")
        with pytest.raises(backend.E2Error, match="e2_dense_wgrad"):
            backend._chk(lib.e2_dense_wgrad(ctx.h, ptr, ptr, ptr, n, k, m, 1), "e2_dense_wgrad")
    assert not t.any()


# ---- C. nets ---------------------------------------------------------------------------------------
def check_loss_pred_grads(m, ref, feed, what):
    args = args_of(m, feed)
    lref, pref = ref.loss_and_grads(feed)
    loss = float(m.loss(*args))
    assert abs(loss - lref) / abs(lref) < TOL, (what, loss, lref)
    e = rel(m.predict(feed[m.input_node.name]), pref)
    assert e < TOL, (what, e)
    names = list(m.loss_node.all_trainable_params.keys())
    got, want = m.gradients(*args), ref.grads()
    assert len(got) == len(want) == len(names)
    errs = dict((nme, rel(g, w)) for nme, g, w in zip(names, got, want))
    print("%s: loss %.7f ref %.7f, prediction %.1e, gradients worst %s"
          % (what, loss, lref, e, sorted(errs.items(), key=lambda kv: -kv[1])[:3]))
    for nme, w in zip(names, want):
        assert np.abs(w).max() > 0, nme
        assert errs[nme] < TOL, (what, nme, errs[nme])
    return names


def check_params(m, ref, what):
    """trainable parameters at 5e-4, running statistics at 1e-5 (tests/test_mnist_gpu.py)"""
    worst = ('', 0.0)
    for node in m.nodes.values():
        for k, p in node.params.items():
            if k in ('w', 'b') + BN_KEYS:
                e = rel(p.get_value(), ref.p(p).detach().numpy())
                worst = max(worst, ('%s_%s' % (node.name, k), e), key=lambda kv: kv[1])
                assert e < (1e-5 if k in ('mean', 'std') else 5e-4), (what, node.name, k, e)
    return worst


def steps_against_float64(m, ref, feeds, optimiser='Adam'):
    for step, feed in enumerate(feeds):
        lref = ref.step(feed, optimiser)
        loss = float(m.trainingstep(*args_of(m, feed), optimiser=optimiser)[0])
        assert abs(loss - lref) / abs(lref) < TOL, (step, loss, lref)
        worst = check_params(m, ref, step)
        print("step %d: loss %.7f ref %.7f, parameters worst %s" % (step, loss, lref, worst))


def test_upconv_with_batch_norm_behind_a_pooled_tanh_batch_norm_conv():
    """net 1 at batch 2: loss, prediction, every gradient (eager, captured, replayed), three Adam
    steps with the running statistics of both nodes"""
    name, make, ncls, batch, seed = NETS[0]
    m = make()
    feed = feed_for(m, seed, ncls, batch)
    ref = BnRef(m)
    assert [type(n).__name__ for n in bn_nodes(m)] == ['Conv', 'UpConv']
    before = all_params(m)
    for call in range(3):
        names = check_loss_pred_grads(m, ref, feed, "%s call %d" % (name, call))
    assert 'up_gamma' in names and 'c1_gamma' in names
    after = all_params(m)
    assert all(same_bits(before[k], after[k]) for k in before)        # no step function ran
    steps_against_float64(m, ref, [feed] * 3)
    moved = all_params(m)
    for n in ('c1', 'up'):
        assert not same_bits(moved[n + '_mean'], before[n + '_mean'])
        assert not same_bits(moved[n + '_std'], before[n + '_std'])
    assert m.optimisers['Adam'].step.func.use_graph


def _mnist_sgd(graph):
    from elektronn2_amd import nets, neuromancer as nm
    from elektronn2_amd.neuromancer import plan_options
    with plan_options(graph=graph):
        nm.model_manager.reset()
        np.random.seed(11)
        m = nets.mnist()
        m.set_opt_meta_params('SGD', SGD)
        ref = BnRef(m)
        reg = {k: p.apply_reg for k, p in m.loss_node.all_trainable_params.items()}
        assert reg['conv_gamma'] == 3.0 and reg['conv_w'] is True and reg['conv_b'] is False
        feeds = mnist_batches(4)
        before = all_params(m)
        # loss / prediction / gradient functions leave the running statistics alone
        m.loss(*args_of(m, feeds[0])); m.gradients(*args_of(m, feeds[0])); m.predict(feeds[0]['raw'])
        assert all(same_bits(before[k], v) for k, v in all_params(m).items())
        losses = []
        for step, feed in enumerate(feeds):
            lref = ref.step(feed, 'SGD')
            loss = float(m.trainingstep(*args_of(m, feed), optimiser='SGD')[0])
            assert abs(loss - lref) / abs(lref) < TOL, (graph, step, loss, lref)
            losses.append(loss)
        worst = check_params(m, ref, graph)
        print("SGD, graph=%s: losses %s, parameters worst %s" % (graph, losses, worst))
        assert m.optimisers['SGD'].step.func.use_graph == graph
        after = all_params(m)
        assert not same_bits(after['conv_mean'], before['conv_mean'])
        # gamma's decay is three times a weight's: the decay alone moves it by 3 lr wd gamma a step
        assert rel(after['conv2_gamma'], ref.p(m.nodes['conv2'].gamma).detach().numpy()) < 5e-4
        return losses, after


def test_mnist_net_under_sgd_eager_and_replayed():
    """net 2: four SGD steps (eager, captured, replayed, replayed) on new batches against float64 --
    gamma with 3 x the weight decay, the running statistics moved by the step function only -- and
    the same steps without graphs"""
    res = {g: _mnist_sgd(g) for g in (True, False)}
    for u, v in zip(res[True][0], res[False][0]):
        assert abs(u - v) < 1e-5 * abs(v), (res[True][0], res[False][0])
    for k in res[True][1]:
        assert rel(res[True][1][k], res[False][1][k]) < 1e-4, k


def test_predict_mode_copy_of_a_trained_net():
    """net 3: two Adam steps in train mode, then the same graph in predict mode with w, b, gamma,
    mean, std handed over by value"""
    name, make, ncls, batch, seed = NETS[1]
    a = make()
    feed = feed_for(a, seed, ncls, batch)
    ref_a = BnRef(a)
    steps_against_float64(a, ref_a, [feed] * 2)
    vals = params_by_value(a)
    assert not np.array_equal(vals['c0']['mean'], np.zeros(6, np.float32))      # the statistics moved
    b = net_small('predict', vals)
    ref = BnRef(b)
    x = feed['raw']
    # predict = the float64 forward with the stored statistics
    whole = b.predict(x)
    assert rel(whole, ref.predict(x)) < TOL
    # ... sample by sample: what train mode cannot do
    for i in range(x.shape[0]):
        one = b.predict(x[i:i + 1])
        assert rel(one, ref.predict(x[i:i + 1])) < TOL
        assert np.abs(one - whole[i:i + 1]).max() < 1e-6, i
    assert np.abs(a.predict(x[:1]) - a.predict(x)[:1]).max() > 1e-3
    # gradients: w and b only, the statistics held constant
    names = check_loss_pred_grads(b, ref, feed, "predict-mode copy")
    assert len(names) == 8 and not any(k.endswith(BN_KEYS) for k in names)
    # an Adam step leaves gamma, mean and std bit-identical (and moves the rest)
    before = all_params(b)
    steps_against_float64(b, ref, [feed] * 2)
    after = all_params(b)
    for k in before:
        if k.endswith(BN_KEYS):
            assert same_bits(after[k], before[k]), k
        else:
            assert not same_bits(after[k], before[k]), k


def test_two_perceptron_heads_share_one_trunk_gradient(monkeypatch):
    """net 4: the second e2_dense_dgrad into the trunk's gradient runs with accumulate=True"""
    from elektronn2_amd import backend
    name, make, ncls, batch, seed = NETS[2]
    m = make()
    feed = feed_for(m, seed, ncls, batch)
    ref = BnRef(m)
    for call in range(3):
        names = check_loss_pred_grads(m, ref, feed, "%s call %d" % (name, call))
    assert 'trunk_w' in names and 'head_b_gamma' in names
    # the trunk's output gradient itself: both heads' shares
    plan = m._grad_func.func
    trunk = m.nodes['trunk']
    ref.forward(feed)
    ref.val[trunk].retain_grad()
    for v in ref.P.values():
        v.grad = None
    ref.val[m.loss_node].backward()
    torch.cuda.synchronize()
    got = plan.user_view(trunk, plan.grad[trunk]).cpu().numpy()
    assert rel(got, ref.val[trunk].grad.numpy()) < TOL
    steps_against_float64(m, ref, [feed] * 3)
    # the launches of one eager evaluation: first writer, then adder
    flags = []
    orig = backend.Context.dense_dgrad

    def spy(self, dy, w, dx, accumulate=False):
        flags.append(bool(accumulate))
        return orig(self, dy, w, dx, accumulate=accumulate)
    monkeypatch.setattr(backend.Context, 'dense_dgrad', spy)
    m2 = make()
    got2 = m2.gradients(*args_of(m2, feed))
    monkeypatch.setattr(backend.Context, 'dense_dgrad', orig)
    assert flags == [False, True], flags
    assert len(got2) == len(names)


@pytest.fixture()
def process_bf16():
    import elektronn2_amd
    elektronn2_amd.set_mfma_dtype('bf16')
    yield
    elektronn2_amd.set_mfma_dtype('f32')


def test_bf16_mode_keeps_batch_norm_in_f32_and_feeds_the_next_conv(process_bf16):
    """net 1, local to each layer on the tensors the pass itself produced (bf16 rounding upstream
    does not enter): each batch-norm node's output is the float64 restatement of the `lin` tensor
    its plan holds, at the op bound; the conv behind the UpConv's batch norm computes from that
    output -- conv(bf16(out), bf16(w)) + b, relu at the bf16 layer bound of tests/test_bf16_gpu.py
    (2e-5); three steps stay finite"""
    from test_bf16_gpu import TOL as TOL_BF16, bf16_round
    name, make, ncls, batch, seed = NETS[0]
    m = make()
    feed = feed_for(m, seed, ncls, batch)
    m.gradients(*args_of(m, feed))
    plan = m._grad_func.func
    torch.cuda.synchronize()
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    for node in bn_nodes(m):
        lin = f64(plan.scratch[node, 'lin'])
        r = BO.forward(lin, node.gamma.get_value(), node.b.get_value(), 'lin')
        want = act_f(node.activation_func, r['out'])
        e = chan_err(f64(plan.out[node]), want)
        C = node.n_f
        save = f64(plan.scratch[node, 'bn_save'])
        e_s = max(chan_err(save[:C], r['mean']), chan_err(save[C:], r['std']))
        print("bf16 mode, %s (%s): out %.2e, statistics %.2e" % (node.name, node.activation_func, e, e_s))
        # (2e-5: the bound of the activation op where the node's activation is one, tanh here)
        assert e < (TOL_OUT if node.activation_func in ('relu', 'lin') else 2e-5), (node.name, e)
        assert e_s < TOL_OUT, (node.name, e_s)
        assert np.abs(want).max() > 0.1
    c2, up = m.nodes['c2'], m.nodes['up']
    assert c2.parent is up
    want, _ = O.conv_node_fwd(bf16_round(f64(plan.out[up])), bf16_round(c2.w.get_value()),
                              c2.b.get_value(), (1, 1, 1), 'relu')
    e = rel(f64(plan.out[c2]), want)
    unrounded, _ = O.conv_node_fwd(f64(plan.out[up]), c2.w.get_value(), c2.b.get_value(), (1, 1, 1), 'relu')
    print("bf16 mode, c2 from the UpConv's batch-normalised output: %.2e (unrounded operands %.2e)"
          % (e, rel(f64(plan.out[c2]), unrounded)))
    assert e < TOL_BF16, e
    losses = [float(m.trainingstep(*args_of(m, feed), optimiser='Adam')[0]) for _ in range(3)]
    assert np.isfinite(losses).all()
    for v in all_params(m).values():
        assert np.isfinite(v).all()
