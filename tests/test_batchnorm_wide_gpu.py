"""csrc/bn_wide.hip through the C ABI and through the plan: e2_batchnorm_wide_fwd / _bwd, the batch
normalisation of conv-sized tensors (a channel cut into slabs of whole rows, C x slabs work-groups).

References are float64 and never the code under test: oracle/bn_oracle.py's closed forms on the
planted inputs of tests/test_batchnorm_host.py, and ``BnRef`` for whole steps.  The launches, their
strided views, NULL outputs and the error table are those of tests/test_batchnorm_gpu.py: ``Wide``
gives the new entries the old pair's signature at a fixed ``splits``, so the same ``Launch`` drives both.
Bounds: the project's fixed ones (1e-5 / 2e-5 / 1e-6 per channel) at the shapes where the reference
is shown to meet them; at the two shapes that cross the tiling, 8 x the error against float64 of the
float32 two-pass restatement ``BO.fwd_bwd(dtype=np.float32)``, as
test_batchnorm_gpu.test_offset_input_holds_the_two_pass_bound computes it.
"""
import numpy as np
import pytest
import torch

from oracle import bn_oracle as BO
from test_batchnorm_gpu import (OFFSET_KEYS, Launch, check_loss_pred_grads, errors_of, grad_base, same_bits,
                                steps_against_float64)
from test_batchnorm_host import DYADIC_CH, KINK_GAP, NETS, BnRef, bn_case, bn_ref, chan_err, feed_for

pytestmark = pytest.mark.gpu
KEYS = ('out', 'save', 'run_mean', 'run_std', 'dx', 'dgamma', 'dbias')


class Wide(object):
    """the old pair's signature on the new entries, at a fixed ``splits``"""

    def __init__(self, ctx, splits):
        self.ctx, self.splits = ctx, splits

    def batchnorm_act_fwd(self, *a):
        self.ctx.batchnorm_wide_fwd(*a, splits=self.splits)

    def batchnorm_act_bwd(self, *a):
        self.ctx.batchnorm_wide_bwd(*a, splits=self.splits)


# 24 rows, 1 row, 102 rows: one slab, several, and counts that do not divide the rows
SMALL = [((3, 5, 2, 4, 7), 1), ((3, 5, 2, 4, 7), 5), ((3, 5, 2, 4, 7), 24), ((1, 4, 1, 1, 257), 1),
         ((2, 3, 3, 17, 19), 1), ((2, 3, 3, 17, 19), 4), ((2, 3, 3, 17, 19), 7)]


@pytest.mark.parametrize("train", [True, False], ids=["train", "predict"])
@pytest.mark.parametrize("act", ['relu', 'lin'])
@pytest.mark.parametrize("kind", ['plain', 'corners'])
@pytest.mark.parametrize("shape,splits", SMALL, ids=lambda v: str(v).replace(' ', ''))
def test_closed_forms_at_the_fixed_bounds(ctx, shape, splits, kind, act, train):
    """every output per channel; the += onto a non-zero dgamma / dbias; a second launch gives the
    same bits; the dyadic channel's mean is exactly 0 and `out` exactly 0 at its planted zeros"""
    w = Wide(ctx, splits)
    r, c = bn_ref(shape, kind, act, train), bn_case(shape, kind)
    L = Launch(w, shape, kind, act, train)
    errs = errors_of(L, r, shape, kind, train)
    print(shape, splits, kind, act, train, " ".join("%s %.1e" % (k, v[0]) for k, v in errs.items()))
    for k, (e, bound) in errs.items():
        assert e < bound, (k, e, bound)
    L.check_storage()
    again, Z = Launch(w, shape, kind, act, train), Launch(w, shape, kind, act, train, zero_base=True)
    for k in KEYS:
        assert same_bits(getattr(again, k), getattr(L, k)), k
    dg0, db0 = grad_base(shape[1])
    assert same_bits(L.dgamma, dg0 + Z.dgamma) and same_bits(L.dbias, db0 + Z.dbias)
    assert not same_bits(L.dbias, Z.dbias)
    if kind == 'corners' and train:
        assert L.save[DYADIC_CH] == 0.0
        assert np.all(L.out[:, DYADIC_CH][c['x'][:, DYADIC_CH] == 0] == 0.0)


# every row 16-byte aligned; one slab of six tile trips with a ragged tail and rows of 133
@pytest.mark.parametrize("kind", ['plain', 'offset'])
@pytest.mark.parametrize("splits", [1, 0], ids=["one", "auto"])
@pytest.mark.parametrize("shape", [(2, 2, 2, 5, 64), (1, 2, 4, 40, 133)], ids=lambda v: str(v).replace(' ', ''))
def test_shapes_that_cross_the_tiling_hold_the_two_pass_bound(ctx, shape, splits, kind):
    c, C = bn_case(shape, kind), shape[1]
    r = bn_ref(shape, kind, 'relu', True)
    assert np.abs(r['pre']).min() >= KINK_GAP
    f = BO.fwd_bwd(c['x'], c['gamma'], c['bias'], c['dout'], 'relu', dtype=np.float32)
    f['run_mean'], f['run_std'] = BO.running_update(c['run_mean'], c['run_std'], f['mean'], f['std'], np.float32)
    L = Launch(Wide(ctx, splits), shape, kind, 'relu', True, zero_base=True)
    got = dict(out=L.out, mean=L.save[:C], std=L.save[C:], run_mean=L.run_mean, run_std=L.run_std,
               dx=L.dx, dgamma=L.dgamma, dbias=L.dbias)
    failed = []
    for k in OFFSET_KEYS:
        e_np, e_hip = chan_err(f[k], r[k]), chan_err(got[k], r[k])
        print("%s %s %-8s restatement %.2e  bound %.2e  kernel %.2e" % (shape, kind, k, e_np, 8 * e_np, e_hip))
        if not e_hip <= 8 * e_np:
            failed.append((k, e_hip, 8 * e_np))
    assert not failed, failed
    L.check_storage()


@pytest.mark.parametrize("act,train", [('relu', True), ('lin', False)], ids=["relu-train", "lin-predict"])
@pytest.mark.parametrize("geom", ["cslice_frame", "odd_base"])
def test_strided_views_give_the_dense_bits_and_touch_nothing_else(ctx, geom, act, train):
    shape, w = (2, 3, 3, 17, 19), Wide(ctx, 4)
    D = Launch(w, shape, 'corners', act, train)
    L = Launch(w, shape, 'corners', act, train, geom=geom, views=('x', 'out', 'dout', 'dx'))
    for k in KEYS:
        assert same_bits(getattr(L, k), getattr(D, k)), k
    L.check_storage()                  # nothing outside the views; x and dout only read


@pytest.mark.parametrize("train", [True, False], ids=["train", "predict"])
@pytest.mark.parametrize("skip", ['dgamma', 'dbias', 'dx'])
def test_null_gradient_outputs_leave_the_others_to_the_bit(ctx, skip, train):
    shape, w = (2, 3, 3, 17, 19), Wide(ctx, 4)
    L = Launch(w, shape, 'corners', 'relu', train)
    N = Launch(w, shape, 'corners', 'relu', train, skip=(skip,))
    assert getattr(N, skip) is None
    for k in KEYS:
        if k != skip:
            assert same_bits(getattr(N, k), getattr(L, k)), k


def test_bad_arguments_raise(ctx):
    from elektronn2_amd import backend
    sh = (2, 3, 1, 4, 5)                                       # 8 rows
    x, out, other = (torch.zeros(s, device="cuda") for s in (sh, sh, (2, 3, 1, 4, 6)))
    v, save = torch.ones(3, device="cuda"), torch.zeros(6, device="cuda")
    short = torch.zeros(2, device="cuda")
    fwd, bwd = ctx.batchnorm_wide_fwd, ctx.batchnorm_wide_bwd
    bad_fwd = [lambda: fwd(x, v, v, v, v, True, True, 'relu', out, save, ws=short),
               lambda: fwd(x, v, v, v, v, True, True, 'relu', out, save, splits=9),
               lambda: fwd(x, v, v, v, v, True, True, 'relu', other, save),
               lambda: fwd(x, v, v, v, v, True, True, 'tanh', out, save),
               lambda: fwd(x, v, v, None, None, False, False, 'relu', out, save)]
    bad_bwd = [lambda: bwd(x, x, v, v, save, True, 'relu', out, v, v, ws=short),
               lambda: bwd(x, x, v, v, save, True, 'relu', out, v, v, splits=9),
               lambda: bwd(other, x, v, v, save, True, 'relu', out, v, v),
               lambda: bwd(x, x, v, v, save, True, 'relu', other, v, v),
               lambda: bwd(x, x, v, v, save, True, 'tanh', out, v, v)]
    for calls, name in ((bad_fwd, "e2_batchnorm_wide_fwd"), (bad_bwd, "e2_batchnorm_wide_bwd")):
        for call in calls:
            with pytest.raises(backend.E2Error, match=name):
                call()
    torch.cuda.synchronize()
    assert not out.any() and not short.any()


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "old"])
def test_net_with_batch_norm_in_conv_and_upconv_on_the_chosen_route(monkeypatch, wide):
    """net 1 at batch 2 against the float64 step: loss, prediction and gradients (eager, captured,
    replayed), three Adam steps with the running statistics; the Context methods the plan called"""
    from elektronn2_amd import backend
    from elektronn2_amd.neuromancer import plan_options
    calls = set()
    for name in ('batchnorm_act_fwd', 'batchnorm_act_bwd', 'batchnorm_wide_fwd', 'batchnorm_wide_bwd'):
        def spy(self, *a, _orig=getattr(backend.Context, name), _name=name, **kw):
            calls.add(_name)
            return _orig(self, *a, **kw)
        monkeypatch.setattr(backend.Context, name, spy)
    name, make, ncls, batch, seed = NETS[0]
    with plan_options(bn_wide=wide):
        m = make()
        feed, ref = feed_for(m, seed, ncls, batch), BnRef(m)
        for call in range(3):
            check_loss_pred_grads(m, ref, feed, "%s call %d" % (name, call))
        steps_against_float64(m, ref, [feed] * 3)
        assert m.optimisers['Adam'].step.func.use_graph
    route = 'wide' if wide else 'act'
    assert calls == {'batchnorm_%s_fwd' % route, 'batchnorm_%s_bwd' % route}, calls
