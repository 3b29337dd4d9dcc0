"""Batch normalisation and the Perceptron, host side (no GPU): what tests/test_batchnorm_gpu.py
stands on.

  1. oracle/bn_oracle.py -- the float64 closed forms of e2_batchnorm_act_fwd / _bwd in train and
     predict mode -- against torch float64 autograd of oracle/mnist_oracle.py's ``batchnorm`` +
     ``relu``, and the forward against a plain loop over channels.
  2. The inputs the GPU op tests plant do what they are planted for: the dyadic-symmetric channel
     has a mean of exactly 0.0 in float32 and float64 (so exact-zero pre-activations exist), the
     constant channel has variance exactly 0, no other relu unit sits within 1e-5 of its kink, no
     per-channel reference is a heavily cancelled sum, and the offset input 30 + 0.25 randn
     separates a float32 two-pass restatement of the statistics from a one-pass E[x^2] - mean^2 by
     far more than the factor 8 the GPU bound allows.
  3. ``BnRef``, the float64 restatement of whole graphs with batch normalisation in Conv / UpConv /
     Perceptron (both modes), several Perceptron heads and SquaredLoss terms, and the nets of the
     GPU file; every evaluation the GPU tests make is well-posed on the reference.
"""
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import bn_oracle as BO
from oracle import e2_oracle as O
from oracle import mnist_oracle as MO
from test_conv_modes_host import MIN_PRE, Ref, conv_ref
from test_regression_loss_host import ref_aggregate, ref_squared

# ---- the op cases ------------------------------------------------------------------------------
# S = 56, 257, 969, 1, 1: under one trip, one trip + 1, several trips with a ragged tail of the
# kernels' `for (s = threadIdx.x; s < S; s += 256)`; n = 1; many channels of 20 elements; cnt = 1
BN_SHAPES = [(3, 5, 2, 4, 7), (1, 4, 1, 1, 257), (2, 3, 3, 17, 19), (20, 200, 1, 1, 1), (1, 1, 1, 1, 1)]
AUTOGRAD_SHAPES = [(3, 5, 2, 4, 7), (1, 4, 1, 1, 257), (20, 200, 1, 1, 1)]
CORNER_SHAPES = [(3, 5, 2, 4, 7), (1, 4, 1, 1, 257), (2, 3, 3, 17, 19)]      # C >= 3, S > 1
OFFSET_SHAPES = [(3, 5, 2, 4, 7), (2, 3, 3, 17, 19)]
DYADIC_CH, CONST_CH, CONST_VALUE = 0, 1, 2.5
# the bounds of the op test this file's GPU twin took over from tests/test_mnist_gpu.py
TOL_OUT, TOL_GRAD, TOL_RUN_STD = 1e-5, 2e-5, 1e-6
# Where a channel's reference is EXACTLY 0 (the mean of the dyadic channel, dgamma and dx of a
# constant channel, every gradient of a channel whose relu is shut) there is no magnitude to
# divide by: the error is taken against 1.0, the scale of the inputs (x, dout, gamma = O(1)).
ABS_FLOOR = 1.0
KINK_GAP = 1e-5           # no unplanted relu pre-activation closer to 0 than this
MAX_CANCEL = 16.0         # sum |terms| / |sum terms| of every per-channel reference


# cases whose first draw put an unplanted relu unit within KINK_GAP of its kink (decided on the
# float64 reference: test_no_unplanted_relu_unit_sits_at_its_kink), drawn again
RESEED = {((2, 3, 3, 17, 19), 'corners'): (1,)}


def chan_err(got, ref):
    """max over channels of max |got_c - ref_c| / max |ref_c| (ABS_FLOOR where ref_c is all 0);
    (C,) vectors, (2C,) ``save`` as two vectors, or (n, C, ...) tensors"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.ndim == 1:
        got, ref = got[None, :, None], ref[None, :, None]
    g = np.moveaxis(got, 1, 0).reshape(got.shape[1], -1)
    r = np.moveaxis(ref, 1, 0).reshape(ref.shape[1], -1)
    mag = np.abs(r).max(axis=1)
    mag = np.where(mag == 0, ABS_FLOOR, mag)
    err = np.abs(g - r).max(axis=1) / mag
    return float(np.where(np.isfinite(err), err, np.inf).max())


def dyadic_symmetric(cnt, rng):
    """``cnt`` multiples of 1/4 in [-3, 3]: every value with its negative, at least cnt // 8 (and
    at least 2) exact zeros, in random order.  Every partial sum in any order is a multiple of
    1/4 far below 2^24 / 4, so float32 adds them without rounding: the sum is exactly 0."""
    n_zero = max(2, cnt // 8)
    n_zero += (cnt - n_zero) % 2
    half = rng.randint(1, 13, (cnt - n_zero) // 2).astype(np.float32) / np.float32(4)
    v = np.concatenate([half, -half, np.zeros(n_zero, np.float32)])
    return v[rng.permutation(cnt)]


@functools.lru_cache(maxsize=None)
def bn_case(shape, kind='plain'):
    """float32 inputs of one op case, made once, shared, read-only: x, gamma, bias, dout, run_mean,
    run_std.  'plain': x = 3 + 2 randn; 'corners': the same with channel 0 dyadic-symmetric with
    planted zeros under bias 0 and channel 1 constant; 'offset': x = 30 + 0.25 randn.
    dout = 3 + 2 xhat + 0.5 randn, so that neither dbias = sum dpre nor dgamma = sum dpre xhat
    cancels (test_no_per_channel_reference_is_a_cancelled_sum)."""
    rng = np.random.RandomState(zlib.crc32(repr((shape, kind) + RESEED.get((shape, kind), ())).encode()))
    n, C = shape[:2]
    cnt = int(np.prod(shape)) // C
    z = rng.randn(*shape)
    x = (30 + 0.25 * z if kind == 'offset' else 3 + 2 * z).astype(np.float32)
    gamma = (rng.rand(C) + 0.5).astype(np.float32)
    bias = (0.3 * rng.randn(C)).astype(np.float32)
    if kind == 'corners':
        assert shape in CORNER_SHAPES
        x[:, DYADIC_CH] = dyadic_symmetric(cnt, rng).reshape((n,) + shape[2:])
        bias[DYADIC_CH] = 0.0
        x[:, CONST_CH] = CONST_VALUE
    x64 = x.astype(np.float64)
    mean, s0, _ = BO.batch_stats(x64)
    sh = (1, C) + (1,) * (len(shape) - 2)
    xhat = (x64 - mean.reshape(sh)) / np.where(s0 > 0, s0, 1.0).reshape(sh)
    dout = (3 + 2 * xhat + 0.5 * rng.randn(*shape)).astype(np.float32)
    case = dict(x=x, gamma=gamma, bias=bias, dout=dout,
                run_mean=rng.randn(C).astype(np.float32),
                run_std=(rng.rand(C) + 0.5).astype(np.float32))
    for a in case.values():
        a.setflags(write=False)
    return case


def all_cases():
    return ([(s, 'plain') for s in BN_SHAPES] + [(s, 'corners') for s in CORNER_SHAPES]
            + [(s, 'offset') for s in OFFSET_SHAPES])


@functools.lru_cache(maxsize=None)
def bn_ref(shape, kind, act, train):
    """the float64 closed forms of one case: BO.fwd_bwd plus the running statistics after one
    update (train) -- predict mode applies the case's run_mean / run_std"""
    c = bn_case(shape, kind)
    stats = None if train else (c['run_mean'], c['run_std'])
    r = BO.fwd_bwd(c['x'], c['gamma'], c['bias'], c['dout'], act, stats)
    if train:
        r['run_mean'], r['run_std'] = BO.running_update(c['run_mean'], c['run_std'], r['mean'], r['std'])
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


# ---- the dense cases ---------------------------------------------------------------------------
DENSE_SHAPES = [(1, 1, 1), (1, 300, 1), (3, 1, 257), (20, 57, 33), (20, 576, 200), (20, 200, 10),
                (2, 513, 5)]
DENSE_TOL, DENSE_LONG_K = 2e-6, 57


@functools.lru_cache(maxsize=None)
def dense_case(n, k, m):
    rng = np.random.RandomState(zlib.crc32(repr((n, k, m)).encode()))
    case = dict(x=rng.randn(n, k), w=rng.randn(k, m), dy=rng.randn(n, m), dx0=rng.randn(n, k),
                dw0=rng.randn(k, m))
    case = dict((key, v.astype(np.float32)) for key, v in case.items())
    for a in case.values():
        a.setflags(write=False)
    return case


def dense_refs(n, k, m):
    """op -> (a, b, base, float64 product): fwd y = x w, dgrad dx = dy w^T, wgrad dw = x^T dy"""
    c = dense_case(n, k, m)
    f = lambda a: a.astype(np.float64)
    return dict(fwd=(c['x'], c['w'], None, f(c['x']) @ f(c['w'])),
                dgrad=(c['dy'], np.ascontiguousarray(c['w'].T), c['dx0'], f(c['dy']) @ f(c['w']).T),
                wgrad=(np.ascontiguousarray(c['x'].T), c['dy'], c['dw0'], f(c['x']).T @ f(c['dy'])))


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---- 1. the closed forms -----------------------------------------------------------------------
def _autograd(case, act, train, keep=None):
    """(out, mean, std, dx, dgamma, dbias) by torch float64 autograd of MO.batchnorm / MO.relu"""
    t = lambda a, g=True: torch.tensor(np.asarray(a, np.float64), requires_grad=g)
    X, G, B = t(case['x']), t(case['gamma']), t(case['bias'])
    if train:
        y, mean, std = MO.batchnorm(X, G, B)
    else:
        mean, std = t(case['run_mean'], False), t(case['run_std'], False)
        sh = (1, -1) + (1,) * (X.dim() - 2)
        y = (G / std).view(sh) * X + (B - G * mean / std).view(sh)
    out = MO.relu(y) if act == 'relu' else y
    (out * t(case['dout'], False)).sum().backward()
    return [v.detach().numpy() for v in (out, mean, std)] + [X.grad.numpy(), G.grad.numpy(), B.grad.numpy()]


@pytest.mark.parametrize("train", [True, False], ids=["train", "predict"])
@pytest.mark.parametrize("act", ['relu', 'lin'])
@pytest.mark.parametrize("shape", AUTOGRAD_SHAPES, ids=str)
def test_closed_forms_equal_autograd(shape, act, train):
    for kind in ('plain', 'corners'):
        if kind == 'corners' and shape not in CORNER_SHAPES:
            continue
        case = bn_case(shape, kind)
        r = bn_ref(shape, kind, act, train)
        want = _autograd(case, act, train)
        keep = np.ones(shape[1], bool)
        if kind == 'corners' and train:
            keep[CONST_CH] = False        # (autograd's 0 * inf there; the rule is the project's)
            assert not np.isfinite(want[3][:, CONST_CH]).all()
        for name, w in zip(('out', 'mean', 'std', 'dx', 'dgamma', 'dbias'), want):
            g = r[name]
            g, w = (g[:, keep], w[:, keep]) if g.ndim > 1 else (g[keep], w[keep])
            assert chan_err(g, w) < 1e-9, (kind, name, chan_err(g, w))
        assert np.array_equal(r['save'], np.concatenate([r['mean'], r['std']]))


def test_forward_equals_a_plain_loop_over_channels():
    shape = (3, 5, 2, 4, 7)
    for kind in ('plain', 'corners'):
        c = bn_case(shape, kind)
        for act in ('relu', 'lin'):
            out, mean, std = BO.numpy_loop_forward(c['x'], c['gamma'], c['bias'], act)
            r = bn_ref(shape, kind, act, True)
            assert chan_err(r['mean'], mean) < 1e-12 and chan_err(r['std'], std) < 1e-12
            assert np.abs(r['out'] - out).max() < 1e-9       # (1e6 * 1e-16 in the constant channel)


def test_running_update_and_predict_mode_are_the_stated_formulas():
    shape = (3, 5, 2, 4, 7)
    c, r = bn_case(shape), bn_ref(shape, 'plain', 'relu', True)
    assert np.allclose(r['run_mean'], 0.9995 * c['run_mean'].astype(np.float64) + 0.0005 * r['mean'], rtol=1e-15)
    assert np.allclose(r['run_std'], 0.9995 * c['run_std'].astype(np.float64) + 0.0005 * r['std'], rtol=1e-15)
    assert np.all(r['std'] - r['s0'] == pytest.approx(1e-6, rel=1e-6))         # std INCLUDES the 1e-6
    p = bn_ref(shape, 'plain', 'lin', False)
    assert np.array_equal(p['mean'], c['run_mean'].astype(np.float64))
    a = (c['gamma'].astype(np.float64) / c['run_std']).reshape(1, -1, 1, 1, 1)
    assert np.allclose(p['dx'], a * c['dout'], rtol=1e-15)                     # statistics are constants


# ---- 2. the planted inputs ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", CORNER_SHAPES, ids=str)
def test_planted_channels_do_what_they_are_planted_for(shape):
    c = bn_case(shape, 'corners')
    x = c['x']
    for dtype in (np.float32, np.float64):
        mean, s0, std = BO.batch_stats(x, dtype)
        assert mean.dtype == dtype
        assert mean[DYADIC_CH] == 0.0 and s0[DYADIC_CH] > 0.5          # exactly 0, either precision
        assert mean[CONST_CH] == dtype(CONST_VALUE) and s0[CONST_CH] == 0.0     # variance exactly 0
        # in any order: a sequential sum and a reversed one
        ch = x[:, DYADIC_CH].ravel().astype(dtype)
        assert np.cumsum(ch)[-1] == 0.0 and np.cumsum(ch[::-1])[-1] == 0.0
    zeros = x[:, DYADIC_CH] == 0
    assert zeros.sum() >= 2 and c['bias'][DYADIC_CH] == 0.0
    r = bn_ref(shape, 'corners', 'relu', True)
    assert np.all(r['pre'][:, DYADIC_CH][zeros] == 0.0)                # exact-zero pre-activations
    # ... where relu'(0) = 0.5 matters: a slope of 0 or 1 there moves dx far beyond the bound
    for slope in (0.0, 1.0):
        dpre = c['dout'].astype(np.float64) * np.where(r['pre'] > 0, 1.0, np.where(r['pre'] == 0, slope, 0.0))
        dbias = dpre.sum(axis=(0, 2, 3, 4))
        assert abs(dbias[DYADIC_CH] - r['dbias'][DYADIC_CH]) > 1e3 * TOL_GRAD * abs(r['dbias'][DYADIC_CH])
    # the constant channel: everything finite, the output is act(bias), dgamma 0
    for act in ('relu', 'lin'):
        rc = bn_ref(shape, 'corners', act, True)
        assert all(np.isfinite(rc[k]).all() for k in ('out', 'dx', 'dgamma', 'dbias', 'std'))
        assert rc['std'][CONST_CH] == 1e-6 and rc['dgamma'][CONST_CH] == 0.0
        want = c['bias'][CONST_CH] if act == 'lin' else max(c['bias'][CONST_CH], 0)
        assert np.abs(rc['out'][:, CONST_CH] - want).max() < 1e-8
        if act == 'lin':
            assert np.abs(rc['dx'][:, CONST_CH]).max() > 1e3           # (gamma / 1e-6) * (d - mean(d))


def test_a_single_element_channel_is_a_constant_channel():
    r = bn_ref((1, 1, 1, 1, 1), 'plain', 'relu', True)
    assert r['s0'][0] == 0.0 and r['std'][0] == 1e-6 and r['dx'].ravel()[0] == 0.0 and r['dgamma'][0] == 0.0


@pytest.mark.parametrize("shape,kind", all_cases(), ids=lambda v: str(v))
def test_no_unplanted_relu_unit_sits_at_its_kink(shape, kind):
    """float32 and float64 must take the same slope everywhere but at the planted zeros"""
    c = bn_case(shape, kind)
    for train in (True, False):
        pre = np.abs(bn_ref(shape, kind, 'relu', train)['pre']).copy()
        if kind == 'corners' and train:
            pre[:, DYADIC_CH][c['x'][:, DYADIC_CH] == 0] = np.inf
        assert pre.min() >= KINK_GAP, (shape, kind, train, pre.min())


@pytest.mark.parametrize("shape,kind", all_cases(), ids=lambda v: str(v))
def test_no_per_channel_reference_is_a_cancelled_sum(shape, kind):
    """mean, dbias and dgamma are sums; relative to a sum that cancels, float32 has no accuracy to
    be held to.  Every one is exactly 0 or at least 1 / MAX_CANCEL of the sum of its terms'
    magnitudes -- in train mode; in predict mode, where xhat is taken from unrelated stored
    statistics, for dbias."""
    c = bn_case(shape, kind)
    red = (0, 2, 3, 4)
    x = c['x'].astype(np.float64)
    worst = 0.0
    for act in ('relu', 'lin'):
        for train in (True, False):
            r = bn_ref(shape, kind, act, train)
            sh = (1, -1, 1, 1, 1)
            dpre = c['dout'].astype(np.float64) * BO.act_slope(r['pre'], act)
            xhat = (x - r['mean'].reshape(sh)) / r['std'].reshape(sh)
            cnt = x.size // x.shape[1]
            sums = [(r['dbias'], dpre)] + ([(r['mean'] * cnt, x), (r['dgamma'], dpre * xhat)] if train else [])
            for total, terms in sums:
                mag = np.abs(terms).sum(axis=red)
                live = total != 0
                worst = max(worst, float((mag[live] / np.abs(total[live])).max()) if live.any() else 0.0)
    assert worst <= MAX_CANCEL, worst


@pytest.mark.parametrize("shape", OFFSET_SHAPES, ids=str)
def test_offset_input_separates_two_pass_from_one_pass_statistics(shape):
    """x = 30 + 0.25 randn: E[x^2] - mean^2 loses log2(30^2 / 0.25^2) = 14 of float32's 24 bits.
    The GPU test bounds the kernel's statistics by 8 times the two-pass float32 error; a one-pass
    form has to miss that bound: the separation asserted here is 30 times."""
    x = bn_case(shape, 'offset')['x']
    _, _, std = BO.batch_stats(x)
    two = np.abs(BO.batch_stats(x, np.float32)[2] - std) / std
    one = np.abs(BO.batch_stats(x, np.float32, one_pass=True)[2] - std) / std
    print(shape, "std, relative to float64: two-pass %.2e, one-pass %.2e (x %.0f)"
          % (two.max(), one.max(), one.max() / two.max()))
    assert two.max() < 1e-6
    assert one.max() >= 30 * two.max()
    # ... and with it everything downstream: the one-pass restatement misses 8 x the two-pass error
    c = bn_case(shape, 'offset')
    ref = bn_ref(shape, 'offset', 'relu', True)
    r2 = BO.fwd_bwd(c['x'], c['gamma'], c['bias'], c['dout'], 'relu', dtype=np.float32)
    r1 = BO.fwd_bwd(c['x'], c['gamma'], c['bias'], c['dout'], 'relu', dtype=np.float32, one_pass=True)
    for key in ('out', 'dx'):
        assert chan_err(r1[key], ref[key]) > 8 * chan_err(r2[key], ref[key]), key


def test_sequential_float32_sums_are_what_they_claim():
    rng = np.random.RandomState(1)
    a, b = rng.randint(-8, 9, (3, 40)).astype(np.float32), rng.randint(-8, 9, (40, 5)).astype(np.float32)
    assert np.array_equal(BO.dense_f32_sequential(a, b), a.astype(np.float64) @ b)        # exact ints
    a, b = rng.randn(4, 300).astype(np.float32), rng.randn(300, 6).astype(np.float32)
    got, want = BO.dense_f32_sequential(a, b), a.astype(np.float64) @ b
    assert got.dtype == np.float32 and 0 < rel(got, want) < 300 * 2.0 ** -24
    acc = np.float32(0)
    for t in range(300):                                      # one element, by hand
        acc = np.float32(np.float64(a[1, t]) * np.float64(b[t, 2]) + np.float64(acc))
    assert got[1, 2] == acc
    base = rng.randn(4, 6).astype(np.float32)
    assert np.array_equal(BO.dense_f32_sequential(a, b, base), base + got)


# ---- 3. whole graphs ---------------------------------------------------------------------------
ADAM = dict(lr=2e-4, mom=0.9, beta2=0.99, wd=0.5e-3)            # examples/mnist.py:18-23
SGD = dict(lr=1e-3, mom=0.9, wd=0.5e-3)
BN_KEYS = ('gamma', 'mean', 'std')


def bn_nodes(m):
    return [n for n in m.nodes.values() if getattr(n, 'batch_normalisation', False)]


class BnRef(Ref):
    """``Ref`` of tests/test_conv_modes_host.py (parameters as float64 leaves, ``adam``, ``grads``)
    with batch normalisation in Conv, UpConv and Perceptron -- 'train' through
    mnist_oracle.batchnorm, 'predict' with the stored statistics as constants --, Perceptrons,
    several inputs (``feed``: {input name: array}), SquaredLoss terms under an AggregateLoss, the
    running statistics as the step functions move them, and SGD (optimiser.py:146-160).  Keeps the
    value of every node (``val``), the tensor each batch norm normalised (``lin``) and its
    statistics (``stats``)."""

    def forward(self, feed, upto=None):
        m = self.model
        if not isinstance(feed, dict):
            feed = {m.input_node.name: feed}
        self.min_pre = np.inf
        val, self.lin, self.stats = {}, {}, {}
        self.val = val
        for node in m.nodes.values():
            kind = type(node).__name__
            par = node.parent
            if kind == 'Input':
                if node.name in feed:
                    val[node] = torch.tensor(np.asarray(feed[node.name], np.float64))
                continue
            if isinstance(par, (list, tuple)) and any(q not in val for q in par) or \
                    (not isinstance(par, (list, tuple)) and par not in val):
                continue                                     # (a loss without its target)
            if kind in ('Conv', 'UpConv', 'Perceptron'):
                h, w, b = val[par], self.p(node.w), self.p(node.b)
                if kind == 'Perceptron':
                    y = (h.flatten(1) if node.flatten else h) @ w
                elif kind == 'UpConv':
                    y = F.conv_transpose3d(h, w.permute(1, 0, 2, 3, 4), stride=tuple(node.pool_shape))
                else:
                    y = conv_ref(h, w, node.conv_mode)
                    if any(q != 1 for q in node.pool_shape):
                        y = (F.max_pool3d if h.dim() == 5 else F.max_pool2d)(y, tuple(node.pool_shape))
                bsh = (1, -1) + (1,) * (y.dim() - 2)
                bn = node.batch_normalisation
                if bn == 'train':
                    self.lin[node] = y
                    y, mean, std = MO.batchnorm(y, self.p(node.gamma), b)
                    self.stats[node] = (mean.detach(), std.detach())
                elif bn == 'predict':
                    self.lin[node] = y
                    g, mu, sd = self.p(node.gamma), self.p(node.mean), self.p(node.std)
                    y = (g / sd).view(bsh) * y + (b - g * mu / sd).view(bsh)
                else:
                    assert not bn
                    y = y + b.view(bsh)
                val[node] = self.act(node, y)
            elif kind == 'Softmax':
                val[node] = torch.softmax(val[par], dim=1)
            elif kind == 'MultinoulliNLL':
                val[node] = MO.nll(val[par[0].parent], val[par[1]])[0] if val[par[0]].dim() == 2 \
                    else self._nll5(val[par[0]], val[par[1]])
            elif kind == 'SquaredLoss':
                assert node.margin is None and node.scale_correction is None
                val[node] = ref_squared(val[par[0]], val[par[1]])
            elif kind == 'AggregateLoss':
                ps = list(par) if isinstance(par, (list, tuple)) else [par]
                if node.elementwise:
                    w = np.asarray(node.mixing_weights.get_value(), np.float32).astype(np.float64)
                    val[node] = ref_aggregate([val[q] for q in ps], w)
                else:
                    val[node] = val[ps[0]].mean()
            elif kind in ('Errors', 'Classification'):
                continue
            else:
                raise NotImplementedError(kind)
            if upto is not None and node is upto:
                return val[node]
        return val.get(m.loss_node), val[m.prediction_node]

    @staticmethod
    def _nll5(pr, tg):
        C = pr.shape[1]
        classes = torch.arange(C, dtype=tg.dtype).view((1, C) + (1,) * (pr.dim() - 2))
        onehot = (tg == classes).to(pr.dtype)
        nll = -(onehot * torch.log(pr + 1e-5)) * pr.numel() / (onehot.sum() + 1e-5) / C
        return nll.sum(dim=1, keepdim=True)

    def loss_and_grads(self, feed):
        for v in self.P.values():
            v.grad = None
        loss, pred = self.forward(feed)
        assert self.min_pre >= MIN_PRE, "ill-posed case: a kinked unit at %.1e" % (self.min_pre,)
        loss.backward()
        return float(loss.detach()), pred.detach().numpy()

    def predict(self, x):
        with torch.no_grad():
            return self.forward(x)[1].numpy()

    @torch.no_grad()
    def move_running_statistics(self):
        """the extra updates of a step function, from the statistics of the last forward"""
        for node, (mean, std) in self.stats.items():
            rm, rs = self.p(node.mean), self.p(node.std)
            rm.copy_(0.9995 * rm + 0.0005 * mean)
            rs.copy_(0.9995 * rs + 0.0005 * std)

    @torch.no_grad()
    def sgd(self, lr, mom, wd):
        for par in self.model.trainable_params:
            p = self.p(par)
            d = self.m.setdefault(id(par), torch.zeros_like(p))
            new_p, new_d = O.sgd_step(p.numpy(), p.grad.numpy(), d.numpy(), lr, mom, wd, par.apply_reg)
            d.copy_(torch.tensor(new_d)); p.copy_(torch.tensor(new_p))

    def step(self, feed, optimiser='Adam', hyper=None):
        """one optimiser iteration as Model.trainingstep runs it; returns the loss before it"""
        loss, _ = self.loss_and_grads(feed)
        if optimiser == 'Adam':
            self.adam(**(hyper or ADAM))
        else:
            self.sgd(**(hyper or SGD))
        self.move_running_statistics()
        return loss


def _nm(seed):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    return nm


def _finish_nll(nm, inp, logits):
    probs = nm.Softmax(logits)
    target = nm.Input_like(probs, override_f=1, name='target')
    loss = nm.AggregateLoss(nm.MultinoulliNLL(probs, target, target_is_sparse=True), name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=probs,
                          prediction_ext=[loss, probs])
    model.set_opt_meta_params('Adam', ADAM)
    return model


def net_upconv(batch=2, seed=81):
    """net 1: relu Conv -> tanh Conv with pooling and batch norm -> relu UpConv with batch norm
    -> relu Conv -> (1,1,1) 'lin' head"""
    nm = _nm(seed)
    inp = nm.Input((batch, 1, 6, 22, 22), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 6, (1, 3, 3), name='c0')                                       # (6, 20, 20)
    out = nm.Conv(out, 8, (3, 3, 3), (1, 2, 2), activation_func='tanh',
                  batch_normalisation='train', name='c1')                             # (4, 9, 9)
    out = nm.UpConv(out, 6, (1, 2, 2), batch_normalisation='train', name='up')        # (4, 18, 18)
    out = nm.Conv(out, 8, (1, 3, 3), name='c2')                                       # (4, 16, 16)
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin', name='head')
    return _finish_nll(nm, inp, out)


def net_small(mode='train', params=None, seed=82):
    """net 3: two 2-D convs (the first pooled) and a Perceptron, all batch-normalised in ``mode``,
    and a 'lin' Perceptron head; ``params``: {node name: {w, b, gamma, mean, std}} by value"""
    nm = _nm(seed)
    kw = lambda name: dict(batch_normalisation=mode, name=name, **(params[name] if params else {}))
    inp = nm.Input((None, 1, 14, 14), 'b,f,y,x', name='raw')
    out = nm.Conv(inp, 6, (3, 3), (2, 2), **kw('c0'))                                 # (6, 6)
    out = nm.Conv(out, 8, (3, 3), **kw('c1'))                                         # (4, 4)
    out = nm.Perceptron(out, 16, flatten=True, **kw('d0'))
    head = dict(w=params['head']['w'], b=params['head']['b']) if params else {}
    out = nm.Perceptron(out, 5, activation_func='lin', name='head', **head)
    return _finish_nll(nm, inp, out)


def params_by_value(m):
    return dict((n.name, dict((k, p.get_value().copy()) for k, p in n.params.items()
                              if k in ('w', 'b') + BN_KEYS))
                for n in m.nodes.values() if 'w' in n.params)


def net_two_heads(batch=4, seed=83):
    """net 4: one pooled 2-D conv, two Perceptron heads on its flattened output (the second
    batch-normalised), a SquaredLoss on each under one AggregateLoss"""
    nm = _nm(seed)
    inp = nm.Input((batch, 1, 12, 12), 'b,f,y,x', name='raw')
    trunk = nm.Conv(inp, 6, (3, 3), (2, 2), name='trunk')                             # (5, 5)
    a = nm.Perceptron(trunk, 4, activation_func='lin', flatten=True, name='head_a')
    b = nm.Perceptron(trunk, 3, activation_func='tanh', flatten=True, batch_normalisation='train',
                      name='head_b')
    ta, tb = nm.Input_like(a, name='target'), nm.Input_like(b, name='target_b')
    loss = nm.AggregateLoss([nm.SquaredLoss(a, ta), nm.SquaredLoss(b, tb)], mixing_weights=[1.0, 0.5],
                            name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=ta, loss_node=loss, prediction_node=a)
    model.set_opt_meta_params('Adam', ADAM)
    return model


def feed_for(m, seed, n_class=2, batch=None):
    """{input name: float32 array}: images in [0, 1), class ids, regression targets ~ N(0, 1)"""
    rng = np.random.RandomState(seed)
    feed = {}
    for n in m.loss_node.input_nodes:
        sh = tuple((batch if s is None else s) for s in n.shape.shape)
        if n is m.input_node:
            a = rng.rand(*sh)
        elif any(type(c).__name__ == 'MultinoulliNLL' for c in n.children.values()):
            a = rng.randint(0, n_class, sh)
        else:
            a = rng.randn(*sh)
        feed[n.name] = a.astype(np.float32)
    return feed


def args_of(m, feed):
    return [feed[n.name] for n in m.loss_node.input_nodes]


# name, constructor, classes, batch for a None axis, seed of the data (chosen on the reference
# alone: MIN_PRE holds over every evaluation the GPU tests make)
NETS = [("upconv", net_upconv, 2, None, 93), ("small", net_small, 5, 3, 92),
        ("two_heads", net_two_heads, 0, None, 93)]


@pytest.mark.parametrize("name,make,ncls,batch,seed", NETS, ids=[n[0] for n in NETS])
def test_restated_nets_run_on_the_cpu(name, make, ncls, batch, seed):
    m = make()
    feed = feed_for(m, seed, ncls, batch)
    ref = BnRef(m)
    before = dict((n, (ref.p(n.mean).clone(), ref.p(n.std).clone())) for n in bn_nodes(m))
    assert before
    for step in range(4):
        loss = ref.step(feed)
        assert np.isfinite(loss)
        assert all(np.abs(g).max() > 0 for g in ref.grads())
    for n, (mu, sd) in before.items():
        assert not torch.equal(ref.p(n.mean), mu) and not torch.equal(ref.p(n.std), sd)
        assert n.gamma.apply_train and n.gamma.apply_reg == 3.0


def mnist_batches(k, seed=2):
    rng = np.random.RandomState(seed)
    return [{'raw': rng.rand(20, 1, 26, 26).astype(np.float32),
             'target': rng.randint(0, 10, (20, 1)).astype(np.float32)} for _ in range(k)]


def test_mnist_net_under_sgd_is_well_posed():
    from elektronn2_amd import nets
    _nm(11)
    m = nets.mnist()
    ref = BnRef(m)
    for feed in mnist_batches(4):
        assert np.isfinite(ref.step(feed, 'SGD'))
    # the restatement is mnist_oracle's: the same loss on the same parameters
    P = dict(('%s_%s' % (n.name, k), ref.p(p).detach().numpy()) for n in m.nodes.values()
             for k, p in n.params.items() if k in ('w', 'b') + BN_KEYS)
    want = MO.loss_and_grads(P, feed['raw'], feed['target'])[0]
    assert abs(ref.loss_and_grads(feed)[0] - want) < 1e-12 * abs(want)


def test_predict_mode_copy_has_no_trainable_statistics_and_depends_on_no_batch():
    a = net_small('train')
    vals = params_by_value(a)
    for v in vals.values():                       # statistics that are not the initial (0, 1)
        if 'mean' in v:
            rng = np.random.RandomState(len(v['mean']))
            v['mean'] = (0.2 * rng.randn(*v['mean'].shape)).astype(np.float32)
            v['std'] = (0.5 + rng.rand(*v['std'].shape)).astype(np.float32)
            v['gamma'] = (0.5 + rng.rand(*v['gamma'].shape)).astype(np.float32)
    b = net_small('predict', vals)
    names = list(b.loss_node.all_trainable_params.keys())
    assert len(names) == 8 and not any(k.endswith(BN_KEYS) for k in names)
    for n in bn_nodes(b):
        assert [n.params[k].apply_train for k in BN_KEYS] == [False, False, False]
        for k in ('w', 'b') + BN_KEYS:
            assert np.array_equal(n.params[k].get_value(), vals[n.name][k])
    ref = BnRef(b)
    feed = feed_for(b, 92, 5, 3)
    ref.loss_and_grads(feed)
    assert all(ref.p(n.params[k]).grad is None for n in bn_nodes(b) for k in BN_KEYS)
    assert not ref.stats                                            # nothing for a step to move
    whole = ref.predict(feed['raw'])
    for i in range(3):                          # sample by sample: the identity train mode lacks
        assert np.abs(ref.predict(feed['raw'][i:i + 1]) - whole[i:i + 1]).max() < 1e-14
    ra = BnRef(a)
    one, three = ra.predict(feed['raw'][:1]), ra.predict(feed['raw'])[:1]
    assert np.abs(one - three).max() > 1e-3
