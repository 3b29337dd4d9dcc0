"""The weighted MultinoulliNLL -- class weights, example weights, mask_class_labeled,
mask_class_not_present (reference loss.py:172-212, 261-347) -- on the device: the three kernel
pairs through the C ABI (generic pair of csrc/softmax_nll.hip, fused head of csrc/head.hip, fused
tail of csrc/tail.hip), then whole training steps on the three paths.

The reference of every comparison is ``ref_loss`` below: a float64 torch-CPU restatement of
loss.py:261-347 (+ AggregateLoss's mean, loss.py:1357-1363), line by line, differentiated by
autograd -- never the kernels' closed form.  Conv layers in front of it come from
oracle.e2_oracle, as in test_ops_gpu.py.  Bounds are the project's own for these ops
(test_ops_gpu.py:16, test_golden_gpu.py:58-59): loss 1e-5 relative, the count within 0.5,
probabilities / dlogits / dpre / dx at TOL = 2e-5 of the reference's largest magnitude,
accumulated dW / db at 1e-4; whole training steps at 1e-4.
"""
import numpy as np
import pytest
import torch

from oracle import e2_oracle as O

pytestmark = pytest.mark.gpu
TOL = 2e-5
ACC = 1e-4
EPS = 1e-5
BOUNDS = dict(probs=TOL, dlogits=TOL, dpre=TOL, dx=TOL, dw=ACC, db=ACC, dwh=ACC, dbh=ACC,
              db1=ACC)
KINDS = ['class_weights', 'masks', 'example_weights', 'all']


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device="cuda")


def relerr(got, ref):
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) \
        else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


# ---- the reference: loss.py:261-347 restated in torch, float64 ------------------------------
def xlogy0(x, y):
    """theano.tensor.xlogx.xlogy0: x * log(y), 0 where x == 0"""
    return torch.where(x == 0, torch.zeros_like(x), x * torch.log(y))


def ref_loss(logits, target, W, dtype=torch.float64):
    """-> (loss, n_tot, pred): ``logits`` a torch tensor (b, n_class, z, x, y) (differentiate
    through it), ``target`` (b, 1, z, x, y) class ids, W = dict(cw, ew, L, M) of numpy arrays or
    None.  n_indep = 1, sparse target, weakness = 0."""
    n_indep = 1
    pred = torch.softmax(logits.to(dtype), dim=1)              # computations.py:175-176
    n_class = pred.shape[1]
    tt = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    target = tt(target)
    classes = torch.arange(n_class, dtype=dtype).reshape(1, n_class, 1, 1, 1)
    target = (target == classes).to(dtype)                     # loss.py:273-278: to 1-hot
    class_weights = 1 if W.get('cw') is None else tt(W['cw']).reshape(1, n_class, 1, 1, 1)
    example_weights = 1 if W.get('ew') is None else tt(W['ew']).unsqueeze(1)   # (b, z, x, y)
    if W.get('L') is not None:                                 # loss.py:307-314
        target = target * tt(W['L']).reshape(-1, n_class, 1, 1, 1)
    nll_up = -xlogy0(target * class_weights * example_weights, pred + EPS)
    n_labelled_up = target.sum()
    if W.get('M') is not None:                                 # loss.py:321-332
        mask_class_not_present = tt(W['M']).reshape(-1, n_class, 1, 1, 1) * torch.ones_like(target)
        nll_dn = -xlogy0(mask_class_not_present * class_weights * example_weights,
                         1.0 - pred + EPS)
        n_labelled_dn = mask_class_not_present.sum()
    else:
        nll_dn = 0.0
        n_labelled_dn = 0.0
    n_tot = n_labelled_up + n_labelled_dn
    nll = (nll_up + nll_dn) * pred.numel() / (n_tot + EPS) / n_indep / n_class
    nll = nll.sum(dim=1, keepdim=True)
    return nll.mean(), float(n_tot), pred                      # AggregateLoss: the mean


def ref_grad(logits_np, target, W, dtype=torch.float64):
    """-> loss, n_tot, probabilities, d loss / d logits (numpy, float64)"""
    lg = torch.tensor(np.asarray(logits_np, np.float64), dtype=dtype, requires_grad=True)
    loss, n_tot, pred = ref_loss(lg, target, W, dtype)
    loss.backward()
    return float(loss.detach()), n_tot, pred.detach().double().numpy(), lg.grad.double().numpy()


def make_weights(rng, kind, N, ncls, sp):
    W = dict(cw=None, ew=None, L=None, M=None)
    if kind in ('class_weights', 'all'):
        W['cw'] = (0.25 + 4 * rng.rand(ncls)).astype(np.float32)
    if kind in ('example_weights', 'all'):
        W['ew'] = (2 * rng.rand(N, *sp)).astype(np.float32)
        W['ew'][:, 0, :2] = 0.0                                 # some examples switched off
    if kind in ('masks', 'all'):
        L = (rng.rand(N, ncls) < 0.6).astype(np.float32)
        M = (rng.rand(N, ncls) < 0.4).astype(np.float32)
        L[0, 0] = 1.0; L[-1, -1] = 0.0                          # both values occur
        M[0, -1] = 1.0; M[-1, 0] = 0.0
        W['L'], W['M'] = L, M
    return W


def unit_weights(N, ncls, sp):
    return dict(cw=np.ones(ncls, np.float32), ew=np.ones((N,) + tuple(sp), np.float32),
                L=np.ones((N, ncls), np.float32), M=np.zeros((N, ncls), np.float32))


def descr(W):
    """the e2_nll_weights descriptor of device copies (None: the unweighted entry points)"""
    from elektronn2_amd import backend
    if W is None:
        return None
    d = lambda a: None if a is None else dev(a)
    ew = None if W.get('ew') is None else dev(W['ew']).unsqueeze(1)
    return backend.nll_weights(class_w=d(W.get('cw')), example_w=ew, labelled=d(W.get('L')),
                               not_present=d(W.get('M')))


# ---- the three kernel pairs: run -> dict of results, reference -> dict of the same keys ------
def run_generic(ctx, logits, t, W):
    N, C = logits.shape[:2]
    probs = torch.full(logits.shape, float("nan"), device="cuda")
    dl = torch.full(logits.shape, float("nan"), device="cuda")
    stats = torch.zeros(2, device="cuda")
    loss = torch.zeros(1, device="cuda")
    wd = descr(W)
    ctx.softmax_nll_fwd(dev(logits), dev(t), probs, stats, weights=wd)
    ctx.softmax_nll_bwd(probs, dev(t), stats, dl, loss, weights=wd)
    return dict(probs=probs, dlogits=dl, loss=float(loss), count=float(stats[1]),
                loss_sum=float(stats[0]))


def ref_generic(logits, t, W):
    loss, n_tot, p, dlog = ref_grad(logits, t, W)
    return dict(probs=p, dlogits=dlog, loss=loss, count=n_tot)


def run_head(ctx, xfull, lo, w, b, t, W):
    cin, ncls = w.shape[1], w.shape[0]
    xd = dev(xfull)[:, lo:lo + cin]                             # channel-sliced view
    sp = xfull.shape[2:]
    N = xfull.shape[0]
    probs = torch.full((N, ncls) + sp, float("nan"), device="cuda")
    stats = torch.zeros(2, device="cuda")
    wd = descr(W)
    ctx.head_fwd(xd, dev(w), dev(b), dev(t), probs, stats, weights=wd)
    dx = torch.full((N, cin) + sp, float("nan"), device="cuda")
    dw = torch.zeros(w.shape, device="cuda")
    db = torch.zeros(ncls, device="cuda")
    loss = torch.zeros(1, device="cuda")
    ctx.head_bwd(xd, dev(w), probs, dev(t), stats, dx, False, dw, db, loss, weights=wd)
    return dict(probs=probs, dx=dx, dw=dw, db=db, loss=float(loss), count=float(stats[1]))


def ref_head(x, w, b, t, W):
    logits = O.conv3d_fwd(x, w) + b.reshape(1, -1, 1, 1, 1)
    loss, n_tot, p, dlog = ref_grad(logits, t, W)
    return dict(probs=p, dx=O.conv3d_dgrad(dlog, w, x.shape), dw=O.conv3d_wgrad(dlog, x, w.shape),
                db=dlog.sum(axis=(0, 2, 3, 4)), loss=loss, count=n_tot)


def run_tail(ctx, x, w1, b1, wh, bh, t, W):
    N, c1 = x.shape[:2]
    sp = x.shape[2:]
    c2, ncls = w1.shape[0], wh.shape[0]
    k = (1, 1, 1)
    assert ctx.tail_supported(c1, c2, ncls)
    wpf = torch.zeros(ctx.conv_ws_bytes(c2, c1, k) // 4 + 64, device="cuda")
    wpd = torch.zeros_like(wpf)
    ctx.conv3d_pack(dev(w1), 0, wpf)
    ctx.conv3d_pack(dev(w1), 1, wpd)
    probs = torch.full((N, ncls) + sp, float("nan"), device="cuda")
    dpre = torch.full((N, c2) + sp, float("nan"), device="cuda")
    dx = torch.full((N, c1) + sp, float("nan"), device="cuda")
    stats = torch.full((2,), float("nan"), device="cuda")
    ws = torch.full((ctx.tail_ws_bytes(x.shape, c2, ncls) // 4 + 16,), float("nan"), device="cuda")
    ns = ctx.tail_fwd_bwd(dev(x), wpf, wpd, dev(b1), dev(wh.reshape(ncls, c2)), dev(bh), dev(t),
                          probs, dpre, dx, stats, ws, weights=descr(W))
    dwh = torch.zeros((ncls, c2), device="cuda")
    dbh = torch.zeros((ncls,), device="cuda")
    db1 = torch.zeros((c2,), device="cuda")
    loss = torch.zeros(1, device="cuda")
    ctx.tail_reduce(ws, ns, c2, ncls, dwh, dbh, db1, stats, loss)
    return dict(probs=probs, dpre=dpre, dx=dx, dwh=dwh, dbh=dbh, db1=db1, loss=float(loss),
                count=float(stats[1]))


def ref_tail(x, w1, b1, wh, bh, t, W):
    pre = O.conv3d_fwd(x, w1)
    h = O.bias_act_fwd(pre, b1, 'relu')
    logits = O.conv3d_fwd(h, wh) + bh.reshape(1, -1, 1, 1, 1)
    loss, n_tot, p, dlog = ref_grad(logits, t, W)
    dh = O.conv3d_dgrad(dlog, wh, h.shape)
    dpre, db1 = O.bias_act_bwd(dh, pre, b1, 'relu')
    return dict(probs=p, dpre=dpre, dx=O.conv3d_dgrad(dpre, w1, x.shape),
                dwh=O.conv3d_wgrad(dlog, h, wh.shape).reshape(wh.shape[0], -1),
                dbh=dlog.sum(axis=(0, 2, 3, 4)), db1=db1, loss=loss, count=n_tot, logits=logits)


def compare(got, ref, what="", bounds=BOUNDS, loss_bound=1e-5):
    """prints every figure before it asserts"""
    figs = {}
    figs['loss'] = abs(got['loss'] - ref['loss']) / max(abs(ref['loss']), 1e-30)
    figs['count'] = abs(got['count'] - ref['count'])
    for k in bounds:
        if k in got:
            figs[k] = relerr(got[k], ref[k])
    print("weighted-nll %s: loss %.9g (ref %.9g) n_tot %.1f (ref %.1f) " % (
        what, got['loss'], ref['loss'], got['count'], ref['count'])
        + " ".join("%s=%.3g" % kv for kv in sorted(figs.items())))
    assert np.isfinite(got['loss'])
    assert figs['loss'] < loss_bound, (what, figs)
    assert figs['count'] < 0.5, (what, figs)
    for k in bounds:
        if k in got:
            assert figs[k] < bounds[k], (what, k, figs)
    return figs


# ---- inputs ---------------------------------------------------------------------------------
def generic_inputs(seed=3, N=2, C=5, sp=(3, 7, 13)):
    """5 classes (neither the head nor the tail takes those), batch 2, 273 positions per item
    (not a multiple of the 256-position work-group), unlabelled voxels"""
    rng = np.random.RandomState(seed)
    logits = (2 * rng.randn(N, C, *sp)).astype(np.float32)
    t = rng.randint(-1, C, (N, 1) + sp).astype(np.float32)
    return rng, logits, t


HEAD_CASES = [(2, 200), (3, 37), (4, 300)]                  # test_ops_gpu.py:1107


def head_inputs(ncls, cin, seed=31):
    rng = np.random.RandomState(seed)
    sp = (3, 7, 13)
    xfull = rng.rand(2, cin + 3, *sp).astype(np.float32)
    w = (rng.randn(ncls, cin, 1, 1, 1) / np.sqrt(cin)).astype(np.float32)
    b = (rng.randn(ncls) / 4).astype(np.float32)
    t = rng.randint(-1, ncls, (2, 1) + sp).astype(np.float32)
    return rng, xfull, w, b, t


TAIL_CASES = [                                              # test_ops_gpu.py:1145-1152
    (200, 200, 2, 1, (10, 37, 37)),
    (200, 200, 2, 1, (5, 21, 21)),
    (150, 200, 2, 1, (4, 30, 31)),
    (37, 53, 3, 2, (3, 7, 13)),
    (208, 208, 4, 1, (2, 9, 11)),
    (200, 24, 2, 3, (1, 5, 7)),
]


def tail_inputs(c1, c2, ncls, N, sp, zero_b1=False):
    rng = np.random.RandomState(c1 + c2 + ncls)
    k = (1, 1, 1)
    x = rng.rand(N, c1, *sp).astype(np.float32)
    w1 = (rng.randn(c2, c1, *k) / np.sqrt(c1)).astype(np.float32)
    b1 = (rng.randn(c2) / 4).astype(np.float32)
    w1[3] = 0.0; b1[3] = 0.0                               # a unit at exactly zero (slope 0.5)
    if zero_b1:
        b1[:] = 0.0
    wh = (rng.randn(ncls, c2, *k) / np.sqrt(c2)).astype(np.float32)
    bh = (rng.randn(ncls) / 4).astype(np.float32)
    t = rng.randint(-1, ncls, (N, 1) + sp).astype(np.float32)
    return rng, x, w1, b1, wh, bh, t


# ---- the four kinds of weights on every kernel pair -------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_generic_pair_weighted(ctx, kind):
    rng, logits, t = generic_inputs()
    W = make_weights(rng, kind, 2, 5, (3, 7, 13))
    compare(run_generic(ctx, logits, t, W), ref_generic(logits, t, W), "generic/" + kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ncls,cin", HEAD_CASES)
def test_head_weighted(ctx, ncls, cin, kind):
    rng, xfull, w, b, t = head_inputs(ncls, cin)
    W = make_weights(rng, kind, 2, ncls, (3, 7, 13))
    x = xfull[:, 2:2 + cin]
    compare(run_head(ctx, xfull, 2, w, b, t, W), ref_head(x, w, b, t, W),
            "head%s/%s" % ((ncls, cin), kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c1,c2,ncls,N,sp", TAIL_CASES)
def test_tail_weighted(ctx, c1, c2, ncls, N, sp, kind):
    rng, x, w1, b1, wh, bh, t = tail_inputs(c1, c2, ncls, N, sp)
    W = make_weights(rng, kind, N, ncls, sp)
    compare(run_tail(ctx, x, w1, b1, wh, bh, t, W), ref_tail(x, w1, b1, wh, bh, t, W),
            "tail%s/%s" % ((c1, c2, ncls, N, sp), kind))


def test_tail_weighted_count_kernel(ctx):
    """more than 65,536 targets: the labelled count comes from the pre-pass kernel"""
    rng, x, w1, b1, wh, bh, t = tail_inputs(8, 8, 3, 2, (6, 75, 75))
    W = make_weights(rng, 'all', 2, 3, (6, 75, 75))
    compare(run_tail(ctx, x, w1, b1, wh, bh, t, W), ref_tail(x, w1, b1, wh, bh, t, W),
            "tail/count-kernel")


# ---- a not-present class that saturates ------------------------------------------------------
def _sat_levels(n):
    """logit levels of the saturated block: half of it at +40, half a ramp 6 .. 40.  At +40,
    1 - p is ~4e-18: p is exactly 1.0f and every formula agrees with log(eps).  It is on the
    ramp, where 1 - p runs through 1e-3 .. 1e-7 (the size of eps and of an f32 ulp of p), that
    `1 - p` by subtraction loses its digits."""
    lv = np.full(n, 40.0)
    lv[n // 2:] = np.linspace(6.0, 40.0, n - n // 2)
    return lv


def _sat_weights(N, ncls, c):
    W = dict(cw=None, ew=None, L=np.ones((N, ncls), np.float32), M=np.zeros((N, ncls), np.float32))
    W['M'][:, c] = 1.0
    W['L'][:, c] = 0.0
    return W


def _f32_restatement_error(logits, t, W):
    """error of the SAME torch code run in float32 (it subtracts: 1.0 - pred) against float64"""
    l64, _, _, g64 = ref_grad(logits, t, W)
    l32, _, _, g32 = ref_grad(logits, t, W, dtype=torch.float32)
    return abs(l32 - l64) / abs(l64), float(np.abs(g32 - g64).max() / np.abs(g64).max())


def test_saturated_not_present_class(ctx):
    """One not-present class has its logits pushed to +40 on a block of voxels (and up a ramp
    6 .. 40 on the block's other half), on all three kernel pairs.  The kernels form 1 - p_c as the
    sum of the other classes' terms; the stated bounds of this file hold, nothing is widened.
    For comparison the float32 run of the reference's own formula (1.0 - pred by subtraction) is
    measured on the same inputs and printed: on the generic inputs it misses the float64 one by
    4.3e-6 (loss, relative) and 6.2e-3 (dlogits, relative to the largest), i.e. its gradient
    would NOT hold TOL = 2e-5.  Measured on an MI355X, kernels against float64: loss 1.1e-7 /
    1.1e-7 / 5.8e-8 (generic / head / tail), dlogits 1.5e-7, head dx 2.5e-7, tail dpre 2.9e-7 and
    dx 3.2e-7, accumulated dW / db <= 1.3e-7."""
    # generic pair: logits set directly
    rng, logits, t = generic_inputs(seed=5)
    blk = logits[:, 2].reshape(2, -1)
    blk[:, :120] = _sat_levels(120)
    logits[:, 2] = blk.reshape(logits[:, 2].shape)
    W = _sat_weights(2, 5, 2)
    e_loss, e_grad = _f32_restatement_error(logits, t, W)
    print("saturated generic: float32 restatement vs float64: loss %.3g dlogits %.3g" % (e_loss, e_grad))
    compare(run_generic(ctx, logits, t, W), ref_generic(logits, t, W), "generic/saturated")
    # head: x on the block = level * w_c / |w_c|^2 -> logit_c = level + b_c
    rng, xfull, w, b, t = head_inputs(3, 37)
    x = xfull[:, 2:2 + 37]
    wc = w[1].reshape(-1).astype(np.float64)
    xs = x.reshape(2, 37, -1)
    xs[:, :, :120] = (wc / (wc @ wc))[None, :, None] * _sat_levels(120)[None, None, :]
    xfull[:, 2:2 + 37] = xs.reshape(x.shape)
    x = xfull[:, 2:2 + 37]
    W = _sat_weights(2, 3, 1)
    ref = ref_head(x, w, b, t, W)
    assert ref['probs'][:, 1].max() > 1 - 1e-12
    compare(run_head(ctx, xfull, 2, w, b, t, W), ref, "head/saturated")
    # tail: b1 = 0 makes the logits homogeneous in x; head row c positive; x scaled per position
    rng, x, w1, b1, wh, bh, t = tail_inputs(37, 53, 3, 2, (3, 7, 13), zero_b1=True)
    wh[0] = np.abs(wh[0])
    lg1 = ref_tail(x, w1, b1, wh, bh, t, dict())['logits'][:, 0].reshape(2, -1)
    alpha = (_sat_levels(120)[None, :] - bh[0]) / (lg1[:, :120] - bh[0])
    xs = x.reshape(2, 37, -1)
    xs[:, :, :120] *= alpha[:, None, :].astype(np.float32)
    x = xs.reshape(x.shape)
    W = _sat_weights(2, 3, 0)
    ref = ref_tail(x, w1, b1, wh, bh, t, W)
    assert ref['probs'][:, 0].max() > 1 - 1e-9
    compare(run_tail(ctx, x, w1, b1, wh, bh, t, W), ref, "tail/saturated")


# ---- limit cases (loss.py:180,186): all-default weights are the ordinary NLL ---------------------
def _same(a, b, what):
    for k in a:
        if isinstance(a[k], torch.Tensor):
            d = float((a[k] - b[k]).abs().max()) / max(float(b[k].abs().max()), 1e-30)
        else:
            d = abs(a[k] - b[k]) / max(abs(b[k]), 1e-30)
        print("limit %s %s: %.3g" % (what, k, d))
        assert d < 1e-6, (what, k, d)


def test_unit_weights_equal_the_unweighted_entry_points(ctx):
    rng, logits, t = generic_inputs()
    _same(run_generic(ctx, logits, t, unit_weights(2, 5, (3, 7, 13))),
          run_generic(ctx, logits, t, None), "generic")
    rng, xfull, w, b, t = head_inputs(3, 37)
    _same(run_head(ctx, xfull, 2, w, b, t, unit_weights(2, 3, (3, 7, 13))),
          run_head(ctx, xfull, 2, w, b, t, None), "head")
    rng, x, w1, b1, wh, bh, t = tail_inputs(37, 53, 3, 2, (3, 7, 13))
    _same(run_tail(ctx, x, w1, b1, wh, bh, t, unit_weights(2, 3, (3, 7, 13))),
          run_tail(ctx, x, w1, b1, wh, bh, t, None), "tail")
    # a descriptor whose members are all NULL is the unweighted loss too
    _same(run_tail(ctx, x, w1, b1, wh, bh, t, dict()), run_tail(ctx, x, w1, b1, wh, bh, t, None),
          "tail/null members")


# ---- degenerate: nothing labelled, nothing marked not-present -> n_tot = 0 ----------------------
def test_nothing_labelled_gives_zero_loss_and_zero_gradients(ctx):
    def check(res, what):
        assert res['loss'] == 0.0 and res['count'] == 0.0, (what, res['loss'], res['count'])
        for k, v in res.items():
            if isinstance(v, torch.Tensor) and k != 'probs':
                assert torch.isfinite(v).all() and float(v.abs().max()) == 0.0, (what, k)
        assert torch.isfinite(res['probs']).all()
    W = lambda N, k, sp: dict(cw=(1 + np.arange(k)).astype(np.float32), L=np.zeros((N, k), np.float32),
                              M=np.zeros((N, k), np.float32), ew=np.ones((N,) + sp, np.float32))
    rng, logits, t = generic_inputs()
    check(run_generic(ctx, logits, t, W(2, 5, (3, 7, 13))), "generic")
    rng, xfull, w, b, t = head_inputs(3, 37)
    check(run_head(ctx, xfull, 2, w, b, t, W(2, 3, (3, 7, 13))), "head")
    rng, x, w1, b1, wh, bh, t = tail_inputs(37, 53, 3, 2, (3, 7, 13))
    check(run_tail(ctx, x, w1, b1, wh, bh, t, W(2, 3, (3, 7, 13))), "tail")


# ---- sum mode (e2_set_loss_grad_mode): unnormalised gradients, count_out = n_tot ----------------
def test_sum_mode_gradients_and_count(ctx):
    def check(run, ref, keys, what):
        norm = run()
        cnt = torch.zeros(1, device="cuda")
        ctx.set_loss_grad_mode(1, cnt)
        try:
            raw = run()
        finally:
            ctx.set_loss_grad_mode(0, None)
        print("sum mode %s: count_out %.1f, n_tot %.1f" % (what, float(cnt), ref['count']))
        assert abs(float(cnt) - ref['count']) < 0.5
        assert abs(raw['loss'] - norm['loss']) <= 1e-6 * abs(norm['loss'])     # loss values unaffected
        for k in keys:
            want = norm[k] * (ref['count'] + EPS)
            d = float((raw[k] - want).abs().max()) / float(want.abs().max())
            print("   %s: %.3g" % (k, d))
            assert d < TOL, (what, k, d)
    rng, logits, t = generic_inputs()
    W = make_weights(rng, 'all', 2, 5, (3, 7, 13))
    check(lambda: run_generic(ctx, logits, t, W), ref_generic(logits, t, W), ['dlogits'], "generic")
    rng, xfull, w, b, t = head_inputs(3, 37)
    W = make_weights(rng, 'all', 2, 3, (3, 7, 13))
    check(lambda: run_head(ctx, xfull, 2, w, b, t, W), ref_head(xfull[:, 2:39], w, b, t, W),
          ['dx', 'dw', 'db'], "head")
    rng, x, w1, b1, wh, bh, t = tail_inputs(37, 53, 3, 2, (3, 7, 13))
    W = make_weights(rng, 'all', 2, 3, (3, 7, 13))
    check(lambda: run_tail(ctx, x, w1, b1, wh, bh, t, W), ref_tail(x, w1, b1, wh, bh, t, W),
          ['dpre', 'dx', 'dwh', 'dbh', 'db1'], "tail")


# =============================================================================================
# whole training steps: one small net per path
# =============================================================================================
MODEL_TOL = 1e-4                         # the project's model-step bound
SP = (3, 23, 23)
NETS = {
    # [1x1x1 relu conv] -> [1x1x1 lin conv to 2 classes]: the tail launch (neuro3d style)
    'tail': [(8, (1, 4, 4), (1, 2, 2), 'relu'), (12, (1, 3, 3), (1, 1, 1), 'relu'),
             (16, (1, 1, 1), (1, 1, 1), 'relu'), (2, (1, 1, 1), (1, 1, 1), 'lin')],
    # a (1,3,3) conv in front of the 3-class head: the fused head, no tail (U-Net style)
    'head': [(8, (1, 4, 4), (1, 2, 2), 'relu'), (12, (1, 3, 3), (1, 1, 1), 'relu'),
             (3, (1, 1, 1), (1, 1, 1), 'lin')],
    # 5 classes: neither (the generic pair)
    'generic': [(8, (1, 4, 4), (1, 2, 2), 'relu'), (12, (1, 3, 3), (1, 1, 1), 'relu'),
                (5, (1, 1, 1), (1, 1, 1), 'lin')],
}
CW0 = {2: [1.0, 4.0], 3: [1.0, 4.0, 0.5], 5: [1.0, 4.0, 0.5, 2.0, 1.5]}


def build_net(path, params, batch=2):
    """the net of NETS[path] under a MultinoulliNLL with class weights (a sequence), example
    weights and both masks"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    spec = NETS[path]
    ncls = spec[-1][0]
    inp = nm.Input((batch, 1) + SP, 'b,f,z,x,y', name='raw')
    out = inp
    for (n_f, k, pool, act), (w, b) in zip(spec, params):
        out = nm.Conv(out, n_f, k, pool, activation_func=act, w=np.asarray(w, np.float32),
                      b=np.asarray(b, np.float32))
    probs = nm.Softmax(out)
    target = nm.Input_like(probs, override_f=1, name='target')
    osp = tuple(probs.shape.spatial_shape)
    ew = nm.Input((batch,) + osp, 'b,z,x,y', name='ew')
    ll = nm.Input((batch, ncls), 'b,f', name='ll')
    npr = nm.Input((batch, ncls), 'b,f', name='np')
    nll = nm.MultinoulliNLL(probs, target, target_is_sparse=True, class_weights=CW0[ncls],
                            example_weights=ew, mask_class_labeled=ll, mask_class_not_present=npr)
    loss = nm.AggregateLoss(nll, name='loss')
    m = nm.model_manager.getmodel()
    m.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=probs)
    m.set_opt_meta_params('Adam', dict(lr=5e-4, mom=0.9, beta2=0.999, wd=0.5e-4))
    return m, nll


def batch_of(path, seed, batch=2):
    spec = NETS[path]
    ncls = spec[-1][0]
    rng = np.random.RandomState(seed)
    osp = O.net_out_shape(spec, SP)
    x = rng.rand(batch, 1, *SP).astype(np.float32)
    t = rng.randint(-1, ncls, (batch, 1) + osp).astype(np.float32)
    W = make_weights(rng, 'all', batch, ncls, osp)
    return x, t, W


def args_of(x, t, W):
    """trainingstep(data, target, *extras): extras in the order of loss_node.input_nodes"""
    return (x, t, W['ew'], W['L'], W['M'])


def ref_step(path, params, x, t, W):
    """loss and the gradient of every (w, b): oracle layers + the restated loss"""
    spec = NETS[path]
    logits, caches = O.net_fwd(spec, params, x)
    loss, n_tot, p, d = ref_grad(logits, t, W)
    grads = [None] * len(spec)
    for i in reversed(range(len(spec))):
        n_f, k, pool, act = spec[i]
        w, b = params[i]
        h, cache = caches[i]
        d, dw, db = O.conv_node_bwd(d, h, np.asarray(w, np.float64), b, cache, pool, act,
                                    need_dx=(i > 0))
        grads[i] = (dw, db)
    return loss, grads


def train_plan(m):
    return m.optimisers['Adam'].step.func


def assert_path(m, nll, path):
    plan = train_plan(m)
    ran_tail = (nll, 'tail_slots') in plan.scratch
    ran_head = (nll, 'head_ws') in plan.scratch
    assert (ran_tail, ran_head) == {'tail': (True, False), 'head': (False, True),
                                    'generic': (False, False)}[path], (path, ran_tail, ran_head)
    assert plan.scratch.get((nll, 'weights')) is not None


@pytest.mark.parametrize("path", ['tail', 'head', 'generic'])
def test_model_step_loss_and_every_gradient(path):
    params = O.init_net(NETS[path], 1, seed=4)
    x, t, W = batch_of(path, 11)
    W['cw'] = np.asarray(CW0[NETS[path][-1][0]], np.float32)
    m, nll = build_net(path, params)
    assert [n.name for n in m.loss_node.input_nodes] == ['raw', 'target', 'ew', 'll', 'np']
    loss_ref, grads_ref = ref_step(path, params, x, t, W)
    g = m.gradients(*args_of(x, t, W))
    names = list(m.loss_node.all_trainable_params.keys())
    assert len(g) == 2 * len(NETS[path])
    for i in range(len(NETS[path])):
        for j, kind in enumerate('wb'):
            e = relerr(g[names.index('conv%s_%s' % (i or '', kind))], grads_ref[i][j])
            print("model %s: d%s layer %d: %.3g" % (path, kind, i, e))
            assert e < MODEL_TOL, (path, kind, i, e)
    loss, tsec, _ = m.trainingstep(*args_of(x, t, W), optimiser='Adam')
    print("model %s: loss %.9g ref %.9g" % (path, float(loss), loss_ref))
    assert abs(float(loss) - loss_ref) / abs(loss_ref) < MODEL_TOL
    assert_path(m, nll, path)


@pytest.mark.parametrize("path", ['tail', 'head', 'generic'])
def test_replay_follows_new_masks_and_class_weights_without_recapture(path):
    """steps 2.. run from the captured graph; new masks arrive through the input arena, new class
    weights through the parameter's device buffer: no new capture, the loss follows"""
    params = O.init_net(NETS[path], 1, seed=4)
    ncls = NETS[path][-1][0]
    x, t, W = batch_of(path, 11)
    W['cw'] = np.asarray(CW0[ncls], np.float32)
    m, nll = build_net(path, params)
    for _ in range(2):                                       # eager, then the capture
        m.trainingstep(*args_of(x, t, W), optimiser='Adam')
    plan = train_plan(m)
    graphs = plan._graphs
    assert graphs, "the step was not captured"
    handles = list(graphs)
    cur = [(np.asarray(p.get_value(), np.float64)) for p in m.trainable_params]
    names = list(m.loss_node.all_trainable_params.keys())
    P = [(cur[names.index('conv%s_w' % (i or ''))], cur[names.index('conv%s_b' % (i or ''))])
         for i in range(len(NETS[path]))]
    W2 = dict(W)
    W2['L'] = 1.0 - W['L']; W2['L'][0, 0] = 1.0
    W2['M'] = 1.0 - W['M']; W2['M'][0, 0] = 0.0
    W2['cw'] = np.asarray(CW0[ncls], np.float32)[::-1].copy() * 1.5
    nll.class_weights.set_value(W2['cw'])
    loss_new, _, _ = m.trainingstep(*args_of(x, t, W2), optimiser='Adam')
    assert plan._graphs is graphs and list(plan._graphs) == handles, "the graph was re-captured"
    ref_new, _ = ref_step(path, P, x, t, W2)
    ref_old, _ = ref_step(path, P, x, t, W)
    print("replay %s: loss %.9g, reference with the new values %.9g, with the old ones %.9g"
          % (path, float(loss_new), ref_new, ref_old))
    assert abs(float(loss_new) - ref_new) / abs(ref_new) < MODEL_TOL
    assert abs(ref_new - ref_old) / abs(ref_old) > 100 * MODEL_TOL       # (the case tells them apart)
    assert abs(float(loss_new) - ref_old) / abs(ref_old) > 10 * MODEL_TOL


def test_ring_steps_equal_single_steps():
    """trainingsteps(k, ring=...) with the weight inputs in the ring slots == k single steps
    (losses 1e-5, parameters 1e-4: the bounds of test_model_gpu's ring test)"""
    path = 'tail'
    params = O.init_net(NETS[path], 1, seed=6)
    batches = [batch_of(path, 20 + j) for j in range(3)]
    a, _ = build_net(path, params)
    la = [float(a.trainingstep(*args_of(*batches[i % 3]), optimiser='Adam')[0]) for i in range(7)]
    pa = [p.get_value() for p in a.loss_node.all_trainable_params.values()]
    b, nll = build_net(path, params)
    lb = [float(b.trainingstep(*args_of(*batches[0]), optimiser='Adam')[0])]
    plan = train_plan(b)
    assert [n.name for n in plan.inputs] == ['raw', 'target', 'ew', 'll', 'np']
    ring = torch.zeros(3, plan.input_arena.numel(), device=plan.ctx.device)
    for j in range(3):
        for node, src in zip(plan.inputs, args_of(*batches[j])):
            o, n = plan.input_slices[node]
            assert n == src.size
            ring[j, o:o + n] = torch.tensor(src.ravel(), device=ring.device)
    plan.set_input_ring(ring)
    plan._step_state[0] += 1                                 # the next slot is the one of step 1
    l4, _ = b.trainingsteps(4, optimiser='Adam', ring=ring)
    l2, _ = b.trainingsteps(2, optimiser='Adam', ring=ring)
    lb += [float(v) for v in l4] + [float(v) for v in l2]
    assert plan._multi, "no multi-step graph was captured"
    for i, (u, v) in enumerate(zip(la, lb)):
        print("ring step %d: %.9g vs %.9g" % (i, u, v))
        assert abs(u - v) < 1e-5 * abs(u), (i, la, lb)
    for u, v in zip(pa, [p.get_value() for p in b.loss_node.all_trainable_params.values()]):
        assert relerr(v, u) < 1e-4
    assert_path(b, nll, path)


def test_checkpoint_round_trip_and_untouched_class_weights(tmp_path):
    """save -> modelload -> the same loss on the same batch; after Adam steps with weight decay
    the class-weight parameter holds exactly what it was given (no gradient slot, outside the
    optimiser's prefix of the parameter arena)"""
    from elektronn2_amd.neuromancer.model import modelload
    path = 'tail'
    params = O.init_net(NETS[path], 1, seed=4)
    x, t, W = batch_of(path, 11)
    m, nll = build_net(path, params)
    given = np.array([0.3, 2.75], np.float32)
    nll.class_weights.set_value(given)
    for _ in range(3):
        m.trainingstep(*args_of(x, t, W), optimiser='Adam')
    assert np.array_equal(nll.class_weights.get_value(), given)
    off, n, _ = m._slots[id(nll.class_weights)]
    assert off >= m.n_train and m.G.numel() <= max(m.n_train, 4)      # no gradient slot
    assert all(p is not nll.class_weights for p in m.trainable_params)
    f = str(tmp_path / "w.mdl")
    m.save(f)
    l0 = float(m.loss(*args_of(x, t, W)))
    m2 = modelload(f, name='rebuilt')
    assert np.array_equal(m2.nodes['nll'].class_weights.get_value(), given)
    l1 = float(m2.loss(*args_of(x, t, W)))
    assert l0 == l1, (l0, l1)
