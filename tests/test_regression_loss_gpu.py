"""SquaredLoss / AbsLoss / BinaryNLL / GaussianNLL and mixed AggregateLoss on the GPU
(csrc/loss_elem.hip; loss.py:829-887, 953-1101, 1215-1276, 1346-1363).

The reference of every comparison is the float64 torch-CPU restatement of
tests/test_regression_loss_host.py (checked there against the closed forms), differentiated by
autograd, on the float32 inputs the kernels saw -- never the kernels' closed form, never the code
under test.  Bounds are the project's own: ops at 2e-5 of the reference's largest magnitude
(tests/test_ops_gpu.py:16); losses at 1e-5 relative, counts exact (tests/test_weighted_nll_gpu.py:
10-12 allows 0.5); whole steps -- loss, prediction, every gradient, parameters after Adam steps --
at 1e-4 (tests/test_model_gpu.py:17); several steps in one graph / deferred steps against single
steps at 1e-5 (losses) and 1e-4 (parameters) as tests/test_activations_gpu.py does; a resumed
run at tests/test_checkpoint.py:171-185's bit-equal parameters and 1e-5."""
import numpy as np
import pytest
import torch

from test_activations_gpu import Ref, ADAM
from test_activations_host import act_torch
from test_dropout_gpu import VIEWS, SHAPES
from test_regression_loss_host import (ref_squared, ref_abs, ref_binary, ref_gauss, ref_aggregate,
                                       n_labelled, is_masked)

pytestmark = pytest.mark.gpu
TOL = 2e-5          # ops
TOL_LOSS = 1e-5     # a loss value
TOL_STEP = 1e-4     # loss, gradients, parameters after an Adam step
MAX_SIGMOID_PRE = 5.0
MIN_MARGIN_GAP = 1e-3   # ||d| - margin| of every constructed element of the op tests


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device='cuda')


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float32).astype(np.float64), requires_grad=grad)


def close(got, want, tol):
    return abs(float(got) - float(want)) <= tol * abs(float(want))


# kind, options.  margin / scale_correction as float32 values (the kernels read them as float32)
M, SC = float(np.float32(0.3)), float(np.float32(0.7))
CASES = [("squared", dict()), ("squared", dict(margin=M)), ("squared", dict(scale_correction=SC)),
         ("squared", dict(margin=M, scale_correction=SC)),
         ("abs", dict()), ("abs", dict(margin=M)), ("abs", dict(scale_correction=SC)),
         ("abs", dict(margin=M, scale_correction=SC)),
         ("binary_nll", dict()), ("binary_nll", dict(subtract_label_entropy=True)),
         ("gauss_nll", dict()), ("gauss_nll", dict(sig_is_log=True))]
CASE_IDS = ["%s%s" % (k, "".join("-" + o for o in sorted(kw))) for k, kw in CASES]


def make_inputs(rng, kind, kw, shape, masked=0.3):
    """(pred, sig or None, target) float32.  Margin cases are CONSTRUCTED with
    ||d| - margin| >= 2e-3 (well above MIN_MARGIN_GAP after the float32 rounding of p = t - d)"""
    n = int(np.prod(shape))
    if kind == "gauss_nll":
        mu, t = rng.randn(*shape), rng.randn(*shape)
        sig = rng.uniform(-3, 3, shape) if kw.get("sig_is_log") else rng.uniform(0.05, 3, shape)
        return mu.astype(np.float32), sig.astype(np.float32), t.astype(np.float32)
    if kind == "binary_nll":
        p, t = rng.uniform(0.02, 0.98, shape), rng.uniform(0, 1, shape)
        t.flat[rng.permutation(n)[: n // 5]] = rng.randint(0, 2, n // 5)       # hard labels too
    else:
        t = rng.randn(*shape) * 1.5
        if "margin" in kw:
            gap = 2e-3 + rng.rand(*shape) * 0.4
            mag = np.abs(kw["margin"] + np.where(rng.rand(*shape) < 0.5, gap, -gap))
            p = t - mag * np.where(rng.rand(*shape) < 0.5, 1.0, -1.0)
        else:
            p = t + rng.randn(*shape)
    t = t.astype(np.float32)
    t.flat[rng.permutation(n)[: int(round(masked * n))]] = -666.0
    return p.astype(np.float32), None, t


def restated(kind, kw, p, s, t):
    """the node's output from float64 tensors"""
    if kind == "squared":
        return ref_squared(p, t, kw.get("margin"), kw.get("scale_correction"))
    if kind == "abs":
        return ref_abs(p, t, kw.get("margin"), kw.get("scale_correction"))
    if kind == "binary_nll":
        return ref_binary(p, t, kw.get("subtract_label_entropy", False))
    return ref_gauss(p, s, t, kw.get("sig_is_log", False))


def reference(kind, kw, p, s, t, w=1.0, K=1):
    """(L, n_lab, coef, total, dtotal/dp, dtotal/ds) for ONE term with mixing weight w among K"""
    tp, tt = t64(p, True), t64(t)
    ts = t64(s, True) if s is not None else None
    out = restated(kind, kw, tp, ts, tt)
    L = out.mean()
    total = w * L / K
    leaves = [tp] + ([ts] if ts is not None else [])
    g = [x.numpy() for x in torch.autograd.grad(total, leaves)]
    n_lab = p.size if kind == "gauss_nll" else n_labelled(t)
    den = p.size if kind == "gauss_nll" else n_lab + 1
    return (float(L.detach()), n_lab, w / (K * den), float(total.detach()), g[0],
            g[1] if ts is not None else None)


def margin_gap(kw, p, t):
    if "margin" not in kw:
        return np.inf
    un = ~is_masked(t64(t)).numpy()
    d = np.abs(t.astype(np.float64) - p.astype(np.float64))[un]
    return np.abs(d - kw["margin"]).min() if d.size else np.inf


def term_of(kind, kw):
    from elektronn2_amd import backend
    return backend.loss_term(kind, margin=dev([kw["margin"]]) if "margin" in kw else None,
                             scale_correction=dev([kw["scale_correction"]]) if "scale_correction" in kw else None,
                             subtract_label_entropy=kw.get("subtract_label_entropy", False),
                             sig_is_log=kw.get("sig_is_log", False))


def run_term(ctx, term, pv, sv, tv, w):
    """forward + mix of one term -> (loss_out, term_loss, count, coef tensor)"""
    slab = torch.full((4 * ctx.loss_partials(pv),), float('nan'), device='cuda')
    coef, tl, cnt = (torch.full((8,), -3.0, device='cuda') for _ in range(3))
    out = torch.full((1,), -3.0, device='cuda')
    ctx.loss_fwd(term, pv, sv, tv, slab)
    ctx.loss_mix([term], [slab], [pv.numel()], dev([w]), coef, tl, cnt, out)
    return out, tl, cnt, coef


# ---- 1. the kernels through the C ABI ------------------------------------------------------------------
@pytest.mark.parametrize("view", VIEWS, ids=[v[0] for v in VIEWS])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fwd_mix_bwd_through_the_c_abi(ctx, case, view):
    """partial sums + mix give L, n_lab (exact), coef and the total; backward at TOL, overwriting and
    accumulating onto a non-zero start; nothing outside a view written; sources only read; finite"""
    kind, kw = case
    rng = np.random.RandomState(300 + 13 * CASE_IDS.index("%s%s" % (kind, "".join("-" + o for o in sorted(kw))))
                                + len(view[0]))
    term = term_of(kind, kw)
    w = 0.7
    for shape in SHAPES:
        p, s, t = make_inputs(rng, kind, kw, shape)
        assert margin_gap(kw, p, t) >= MIN_MARGIN_GAP
        L, n_lab, coef_ref, total, gp, gs = reference(kind, kw, p, s, t, w)
        stores = {}

        def put(name, a, fill):
            store, v = view[1](shape)
            store.fill_(fill)
            v.copy_(dev(a))
            stores[name] = (store, v, store.clone())
            return v
        pv, tv = put('p', p, -77.0), put('t', t, -55.0)
        sv = put('s', s, 0.5) if s is not None else None
        out, tl, cnt, coef = run_term(ctx, term, pv, sv, tv, w)
        got = float(out.item())
        assert np.isfinite(got), (shape, got)
        assert close(got, total, TOL_LOSS), (shape, got, total)
        assert close(tl[0].item(), L, TOL_LOSS), (shape, tl[0].item(), L)
        assert cnt[0].item() == n_lab, (shape, cnt[0].item(), n_lab)
        assert close(coef[0].item(), coef_ref, 1e-6), (shape, coef[0].item(), coef_ref)
        assert torch.all(coef[1:] == -3.0) and torch.all(tl[1:] == -3.0) and torch.all(cnt[1:] == -3.0)
        # ---- backward: overwrite, then accumulate onto a non-zero start, through views
        mstore, mview = view[1](shape)
        mstore.fill_(0); mview.fill_(1)
        outside = mstore == 0
        g0 = (rng.randn(*shape) * max(np.abs(gp).max(), 1e-3)).astype(np.float32)
        for acc in (False, True):
            dstore, dv = view[1](shape)
            dstore.fill_(-11.0)
            dv.copy_(dev(g0))
            dbefore = dstore.clone()
            if s is not None:
                sstore, dsv = view[1](shape)
                sstore.fill_(-12.0)
                dsv.copy_(dev(g0))
                sbefore = sstore.clone()
            else:
                dsv = None
            ctx.loss_bwd(term, pv, sv, tv, coef[0:1], dv, dsv, accumulate=acc)
            base = g0.astype(np.float64) if acc else 0.0
            dgot = dv.cpu().numpy()
            assert np.all(np.isfinite(dgot)), (shape, acc)
            assert rel(dgot, base + gp) < TOL, (shape, acc, rel(dgot, base + gp))
            assert torch.equal(dstore[outside], dbefore[outside]), (shape, acc)
            if kind != "gauss_nll":
                un = ~is_masked(t64(t)).numpy()
                want0 = g0 if acc else np.zeros_like(g0)
                assert np.array_equal(bits(dgot[~un]), bits(want0[~un])), (shape, acc)   # masked: exactly 0 added
            if s is not None:
                sgot = dsv.cpu().numpy()
                assert np.all(np.isfinite(sgot)), (shape, acc)
                assert rel(sgot, base + gs) < TOL, (shape, acc, rel(sgot, base + gs))
                assert torch.equal(sstore[outside], sbefore[outside]), (shape, acc)
        if s is not None:          # one of the two gradients alone
            only = torch.full(shape, 9.0, device='cuda')
            ctx.loss_bwd(term, pv, sv, tv, coef[0:1], None, only)
            assert rel(only.cpu().numpy(), gs) < TOL
            ctx.loss_bwd(term, pv, sv, tv, coef[0:1], only, None)
            assert rel(only.cpu().numpy(), gp) < TOL
        for name, (store, v, before) in stores.items():
            assert torch.equal(store, before), (shape, name)          # the sources are only read


def test_bad_arguments_are_errors(ctx):
    from elektronn2_amd import backend
    x = torch.rand((1, 2, 3, 4, 5), device='cuda')
    y = torch.rand((1, 2, 3, 4, 6), device='cuda')
    slab = torch.zeros(4 * ctx.loss_partials(x), device='cuda')
    one = dev([1.0])
    t = backend.loss_term('squared')
    with pytest.raises(backend.E2Error, match="size mismatch"):
        ctx.loss_fwd(t, x, None, y, torch.zeros(64, device='cuda'))
    with pytest.raises(backend.E2Error, match="size mismatch"):
        ctx.loss_bwd(t, x, None, x, one, y)
    with pytest.raises(backend.E2Error, match="no gradient view"):
        ctx.loss_bwd(t, x, None, x, one, None)
    with pytest.raises(backend.E2Error, match="GAUSS_NLL alone"):
        ctx.loss_bwd(t, x, None, x, one, x.clone(), x.clone())
    with pytest.raises(backend.E2Error, match="needs sig"):
        ctx.loss_fwd(backend.loss_term('gauss_nll'), x, None, x, slab)
    with pytest.raises(backend.E2Error, match="too small"):
        ctx.loss_fwd(t, x, None, x, slab[:0])
    bad = backend.loss_term('squared')
    bad.kind = 9
    with pytest.raises(backend.E2Error, match="unknown loss kind"):
        ctx.loss_fwd(bad, x, None, x, slab)
    with pytest.raises(backend.E2Error, match="unknown loss kind"):
        ctx.loss_bwd(bad, x, None, x, one, x.clone())
    eight = torch.zeros(16, device='cuda')
    with pytest.raises(backend.E2Error, match="at most 8"):
        ctx.loss_mix([t] * 9, [slab] * 9, [x.numel()] * 9, eight, eight, eight, eight, one)
    # the C entry itself refuses what the bridge checks first
    import ctypes as C
    ta = (backend.LossTerm * 9)(*([t] * 9))
    pa = (C.c_void_p * 9)(*([slab.data_ptr()] * 9))
    ra = (C.c_size_t * 9)(*([1] * 9))
    na = (C.c_int64 * 9)(*([x.numel()] * 9))
    fp = lambda v: C.c_void_p(v.data_ptr())
    rc = backend.lib().e2_loss_mix(ctx.h, 9, ta, pa, ra, na, fp(eight), fp(eight), fp(eight), fp(eight), fp(one))
    assert rc != 0 and b"1..8" in backend.lib().e2_last_error()
    assert backend.lib().e2_loss_partials(ctx.h, None) == 0
    # the row count depends on the sizes alone and is capped
    big = torch.empty((1, 3, 116, 132, 132), device='cuda')
    assert ctx.loss_partials(big) == 1024
    assert ctx.loss_partials(big[:, :, :, 1:, 3:]) == 1024
    assert ctx.loss_partials(x) == 1 and ctx.loss_partials(x[:, :, :, :, 1:]) == 1


# ---- 2. planted values ---------------------------------------------------------------------------------
def _check_dense(ctx, kind, kw, p, s, t, what):
    L, n_lab, coef_ref, total, gp, gs = reference(kind, kw, p, s, t)
    term = term_of(kind, kw)
    pv, tv = dev(p), dev(t)
    sv = dev(s) if s is not None else None
    out, tl, cnt, coef = run_term(ctx, term, pv, sv, tv, 1.0)
    assert np.isfinite(out.item()), what
    assert close(out.item(), total, TOL_LOSS), (what, out.item(), total)
    assert cnt[0].item() == n_lab, (what, cnt[0].item(), n_lab)
    dp = torch.full(p.shape, 7.0, device='cuda')
    ds = torch.full(p.shape, 7.0, device='cuda') if s is not None else None
    ctx.loss_bwd(term, pv, sv, tv, coef[0:1], dp, ds)
    got = dp.cpu().numpy()
    assert np.all(np.isfinite(got)), what
    assert rel(got, gp) < TOL, (what, rel(got, gp))
    if s is not None:
        assert np.all(np.isfinite(ds.cpu().numpy())) and rel(ds.cpu().numpy(), gs) < TOL, what
    return got, n_lab


def test_planted_masks_margins_and_ties(ctx):
    """-666.0 and -666.004 are masked, -666.01 is not; |d| == margin counts (>=); AbsLoss at p == t
    has slope 0; no element is left out of a comparison"""
    rng = np.random.RandomState(41)
    shape = (1, 2, 1, 3, 8)
    for kind in ("squared", "abs"):
        for kw in (dict(), dict(margin=0.5), dict(margin=0.5, scale_correction=SC)):
            # dyadic values: |d| == margin holds exactly in float32 and float64
            t = np.array(rng.choice([0.75, -0.25, 1.5, 2.0], shape), np.float32)
            side = np.where(rng.rand(*shape) < 0.5, 1.0, -1.0)
            step = rng.choice([0.5, 0.25, 1.0, 0.75, 0.125], shape)        # 0.5: on the margin
            p = (t - side * step).astype(np.float32)
            t.flat[0:3] = [-666.0, -666.004, -666.01]
            p.flat[3], t.flat[3] = 0.25, 0.75                              # |d| == margin exactly
            p.flat[4], t.flat[4] = 0.75, 0.25
            p.flat[5] = t.flat[5]                                          # a tie: sgn 0 = 0
            d = np.abs(t.astype(np.float64) - p.astype(np.float64))
            un = ~is_masked(t64(t)).numpy()
            assert np.all((np.abs(d[un] - 0.5) >= MIN_MARGIN_GAP) | (d[un] == 0.5))
            assert (d == 0.5).sum() >= 2
            got, n_lab = _check_dense(ctx, kind, kw, p, None, t, (kind, kw))
            assert n_lab == p.size - 2
            assert got.flat[0] == 0 and got.flat[1] == 0 and got.flat[2] != 0
            assert got.flat[3] != 0 and got.flat[4] != 0                   # on the margin: counted
            assert got.flat[5] == 0
            if "margin" in kw:
                assert np.all(got.ravel()[(d < 0.5).ravel()] == 0)


def test_planted_bernoulli_corners(ctx):
    """p in {0, 1e-7, 0.5, 1 - 6e-8, 1} x t in {0, 1, 0.3}: the xlogy0 zero branches, gradients up
    to 1e5, all finite; masks; with and without the label entropy"""
    ps = np.array([0.0, 1e-7, 0.5, 1 - 6e-8, 1.0], np.float32)
    ts = np.array([0.0, 1.0, 0.3], np.float32)
    rng = np.random.RandomState(42)
    p = np.concatenate([np.repeat(ps, 3), rng.uniform(0.05, 0.95, 17)]).astype(np.float32)
    t = np.concatenate([np.tile(ts, 5), rng.uniform(0, 1, 17)]).astype(np.float32)
    t[-1], t[-2] = -666.0, -666.004
    p, t = p.reshape(1, 2, 1, 2, 8), t.reshape(1, 2, 1, 2, 8)
    for ent in (False, True):
        got, n_lab = _check_dense(ctx, "binary_nll", dict(subtract_label_entropy=ent), p, None, t, ent)
        assert n_lab == 30 and got.flat[-1] == 0 and got.flat[-2] == 0
        assert np.abs(got).max() > 1e3                                     # (1 / (n_lab + 1)) * 1e5


def test_planted_gaussian_ranges(ctx):
    rng = np.random.RandomState(43)
    shape = (2, 2, 2, 5, 9)
    mu, t = rng.randn(*shape).astype(np.float32), rng.randn(*shape).astype(np.float32)
    sig = rng.uniform(0.05, 4, shape).astype(np.float32)
    sig.flat[:4] = [0.05, 0.05, 4.0, 1.0]
    _check_dense(ctx, "gauss_nll", dict(), mu, sig, t, "sig")
    ls = rng.uniform(-3, 3, shape).astype(np.float32)
    ls.flat[:4] = [-3.0, 3.0, 0.0, -3.0]
    _check_dense(ctx, "gauss_nll", dict(sig_is_log=True), mu, ls, t, "log sig")


@pytest.mark.parametrize("kind,kw", [("squared", dict(margin=0.5, scale_correction=SC)), ("abs", dict()),
                                     ("binary_nll", dict(subtract_label_entropy=True))])
def test_all_masked_target(ctx, kind, kw):
    """n_lab = 0: loss 0, gradient 0, no NaN"""
    shape = (1, 3, 2, 5, 7)
    p = np.random.RandomState(44).uniform(0.1, 0.9, shape).astype(np.float32)
    t = np.full(shape, -666.0, np.float32)
    term = term_of(kind, kw)
    out, tl, cnt, coef = run_term(ctx, term, dev(p), None, dev(t), 1.0)
    assert out.item() == 0.0 and tl[0].item() == 0.0 and cnt[0].item() == 0.0 and coef[0].item() == 1.0
    dp = torch.full(shape, float('nan'), device='cuda')
    ctx.loss_bwd(term, dev(p), None, dev(t), coef[0:1], dp, None)
    assert torch.all(dp == 0)
    assert float(ref_aggregate([restated(kind, kw, t64(p), None, t64(t))], [1.0])) == 0.0


# ---- 3. reproducibility ------------------------------------------------------------------------------------
def test_forward_and_mix_are_bit_reproducible(ctx):
    rng = np.random.RandomState(45)
    shape = (2, 3, 20, 64, 66)
    terms, slabs, preds, tgts = [], [], [], []
    for kind, kw in (("binary_nll", dict()), ("squared", dict(margin=M, scale_correction=SC)),
                     ("gauss_nll", dict())):
        p, s, t = make_inputs(rng, kind, kw, shape)
        terms.append(term_of(kind, kw))
        preds.append((dev(p), dev(s) if s is not None else None))
        tgts.append(dev(t))
        slabs.append(torch.empty(4 * ctx.loss_partials(preds[-1][0]), device='cuda'))
    assert slabs[0].numel() == 4 * 248                      # ceil(506880 / 2048) work-groups
    mix = dev([1.0, 0.25, 2.0])
    seen = []
    for run in range(3):
        coef, tl, cnt = (torch.zeros(8, device='cuda') for _ in range(3))
        out = torch.zeros(1, device='cuda')
        for sl in slabs:
            sl.fill_(float(run))                            # (needs no zero fill: every row is stored)
        for tm, (pv, sv), tv, sl in zip(terms, preds, tgts, slabs):
            ctx.loss_fwd(tm, pv, sv, tv, sl)
        ctx.loss_mix(terms, slabs, [shape_n for shape_n in [int(np.prod(shape))] * 3], mix, coef, tl, cnt, out)
        seen.append((bits(out.cpu().numpy()).tolist(), bits(tl.cpu().numpy()).tolist(),
                     bits(coef.cpu().numpy()).tolist()))
    assert seen[0] == seen[1] == seen[2]


# ---- 4-8. nodes, plans, whole steps ----------------------------------------------------------------------
class RefL(Ref):
    """tests/test_activations_gpu.py's float64 restatement of a graph, with the element-wise losses
    and several inputs.  ``feed``: {input node name: float32 array}.  Asserts on its OWN values that
    the case is well-posed: kinked hidden units (MIN_PRE there), every sigmoid unit's pre-activation
    within MAX_SIGMOID_PRE, no unmasked |d| within 1e-6 of a margin."""

    def forward(self, feed, seed=0, counter=0):
        import torch.nn.functional as F
        m = self.model
        self.min_pre, self.n_kinked = np.inf, 0
        self.max_sig_pre, self.margin_gap = 0.0, np.inf
        self.terms = {}
        val = {}
        for node in m.nodes.values():
            kind = type(node).__name__
            par = node.parent
            if kind == 'Input':
                if node.name in feed:
                    val[node] = t64(feed[node.name])
            elif kind in ('Conv', 'UpConv'):
                h, w, b = val[par], self.p(node.w), self.p(node.b)
                if kind == 'UpConv':
                    y = F.conv_transpose3d(h, w.permute(1, 0, 2, 3, 4), stride=tuple(node.pool_shape))
                else:
                    y = F.conv3d(h, w.flip(2, 3, 4))
                    if any(q != 1 for q in node.pool_shape):
                        y = F.max_pool3d(y, tuple(node.pool_shape))
                assert not node.batch_normalisation
                y = y + b.view(1, -1, 1, 1, 1)
                if node.activation_func == 'sigmoid':
                    self.max_sig_pre = max(self.max_sig_pre, float(y.detach().abs().max()))
                val[node] = self.act(node, y)
            elif kind == 'Pool':
                val[node] = F.max_pool3d(val[par], tuple(node.pool_shape))
            elif kind == 'Crop':
                val[node] = val[par][node._slicer()]
            elif kind == 'Concat':
                val[node] = torch.cat([val[q] for q in par], dim=1)
            elif kind in ('SquaredLoss', 'AbsLoss'):
                mg = None if node.margin is None else float(np.float32(node.margin.get_value()))
                sc = None if node.scale_correction is None else \
                    float(np.float32(node.scale_correction.get_value()))
                p, t = val[par[0]], val[par[1]]
                val[node] = (ref_abs if kind == 'AbsLoss' else ref_squared)(p, t, mg, sc)
                if mg is not None:
                    un = ~is_masked(t)
                    self.margin_gap = min(self.margin_gap,
                                          float(((t - p).detach().abs()[un] - mg).abs().min()))
                self.terms[node.name] = (float(val[node].detach().mean()), int((~is_masked(t)).sum()))
            elif kind == 'BinaryNLL':
                p, t = val[par[0]], val[par[1]]
                val[node] = ref_binary(p, t, node.subtract_label_entropy)
                self.terms[node.name] = (float(val[node].detach().mean()), int((~is_masked(t)).sum()))
            elif kind == 'GaussianNLL':
                val[node] = ref_gauss(val[par[0]], val[par[1]], val[par[2]], node.sig_is_log)
                self.terms[node.name] = (float(val[node].detach().mean()), val[par[0]].numel())
            elif kind == 'AggregateLoss':
                w = np.asarray(node.mixing_weights.get_value(), np.float32).astype(np.float64)
                val[node] = ref_aggregate([val[q] for q in par], w)
            else:
                raise NotImplementedError(kind)
        return val[m.loss_node], val[m.prediction_node]

    def loss_and_grads(self, feed, seed=0, counter=0):
        for v in self.P.values():
            v.grad = None
        loss, pred = self.forward(feed)
        assert self.min_pre >= 1e-6, "ill-posed case: a kinked unit at %.1e" % self.min_pre
        assert self.max_sig_pre <= MAX_SIGMOID_PRE, "sigmoid pre-activation %.2f" % self.max_sig_pre
        assert self.margin_gap >= 1e-6, "ill-posed case: |d| within %.1e of the margin" % self.margin_gap
        loss.backward()
        return float(loss.detach()), pred.detach().numpy()


def _done(nm, inp, loss, pred, ext=None):
    model = nm.model_manager.getmodel()
    tg = [n for n in loss.input_nodes if n is not inp][0]
    model.designate_nodes(input_node=inp, target_node=tg, loss_node=loss, prediction_node=pred,
                          prediction_ext=ext)
    model.set_opt_meta_params('Adam', ADAM)
    return model


def _trunk(nm, batch, seed):
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 1, 5, 18, 18), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 6, (1, 3, 3))
    out = nm.Conv(out, 8, (3, 3, 3), activation_func='tanh')
    return inp, out


def net_a(batch=1, seed=51):
    """3 layers, a 3-feature sigmoid head + BinaryNLL"""
    from elektronn2_amd import neuromancer as nm
    inp, out = _trunk(nm, batch, seed)
    head = nm.Conv(out, 3, (1, 1, 1), activation_func='sigmoid', name='head')
    t = nm.Input_like(head, name='target')
    nll = nm.BinaryNLL(head, t)
    loss = nm.AggregateLoss(nll, name='loss')
    return _done(nm, inp, loss, head, ext=[loss, head])


def net_b(batch=1, seed=52):
    """a lin head + SquaredLoss(margin, scale_correction)"""
    from elektronn2_amd import neuromancer as nm
    inp, out = _trunk(nm, batch, seed)
    head = nm.Conv(out, 1, (1, 1, 1), activation_func='lin', name='head')
    t = nm.Input_like(head, name='target')
    loss = nm.AggregateLoss(nm.SquaredLoss(head, t, margin=0.3, scale_correction=0.7), name='loss')
    return _done(nm, inp, loss, head)


def net_c(batch=1, seed=53):
    """a tanh head + AbsLoss"""
    from elektronn2_amd import neuromancer as nm
    inp, out = _trunk(nm, batch, seed)
    head = nm.Conv(out, 2, (1, 1, 1), activation_func='tanh', name='head')
    t = nm.Input_like(head, name='target')
    loss = nm.AggregateLoss(nm.AbsLoss(head, t), name='loss')
    return _done(nm, inp, loss, head)


def net_d(batch=1, seed=54):
    """two heads on one trunk: lin mu, soft+ sigma, GaussianNLL"""
    from elektronn2_amd import neuromancer as nm
    inp, out = _trunk(nm, batch, seed)
    mu = nm.Conv(out, 2, (1, 1, 1), activation_func='lin', name='mu')
    sig = nm.Conv(out, 2, (1, 1, 1), activation_func='soft+', name='sig')
    t = nm.Input_like(mu, name='target')
    loss = nm.AggregateLoss(nm.GaussianNLL(mu, sig, t), name='loss')
    return _done(nm, inp, loss, mu)


def net_e(batch=1, seed=55, margin=None, sc=None):
    """BinaryNLL on head A, SquaredLoss and AbsLoss on head B (two writers of one gradient)"""
    from elektronn2_amd import neuromancer as nm
    inp, out = _trunk(nm, batch, seed)
    a = nm.Conv(out, 3, (1, 1, 1), activation_func='sigmoid', name='head_a')
    b = nm.Conv(out, 1, (1, 1, 1), activation_func='lin', name='head_b')
    ta, tb = nm.Input_like(a, name='target'), nm.Input_like(b, name='target_b')
    loss = nm.AggregateLoss([nm.BinaryNLL(a, ta), nm.SquaredLoss(b, tb, margin=margin, scale_correction=sc),
                             nm.AbsLoss(b, tb)], mixing_weights=[1.0, 0.25, 2.0], name='loss')
    return _done(nm, inp, loss, a)


def net_e_opts(batch=1, seed=55):
    return net_e(batch, seed, margin=0.3, sc=0.7)


def net_f(batch=1, seed=56):
    """U-Net shaped (UpConvMerge) with a regression head"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 1, 6, 20, 20), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 8, (1, 3, 3), activation_func='elu')
    c1 = nm.Conv(c0, 8, (1, 3, 3), activation_func='tanh')
    p1 = nm.Pool(c1, (1, 2, 2))
    c2 = nm.Conv(p1, 12, (3, 3, 3))
    c3 = nm.Conv(c2, 12, (3, 3, 3), activation_func='elu')
    mrg = nm.UpConvMerge(c1, c3, 16)
    c4 = nm.Conv(mrg, 8, (1, 3, 3))
    head = nm.Conv(c4, 1, (1, 1, 1), activation_func='lin', name='head')
    t = nm.Input_like(head, name='target')
    loss = nm.AggregateLoss(nm.SquaredLoss(head, t), name='loss')
    return _done(nm, inp, loss, head)


def feed_for(m, seed, masked=0.3):
    """{input name: array}: the image in [0, 1); Bernoulli targets in [0, 1] and regression targets
    ~ N(0, 1), both with about 30 % masked elements except under a GaussianNLL (no mask there)"""
    rng = np.random.RandomState(seed)
    feed = {}
    users = dict((n.name, [c for c in n.children.values()]) for n in m.loss_node.input_nodes)
    for n in m.loss_node.input_nodes:
        sh = tuple(n.shape.shape)
        kinds = set(type(c).__name__ for c in users[n.name])
        if n is m.input_node:
            a = rng.rand(*sh)
        elif 'BinaryNLL' in kinds:
            a = rng.rand(*sh)
        else:
            a = rng.randn(*sh)
        a = a.astype(np.float32)
        if n is not m.input_node and 'GaussianNLL' not in kinds:
            a.flat[rng.permutation(a.size)[: int(masked * a.size)]] = -666.0
        feed[n.name] = a
    return feed


def args_of(m, feed):
    return [feed[n.name] for n in m.loss_node.input_nodes]


# name, constructor, seed of the batch (chosen on the reference alone: RefL's assertions)
NETS = [("a_sigmoid_binary", net_a, 61), ("b_lin_squared", net_b, 61), ("c_tanh_abs", net_c, 61),
        ("d_gaussian", net_d, 61), ("e_mixed", net_e, 61), ("f_unet_squared", net_f, 62)]


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("name,make,data_seed", NETS, ids=[n[0] for n in NETS])
def test_loss_gradients_and_adam_steps_against_float64(name, make, data_seed, batch):
    """loss, prediction, EVERY parameter gradient -- eager, captured and replayed calls -- and three
    Adam steps (eager, captured, replayed: the first is the 1-step case) against float64 autograd"""
    m = make(batch)
    feed = feed_for(m, data_seed)
    args = args_of(m, feed)
    ref = RefL(m)
    for call in range(3):                                   # eager, capture, replay
        lref, pref = ref.loss_and_grads(feed)
        loss = float(m.loss(*args))
        print("%s b%d call %d: loss %.7f ref %.7f (kinked closest %.1e, sigmoid pre %.2f, margin gap %.1e)"
              % (name, batch, call, loss, lref, ref.min_pre, ref.max_sig_pre, ref.margin_gap))
        assert close(loss, lref, TOL_STEP), (call, loss, lref)
        e = rel(m.predict(feed[m.input_node.name]), pref)
        assert e < TOL_STEP, (call, e)
        got = m.gradients(*args)
        names = list(m.loss_node.all_trainable_params.keys())
        want = ref.grads()
        assert len(got) == len(want) == len(names)
        errs = dict((nme, rel(g, w)) for nme, g, w in zip(names, got, want))
        print("%s b%d call %d: gradients, worst %s"
              % (name, batch, call, sorted(errs.items(), key=lambda kv: -kv[1])[:3]))
        for nme, g, w in zip(names, got, want):
            assert np.abs(w).max() > 0, nme
            assert errs[nme] < TOL_STEP, (call, nme, errs[nme])
        # the terms as the nodes show them
        for n in m.loss_node.parent:
            L, n_lab = ref.terms[n.name]
            assert close(n.term_value, L, TOL_LOSS), (n.name, n.term_value, L)
            assert n.n_labelled == n_lab, (n.name, n.n_labelled, n_lab)
    for step in range(3):                                   # Adam: eager, captured, replayed
        lref, _ = ref.loss_and_grads(feed)
        ref.adam(**ADAM)
        loss = float(m.trainingstep(*args, optimiser='Adam')[0])
        assert close(loss, lref, TOL_STEP), (step, loss, lref)
        worst = ('', 0.0)
        for nme, p in m.loss_node.all_trainable_params.items():
            e = rel(p.get_value(), ref.p(p).detach().numpy())
            worst = max(worst, (nme, e), key=lambda kv: kv[1])
            assert e < TOL_STEP, (step, nme, e)
        print("%s b%d step %d: loss %.7f ref %.7f, parameters worst %s" % (name, batch, step, loss, lref, worst))
    plan = m.optimisers['Adam'].step.func
    assert plan._graphs, "the step was not captured"


def test_launch_sequence_and_untouched_softmax_path():
    """K + 1 + K launches for K terms: every term has a slab, the aggregate owns coef / total; two
    losses on one prediction make the second backward accumulate; a softmax net keeps its plan"""
    m = net_e()
    feed = feed_for(m, 61)
    m.gradients(*args_of(m, feed))
    plan = m._grad_func.func
    agg = m.loss_node
    assert agg.elementwise and plan._labelled_count() is None
    for k, n in enumerate(agg.parent):
        assert plan.scratch[n, 'agg'] == (agg, k) and plan.out[n] is None
        assert plan.scratch[n, 'partials'].numel() == 4 * plan.ctx.loss_partials(plan.out[n.pred])
    assert plan._loss_dev() is plan.scratch[agg, 'loss']
    from test_activations_gpu import net_convs, batch_for
    s = net_convs()
    x, t = batch_for(s, 31)
    s.gradients(x, t)
    sp = s._grad_func.func
    nll = s.loss_node.parent[0]
    assert not s.loss_node.elementwise
    assert sp._loss_dev() is sp.scratch[nll, 'loss'] and (s.loss_node, 'loss') not in sp.scratch


# ---- 4. parameters read in place -------------------------------------------------------------------------
def test_margin_scale_correction_and_mixing_weights_are_read_in_place():
    """after set_value the next REPLAY of the captured plans follows the new values"""
    m = net_e_opts()
    feed = feed_for(m, 61)
    args = args_of(m, feed)
    for _ in range(3):
        m.gradients(*args)
        m.loss(*args)
    gplan, lplan = m._grad_func.func, m.loss_node._output_func.func
    graphs = (list(gplan._graphs), list(lplan._graphs))
    assert all(graphs)
    se = m.nodes['se']
    for mg, sc, mix in ((0.45, 1.6, [0.5, 3.0, 0.125]), (0.2, 0.35, [2.0, 1.0, 0.0])):
        se.params['margin'].set_value(np.float32(mg))
        se.params['scale_correction'].set_value(np.float32(sc))
        m.loss_node.params['mixing_weights'].set_value(np.asarray(mix, np.float32))
        ref = RefL(m)
        lref, _ = ref.loss_and_grads(feed)
        assert close(float(m.loss(*args)), lref, TOL_STEP)
        got = m.gradients(*args)
        for nme, g, w in zip(m.loss_node.all_trainable_params.keys(), got, ref.grads()):
            assert rel(g, w) < TOL_STEP, (mg, nme, rel(g, w))
        assert close(se.term_value, ref.terms['se'][0], TOL_LOSS)
        assert (list(gplan._graphs), list(lplan._graphs)) == graphs          # no new capture


# ---- 6. the model protocol ---------------------------------------------------------------------------------
def test_model_functions_agree_with_single_synchronous_steps():
    """Model.loss, predict_ext, gradients; trainingstep(sync=False); trainingsteps(4, ring) with the
    device-side loss history -- against synchronous single steps (losses 1e-5, parameters 1e-4)"""
    feeds = None

    def fresh():
        mm = net_a()
        return mm
    a = fresh()
    feeds = [feed_for(a, 70 + i) for i in range(3)]
    A = lambda mm, i: args_of(mm, feeds[i % 3])
    ref = RefL(a)
    lref, pref = ref.loss_and_grads(feeds[0])
    l1 = float(a.loss(*A(a, 0)))
    l2, pr = a.predict_ext(*A(a, 0))
    assert close(l1, lref, TOL_STEP) and close(float(l2), l1, 1e-6) and rel(pr, pref) < TOL_STEP
    for g, w in zip(a.gradients(*A(a, 0)), ref.grads()):
        assert rel(g, w) < TOL_STEP
    sync = [float(a.trainingstep(*A(a, i), optimiser='Adam')[0]) for i in range(9)]
    end_a = [p.get_value() for p in a.loss_node.all_trainable_params.values()]
    # deferred: the first call waits for its own loss, then one call late
    b = fresh()
    late = [float(b.trainingstep(*A(b, i), optimiser='Adam', sync=False)[0]) for i in range(9)]
    torch.cuda.synchronize()
    assert close(late[0], sync[0], 1e-6)
    for i in range(1, 9):
        assert close(late[i], sync[i - 1], 1e-5), (i, late, sync)
    for u, v in zip(end_a, [p.get_value() for p in b.loss_node.all_trainable_params.values()]):
        assert rel(v, u) < 1e-4
    # several steps in one graph, batches out of a ring, losses from the device-side history
    c = fresh()
    for i in range(2):                                       # eager + capture (builds the plan)
        c.trainingstep(*A(c, i), optimiser='Adam')
    single = sync[2:6]
    pl = c.optimisers['Adam'].step.func
    ring = torch.empty((3, pl.input_arena.numel()), device='cuda')
    for i in range(3):                                       # the step after the two above reads slot 0
        for n in c.loss_node.input_nodes:
            o, cnt = pl.input_slices[n]
            ring[i, o:o + cnt] = dev(feeds[(2 + i) % 3][n.name]).reshape(-1)
    losses, tsec = c.trainingsteps(4, optimiser='Adam', ring=ring)
    assert len(losses) == 4 and len(set(float(v) for v in losses)) == 4
    for u, v in zip(single, losses):
        assert close(float(v), u, 1e-5), (single, list(losses))
    hist = pl.loss_history(4)
    assert np.array_equal(np.asarray(hist, np.float32), np.asarray(losses, np.float32))
    d = fresh()
    for i in range(6):
        d.trainingstep(*A(d, i), optimiser='Adam')
    for pc, pd in zip(c.loss_node.all_trainable_params.values(), d.loss_node.all_trainable_params.values()):
        assert rel(pc.get_value(), pd.get_value()) < 1e-4


# ---- 7. checkpoint -----------------------------------------------------------------------------------------
def test_checkpoint_after_two_steps_resumes_to_the_same_third_step(tmp_path):
    from elektronn2_amd.neuromancer.model import modelload
    a = net_e_opts()
    feed = feed_for(a, 61)
    args = args_of(a, feed)
    a.nodes['se'].params['margin'].set_value(np.float32(0.4))
    a.loss_node.params['mixing_weights'].set_value(np.asarray([1.5, 0.25, 2.0], np.float32))
    for _ in range(2):
        a.trainingstep(*args, optimiser='Adam')
    f = str(tmp_path / "loss.mdl")
    a.save(f)
    saved = [p.get_value() for p in a.loss_node.all_trainable_params.values()]
    third = float(a.trainingstep(*args, optimiser='Adam')[0])
    end_p = [p.get_value() for p in a.loss_node.all_trainable_params.values()]
    b = net_e_opts(seed=99)                                  # other weights, nothing on the device
    modelload(f, b)
    for v, p in zip(saved, b.loss_node.all_trainable_params.values()):
        assert np.array_equal(v, p.get_value())              # bit-equal
    assert float(b.nodes['se'].params['margin'].get_value()) == float(np.float32(0.4))
    assert float(b.nodes['se'].params['scale_correction'].get_value()) == float(np.float32(0.7))
    assert np.array_equal(b.loss_node.params['mixing_weights'].get_value(), np.asarray([1.5, 0.25, 2.0], np.float32))
    got = float(b.trainingstep(*args, optimiser='Adam')[0])
    assert close(got, third, 2e-6), (third, got)
    for v, p in zip(end_p, b.loss_node.all_trainable_params.values()):
        assert np.abs(v - p.get_value()).max() <= 1e-5 * np.abs(v).max()
    # the graph rebuilt from the file alone: classes, options, values
    c = modelload(f)
    kinds = [type(n).__name__ for n in c.loss_node.parent]
    assert kinds == ['BinaryNLL', 'SquaredLoss', 'AbsLoss'] and c.loss_node.elementwise
    assert float(c.nodes['se'].params['margin'].get_value()) == float(np.float32(0.4))
    assert np.array_equal(c.loss_node.params['mixing_weights'].get_value(), np.asarray([1.5, 0.25, 2.0], np.float32))
    for v, p in zip(saved, c.loss_node.all_trainable_params.values()):
        assert np.array_equal(v, p.get_value())
    b2 = net_e_opts(seed=98)
    modelload(f, b2)
    assert close(float(c.loss(*args_of(c, feed))), float(b2.loss(*args)), 1e-6)


# ---- 8. bf16 operand mode ----------------------------------------------------------------------------------
@pytest.fixture()
def process_bf16():
    import elektronn2_amd
    elektronn2_amd.set_mfma_dtype('bf16')
    yield
    elektronn2_amd.set_mfma_dtype('f32')


def test_bf16_mode_keeps_the_loss_kernels_in_f32(process_bf16):
    """one gradient evaluation of net (a) in bf16 operand mode: the loss and the gradient the loss
    kernels wrote, against the restatement on the float32 prediction the DEVICE produced, at TOL"""
    m = net_a()
    feed = feed_for(m, 61)
    m.gradients(*args_of(m, feed))
    plan = m._grad_func.func
    torch.cuda.synchronize()
    head = m.nodes['head']
    p = plan.out[head].detach().cpu().numpy()
    t = feed['target']
    L, n_lab, coef, total, gp, _ = reference("binary_nll", dict(), p, None, t)
    assert close(plan._loss_dev().item(), total, TOL_LOSS)
    assert rel(plan.grad[head].detach().cpu().numpy(), gp) < TOL
    nll = m.loss_node.parent[0]
    assert nll.n_labelled == n_lab and close(nll.term_value, L, TOL_LOSS)
