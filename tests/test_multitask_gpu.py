"""Multi-task nets on the GPU: K MultinoulliNLL terms under one AggregateLoss.

1. the generic pair and the mix (e2_nll_multi_fwd / e2_nll_mix / e2_nll_multi_bwd,
   csrc/softmax_nll.hip) and the fused multi-head pair (e2_multihead_fwd / _bwd,
   csrc/multihead.hip) through the C ABI;
2. nets with several softmax heads on one trunk -- fused and generic route -- against a float64
   restatement of the whole step;
3. the model protocol: mixing weights read in place, graph replay, several steps per launch,
   checkpoints, one bf16 step.

The reference of every comparison is tests/test_multitask_host.py's float64 loop (pinned there to
the oracle and to autograd) on the float32 inputs the kernels saw.  Bounds are the project's own:
tests/test_nll_indep_gpu.py::check_against for the loss ops (probabilities 1e-6, loss and sums 1e-5,
dlogits 1e-5, counts exact); tests/test_ops_gpu.py::test_fused_classifier_head for the fused head
(2e-5, dx accumulated onto a constant 1e-3, db 1e-4); whole steps 5e-4 and a bf16 loss 1e-2 as
tests/test_nll_indep_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_activations_gpu import Ref, ADAM, MIN_PRE
from test_multitask_host import multi_nll, case_inputs, W3, EPS

pytestmark = pytest.mark.gpu
TOL = 5e-4          # tests/test_nll_indep_gpu.py (TOL_ADAM)
TOL_HEAD = 2e-5     # tests/test_ops_gpu.py:21


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def relerr(got, ref):
    got = host(got).astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def bits(a):
    a = host(a) if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def close(got, want, tol):
    return abs(float(got) - float(want)) <= tol * abs(float(want))


def nan_like(shape):
    return torch.full(tuple(shape), float("nan"), device="cuda")


# ---- 1a. the generic pair and the mix ---------------------------------------------------------------
SAME = dict(classes=(3, 4, 2), spatial=((3, 7, 19),) * 3)                       # S = 399
MIXED = dict(classes=(3, 4, 2), spatial=((3, 7, 19), (2, 5, 131), (3, 7, 19)))     # S = 399 / 1310
_REF = {}


def reference(name, **kw):
    """(logits, targets, restatement) -- computed once per case, shared, never written to"""
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _REF:
        lgs, tgs = case_inputs(**dict(dict(SAME=SAME, MIXED=MIXED)[name], **kw))
        for a in lgs + tgs:
            a.setflags(write=False)
        _REF[key] = (lgs, tgs, multi_nll(lgs, tgs, W3))
    return _REF[key]


def run_generic(ctx, lgs, tgs, w=W3, alias=False):
    """zero, forward, mix, backward on fresh contiguous buffers"""
    K = len(lgs)
    lgd, tgd = [dev(a) for a in lgs], [dev(a) for a in tgs]
    probs = [nan_like(a.shape) for a in lgs]
    stats = torch.zeros(2 * K, device="cuda")
    ctx.nll_multi_fwd(lgd, tgd, probs, stats)
    p_out = [p.clone() for p in probs]
    coef, term, count = (nan_like((8,)) for _ in range(3))
    loss = nan_like((1,))
    ctx.nll_mix(K, stats, dev(w), coef, term, count, loss)
    dls = probs if alias else [nan_like(a.shape) for a in lgs]
    ctx.nll_multi_bwd(probs, tgd, coef, dls)
    torch.cuda.synchronize()
    return dict(probs=p_out, stats=stats, coef=coef, term=term, count=count, loss=loss, dl=dls)


def check_against(got, want, w=W3):
    total, Ls, Ns, Ps, Ds, Ss = want
    K = len(Ls)
    print("loss %.8f ref %.8f" % (float(got['loss']), total))
    for k in range(K):
        print("  term %d: probs %.2e dlogits %.2e L %.8f ref %.8f count %s ref %d"
              % (k, relerr(got['probs'][k], Ps[k]), relerr(got['dl'][k], Ds[k]) if Ns[k] else 0.0,
                 float(got['term'][k]), Ls[k], float(got['count'][k]), Ns[k]))
    for k in range(K):
        assert relerr(got['probs'][k], Ps[k]) < 1e-6
        assert float(got['stats'][2 * k + 1]) == Ns[k] and float(got['count'][k]) == Ns[k]
        if Ns[k]:
            assert close(got['stats'][2 * k], Ss[k], 1e-5) and close(got['term'][k], Ls[k], 1e-5)
            assert relerr(got['dl'][k], Ds[k]) < 1e-5
        else:                                      # exact zeros, and K unchanged
            assert float(got['stats'][2 * k]) == 0.0 and float(got['term'][k]) == 0.0
            assert not host(got['dl'][k]).any()
        assert close(got['coef'][k], float(w[k]) / (K * (Ns[k] + EPS)), 1e-6)
    if total:
        assert close(got['loss'], total, 1e-5)
    else:
        assert float(got['loss']) == 0.0
    assert np.isnan(host(got['coef'][K:])).all() and np.isnan(host(got['term'][K:])).all()


@pytest.mark.parametrize("name,empty", [("SAME", None), ("MIXED", None), ("SAME", 1), ("SAME", 'all')],
                         ids=["S399", "S399_S1310", "one_head_unlabelled", "nothing_labelled"])
def test_generic_pair_and_mix_against_the_float64_restatement(ctx, name, empty):
    if empty == 'all':
        lgs, tgs, _ = reference(name)
        tgs = [np.full_like(t, -1) for t in tgs]
        want = multi_nll(lgs, tgs, W3)
        assert want[0] == 0.0
    else:
        lgs, tgs, want = reference(name, empty=empty)
    got = run_generic(ctx, lgs, tgs)
    check_against(got, want)
    for d in got['dl']:
        assert np.isfinite(host(d)).all()


def test_probabilities_are_bit_equal_to_per_head_launches_and_alias_and_null_targets(ctx):
    lgs, tgs, want = reference("MIXED")
    got = run_generic(ctx, lgs, tgs)
    for k, (lg, tg) in enumerate(zip(lgs, tgs)):
        p1 = nan_like(lg.shape)
        s1 = torch.zeros(2, device="cuda")
        ctx.softmax_nll_fwd(dev(lg), dev(tg), p1, s1)
        torch.cuda.synchronize()
        assert np.array_equal(bits(p1), bits(got['probs'][k]))
        assert float(s1[1]) == float(got['stats'][2 * k + 1])
        assert close(s1[0], got['stats'][2 * k], 1e-6)
    aliased = run_generic(ctx, lgs, tgs, alias=True)                 # dlogits over the probabilities
    for a, b in zip(aliased['dl'], got['dl']):
        assert np.array_equal(bits(a), bits(b))
    stats = torch.full((6,), 7.0, device="cuda")
    for targets, st in ((None, stats), ([None] * 3, None)):          # probabilities only
        probs = [nan_like(a.shape) for a in lgs]
        ctx.nll_multi_fwd([dev(a) for a in lgs], targets, probs, st)
        torch.cuda.synchronize()
        for p, q in zip(probs, got['probs']):
            assert np.array_equal(bits(p), bits(q))
    assert host(stats).tolist() == [7.0] * 6


def test_generic_pair_on_strided_views_touches_nothing_else(ctx):
    """probabilities as channel slices of one wider buffer (the Concat layout), targets as the
    channels of one (n, 3, ...) buffer (the split layout), logits and dlogits as slices -- each
    inside NaN-filled storage"""
    lgs, tgs, want = reference("SAME")
    n, sp = 2, (3, 7, 19)
    cs = [a.shape[1] for a in lgs]
    off = np.cumsum([1] + cs)                       # one NaN channel in front
    lbuf, pbuf, dbuf = (nan_like((n, sum(cs) + 2) + sp) for _ in range(3))
    tbuf = nan_like((n, 5) + sp)
    for k in range(3):
        lbuf[:, off[k]:off[k + 1]] = dev(lgs[k])
        tbuf[:, 1 + k:2 + k] = dev(tgs[k])
    view = lambda buf: [buf[:, off[k]:off[k + 1]] for k in range(3)]
    tv = [tbuf[:, 1 + k:2 + k] for k in range(3)]
    lcopy, tcopy = lbuf.clone(), tbuf.clone()
    stats = torch.zeros(6, device="cuda")
    coef, term, count, loss = (torch.zeros(8, device="cuda") for _ in range(4))
    ctx.nll_multi_fwd(view(lbuf), tv, view(pbuf), stats)
    ctx.nll_mix(3, stats, dev(W3), coef, term, count, loss[:1])
    ctx.nll_multi_bwd(view(pbuf), tv, coef, view(dbuf))
    torch.cuda.synchronize()
    got = dict(probs=view(pbuf), stats=stats, coef=torch.cat([coef[:3], nan_like((5,))]),
               term=torch.cat([term[:3], nan_like((5,))]), count=count, loss=loss[:1], dl=view(dbuf))
    check_against(got, want)
    for buf in (pbuf, dbuf):                        # not a bit changed outside the output views
        rest = host(buf).copy()
        rest[:, 1:1 + sum(cs)] = np.nan
        assert np.isnan(rest).all()
    assert np.array_equal(bits(lbuf), bits(lcopy)) and np.array_equal(bits(tbuf), bits(tcopy))
    assert not host(loss[1:]).any() and not host(coef[3:]).any()


def test_the_mixing_weights_are_read_in_place_eagerly_and_from_a_captured_graph(ctx):
    lgs, tgs, _ = reference("SAME")
    lgd, tgd = [dev(a) for a in lgs], [dev(a) for a in tgs]
    probs = [nan_like(a.shape) for a in lgs]
    dls = [nan_like(a.shape) for a in lgs]
    stats = torch.zeros(6, device="cuda")
    coef, term, count = (torch.zeros(8, device="cuda") for _ in range(3))
    loss = torch.zeros(1, device="cuda")
    w = dev(W3)

    def launches():
        ctx.fill(stats, 0.0)
        ctx.nll_multi_fwd(lgd, tgd, probs, stats)
        ctx.nll_mix(3, stats, w, coef, term, count, loss)
        ctx.nll_multi_bwd(probs, tgd, coef, dls)

    def check(weights):
        total, Ls, Ns, Ps, Ds, _ = multi_nll(lgs, tgs, weights)
        assert close(loss, total, 1e-5)
        for k in range(3):
            assert close(coef[k], float(weights[k]) / (3 * (Ns[k] + EPS)), 1e-6)
            assert relerr(dls[k], Ds[k]) < 1e-5

    launches()
    torch.cuda.synchronize()
    check(W3)
    w2 = np.array([0.25, 3.0, 1.5], np.float32)
    w.copy_(dev(w2))                                                  # overwrite, rerun
    launches()
    torch.cuda.synchronize()
    check(w2)
    side = torch.cuda.Stream()
    old = ctx.stream
    torch.cuda.synchronize()
    ctx.set_stream(side)
    try:
        with torch.cuda.stream(side):
            ctx.graph_begin()
            launches()
            g = ctx.graph_end()
            w3 = np.array([1.0, 0.0, 2.0], np.float32)
            for weights in (w2, w3):                                  # captured once, replayed
                w.copy_(dev(weights))
                for d in dls:
                    d.fill_(float("nan"))
                ctx.graph_launch(g)
                side.synchronize()
                check(weights)
            ctx.graph_destroy(g)
    finally:
        ctx.set_stream(old)


def test_bad_arguments_and_sum_mode_are_errors_that_launch_nothing(ctx):
    from elektronn2_amd import backend
    lgs, tgs, _ = reference("SAME")
    lgd, tgd = [dev(a) for a in lgs], [dev(a) for a in tgs]
    out = [torch.full(a.shape, 7.0, device="cuda") for a in lgs]
    good_p = [torch.rand(a.shape, device="cuda") for a in lgs]
    stats = torch.full((6,), 7.0, device="cuda")
    coef, term, count = (torch.full((8,), 7.0, device="cuda") for _ in range(3))
    loss = torch.full((1,), 7.0, device="cuda")
    w = dev(W3)
    sw = lambda lst, k, v: [v if i == k else a for i, a in enumerate(lst)]
    bad_fwd = [(lgd, tgd, out, 0), (lgd * 3, tgd * 3, out * 3, 9),                  # k out of range
               (lgd, sw(tgd, 1, None), out, 3),                                     # some targets NULL
               (lgd, tgd, sw(out, 0, out[1]), 3),                                   # classes
               (lgd, sw(tgd, 2, tgd[2][:1]), out, 3),                               # batch
               (sw(lgd, 1, lgd[1][:1]), sw(tgd, 1, tgd[1][:1]), sw(out, 1, out[1][:1]), 3),
               (lgd, sw(tgd, 0, tgd[0][:, :, :, :, :18]), out, 3),                  # spatial
               (lgd, sw(tgd, 0, lgd[0]), out, 3),                                   # target.c != 1
               (sw(lgd, 0, None), tgd, out, 3), (lgd, tgd, sw(out, 2, None), 3)]    # NULL views
    for lg, tg, pr, k in bad_fwd:
        with pytest.raises(backend.E2Error):
            ctx.nll_multi_fwd(lg, tg, pr, stats, k=k)
    with pytest.raises(backend.E2Error):
        ctx.nll_multi_fwd(lgd, tgd, out, None)                                      # targets need stats
    bad_bwd = [(good_p, tgd, out, 0), (good_p, None, out, 3), (good_p, sw(tgd, 1, None), out, 3),
               (good_p, tgd, sw(out, 0, out[1]), 3), (good_p, sw(tgd, 2, tgd[2][:, :, :2]), out, 3)]
    for pr, tg, dl, k in bad_bwd:
        with pytest.raises(backend.E2Error):
            ctx.nll_multi_bwd(pr, tg, coef, dl, k=k)
    for k in (0, 9):
        with pytest.raises(backend.E2Error):
            ctx.nll_mix(k, stats, w, coef, term, count, loss)
    with pytest.raises(backend.E2Error):
        ctx.nll_mix(3, stats, None, coef, term, count, loss)
    ctx.set_loss_grad_mode(True, torch.zeros(1, device="cuda"))
    try:
        with pytest.raises(backend.E2Error, match="sum mode"):
            ctx.nll_multi_fwd(lgd, tgd, out, stats)
        with pytest.raises(backend.E2Error, match="sum mode"):
            ctx.nll_mix(3, stats, w, coef, term, count, loss)
        with pytest.raises(backend.E2Error, match="sum mode"):
            ctx.nll_multi_bwd(good_p, tgd, coef, out)
        _fused_calls_refused(ctx, match="sum mode")
    finally:
        ctx.set_loss_grad_mode(False, None)
    torch.cuda.synchronize()
    for t in out + [stats, coef, term, count, loss]:
        assert float(t.min()) == 7.0 and float(t.max()) == 7.0


# ---- 1b. the fused multi-head pair ---------------------------------------------------------------------
FUSED = [(37, (3, 4, 3), 2, (3, 7, 13)), (64, (2, 2), 2, (3, 7, 13)), (300, (4, 4, 4, 4), 2, (3, 7, 13)),
         (200, (2,) * 8, 2, (3, 7, 13)), (8, (3, 4, 3), 1, (4, 65, 65))]
FUSED_IDS = ["cin37_343", "cin64_22", "cin300_4444", "cin200_2x8", "more_tiles_than_the_grid"]
_FREF = {}


def fused_reference(cin, classes, n, sp):
    """inputs of one fused case and everything float64 says about them; shared, read-only"""
    key = (cin, classes, n, sp)
    if key not in _FREF:
        rng = np.random.RandomState(cin + len(classes))
        K = len(classes)
        xfull = rng.rand(n, cin + 3, *sp).astype(np.float32)
        x = xfull[:, 2:2 + cin]
        ws = [(rng.randn(c, cin) / np.sqrt(cin)).astype(np.float32) for c in classes]
        bs = [(rng.randn(c) / 4).astype(np.float32) for c in classes]
        tgs = []
        for k, c in enumerate(classes):
            t = rng.randint(0, c, (n, 1) + sp).astype(np.float32)
            t[rng.rand(*t.shape) < 0.1 + 0.1 * k] = -1             # clearly different counts
            t.reshape(-1)[5:9] = c
            t.reshape(-1)[11] = 0.5
            tgs.append(t)
        wmix = (0.5 + rng.rand(K)).astype(np.float32)
        x64 = x.astype(np.float64)
        lgs = [np.einsum('oc,ncdhw->nodhw', w.astype(np.float64), x64) + b.reshape(1, -1, 1, 1, 1)
               for w, b in zip(ws, bs)]
        total, Ls, Ns, Ps, Ds, Ss = multi_nll(lgs, tgs, wmix)
        dx = sum(np.einsum('oc,nodhw->ncdhw', w.astype(np.float64), d) for w, d in zip(ws, Ds))
        dws = [np.einsum('nodhw,ncdhw->oc', d, x64) for d in Ds]
        dbs = [d.sum(axis=(0, 2, 3, 4)) for d in Ds]
        for a in [xfull] + ws + bs + tgs:
            a.setflags(write=False)
        _FREF[key] = dict(xfull=xfull, ws=ws, bs=bs, tgs=tgs, wmix=wmix, lgs=lgs, total=total, Ls=Ls,
                          Ns=Ns, Ps=Ps, Ds=Ds, Ss=Ss, dx=dx, dws=dws, dbs=dbs)
    return _FREF[key]


@pytest.mark.parametrize("cin,classes,n,sp", FUSED, ids=FUSED_IDS)
def test_fused_pair_against_float64_and_against_the_generic_route(ctx, cin, classes, n, sp):
    r = fused_reference(cin, classes, n, sp)
    K, tot = len(classes), sum(classes)
    assert ctx.multihead_supported(cin, classes)
    xd = dev(r['xfull'])[:, 2:2 + cin]                           # x as a channel slice
    wd, bd, td = [dev(a) for a in r['ws']], [dev(a) for a in r['bs']], [dev(a) for a in r['tgs']]
    pbuf = nan_like((n, tot + 2) + sp)                           # the Concat layout
    off = np.cumsum([1] + list(classes))
    probs = [pbuf[:, off[k]:off[k + 1]] for k in range(K)]
    stats = torch.zeros(2 * K, device="cuda")
    ctx.multihead_fwd(xd, wd, bd, td, probs, stats)
    coef, term, count = (nan_like((8,)) for _ in range(3))
    loss = nan_like((1,))
    ctx.nll_mix(K, stats, dev(r['wmix']), coef, term, count, loss)
    # a NaN-filled workspace of exactly the promised size inside watched storage
    nb = ctx.multihead_bwd_ws_bytes((n, cin) + sp, tot)
    assert nb % 4 == 0
    wsbuf = nan_like((nb // 4 + 64,))
    ws = wsbuf[32:32 + nb // 4]
    dx = nan_like((n, cin) + sp)                                 # overwritten
    # onto a prefill, twice.  The prefill is a power of two of the gradients' own magnitude, so
    # that adding it and taking it off again costs no digits of what is measured (onto 0.5 the
    # sums of a 5e-3 gradient lose 7 bits: 2e-5 by themselves)
    PW, PB = 2.0 ** -8, -2.0 ** -8
    dws = [torch.full(w.shape, PW, device="cuda") for w in r['ws']]
    dbs = [torch.full(b.shape, PB, device="cuda") for b in r['bs']]
    ctx.multihead_bwd(xd, wd, probs, td, coef, dx, False, dws, dbs, ws)
    dx2 = torch.full((n, cin) + sp, 1e-3, device="cuda")         # accumulated onto a constant
    ctx.multihead_bwd(xd, wd, probs, td, coef, dx2, True, dws, dbs, ws)
    torch.cuda.synchronize()
    assert np.isnan(host(wsbuf[:32])).all() and np.isnan(host(wsbuf[32 + nb // 4:])).all()
    rest = host(pbuf).copy()
    rest[:, 1:1 + tot] = np.nan
    assert np.isnan(rest).all()
    for k in range(K):
        print("head %d: probs %.2e S %.7f ref %.7f N %s ref %d dw %.2e db %.2e"
              % (k, relerr(probs[k], r['Ps'][k]), float(stats[2 * k]), r['Ss'][k], float(stats[2 * k + 1]),
                 r['Ns'][k], relerr((dws[k] - PW) / 2, r['dws'][k]), relerr((dbs[k] - PB) / 2, r['dbs'][k])))
        assert relerr(probs[k], r['Ps'][k]) < TOL_HEAD
        assert float(stats[2 * k + 1]) == r['Ns'][k] and close(stats[2 * k], r['Ss'][k], TOL_HEAD)
        assert close(term[k], r['Ls'][k], TOL_HEAD)
        assert relerr((dws[k] - PW) / 2, r['dws'][k]) < TOL_HEAD
        assert relerr((dbs[k] - PB) / 2, r['dbs'][k]) < 1e-4
    print("total %.8f ref %.8f dx %.2e / %.2e" % (float(loss), r['total'], relerr(dx, r['dx']),
                                                 relerr(dx2 - 1e-3, r['dx'])))
    assert close(loss, r['total'], 1e-5)
    assert relerr(dx, r['dx']) < TOL_HEAD
    assert relerr(dx2 - 1e-3, r['dx']) < 1e-3
    # the same quantities from the generic route on the same tensors.  (Its logits are the float64
    # products rounded to f32, not a conv launch's; dx, dw and db follow from the generic pair's
    # dlogits by float64 products.)
    lgd = [dev(a) for a in r['lgs']]
    gp = [nan_like(a.shape) for a in r['lgs']]
    gstats = torch.zeros(2 * K, device="cuda")
    ctx.nll_multi_fwd(lgd, td, gp, gstats)
    gcoef, gterm, gcount = (nan_like((8,)) for _ in range(3))
    gloss = nan_like((1,))
    ctx.nll_mix(K, gstats, dev(r['wmix']), gcoef, gterm, gcount, gloss)
    gdl = [nan_like(a.shape) for a in r['lgs']]
    ctx.nll_multi_bwd(gp, td, gcoef, gdl)
    torch.cuda.synchronize()
    assert close(loss, gloss, 1e-5)
    gdx = sum(np.einsum('oc,nodhw->ncdhw', w.astype(np.float64), host(d).astype(np.float64))
              for w, d in zip(r['ws'], gdl))
    assert relerr(dx, gdx) < TOL_HEAD
    x64 = r['xfull'][:, 2:2 + cin].astype(np.float64)
    for k in range(K):                                   # dw / db from the generic dlogits
        g64 = host(gdl[k]).astype(np.float64)
        assert relerr((dws[k] - PW) / 2, np.einsum('nodhw,ncdhw->oc', g64, x64)) < TOL_HEAD
        assert relerr((dbs[k] - PB) / 2, g64.sum(axis=(0, 2, 3, 4))) < 1e-4
    for k in range(K):
        assert relerr(probs[k], host(gp[k])) < TOL_HEAD and float(stats[2 * k + 1]) == float(gstats[2 * k + 1])
        assert close(coef[k], gcoef[k], 1e-5)
    # no data gradient wanted; probabilities only
    dws0 = [torch.zeros(w.shape, device="cuda") for w in r['ws']]
    dbs0 = [torch.zeros(b.shape, device="cuda") for b in r['bs']]
    ctx.multihead_bwd(xd, wd, probs, td, coef, None, False, dws0, dbs0, ws)
    p2 = [nan_like(p.shape) for p in probs]
    keep = stats.clone()
    ctx.multihead_fwd(xd, wd, bd, None, p2, None)
    torch.cuda.synchronize()
    for k in range(K):
        assert relerr(dws0[k], r['dws'][k]) < TOL_HEAD
        assert np.array_equal(bits(p2[k]), bits(probs[k]))
    assert torch.equal(keep, stats)


def _fused_calls_refused(ctx, match=None, cin=16, classes=(3, 4, 3)):
    """forward and backward with these sizes raise and launch nothing"""
    from elektronn2_amd import backend
    n, sp, K = 1, (1, 4, 8), len(classes)
    x = torch.rand((n, cin) + sp, device="cuda")
    ws = [torch.rand(c, cin, device="cuda") for c in classes]
    bs = [torch.rand(c, device="cuda") for c in classes]
    td = [torch.zeros((n, 1) + sp, device="cuda") for _ in classes]
    probs = [torch.full((n, c) + sp, 7.0, device="cuda") for c in classes]
    stats = torch.full((2 * K,), 7.0, device="cuda")
    coef = torch.full((K,), 1.0, device="cuda")
    dx = torch.full((n, cin) + sp, 7.0, device="cuda")
    dws = [torch.full(w.shape, 7.0, device="cuda") for w in ws]
    dbs = [torch.full(b.shape, 7.0, device="cuda") for b in bs]
    ws_buf = torch.full((K * 1024 * (cin + 1) * 4,), 7.0, device="cuda")
    with pytest.raises(backend.E2Error, match=match):
        ctx.multihead_fwd(x, ws, bs, td, probs, stats)
    with pytest.raises(backend.E2Error, match=match):
        ctx.multihead_bwd(x, ws, probs, td, coef, dx, False, dws, dbs, ws_buf)
    torch.cuda.synchronize()
    for t in probs + dws + dbs + [stats, dx, ws_buf]:
        assert float(t.min()) == 7.0 and float(t.max()) == 7.0


def test_fused_pair_refuses_what_it_does_not_support_and_launches_nothing(ctx):
    from elektronn2_amd import backend
    for cin, classes in [(16, (9, 8)), (16, (2,) * 9), (513, (2, 2)), (16, (3, 1)), (16, (4,))]:
        assert not ctx.multihead_supported(cin, classes), (cin, classes)
        _fused_calls_refused(ctx, cin=cin, classes=classes)
    assert ctx.multihead_supported(512, (8, 8)) and ctx.multihead_supported(1, (2, 2))
    # mismatches and a short workspace
    n, sp, cin, classes = 1, (1, 4, 8), 16, (3, 4)
    x = torch.rand((n, cin) + sp, device="cuda")
    ws = [torch.rand(c, cin, device="cuda") for c in classes]
    bs = [torch.rand(c, device="cuda") for c in classes]
    td = [torch.zeros((n, 1) + sp, device="cuda") for _ in classes]
    probs = [torch.full((n, c) + sp, 7.0, device="cuda") for c in classes]
    stats = torch.full((4,), 7.0, device="cuda")
    coef = torch.ones(2, device="cuda")
    dws = [torch.full(w.shape, 7.0, device="cuda") for w in ws]
    dbs = [torch.full(b.shape, 7.0, device="cuda") for b in bs]
    nb = ctx.multihead_bwd_ws_bytes((n, cin) + sp, 7)
    ws_buf = torch.full((nb // 4,), 7.0, device="cuda")
    for kw in (dict(targets=[td[0], td[1][:, :, :, :2]]), dict(targets=[td[0], None]),
               dict(probs=[probs[0], probs[1][:, :, :, :, :4]]), dict(stats=None),
               dict(w=[ws[0], None]), dict(bias=None)):
        a = dict(dict(x=x, w=ws, bias=bs, targets=td, probs=probs, stats=stats), **kw)
        with pytest.raises(backend.E2Error):
            ctx.multihead_fwd(a['x'], a['w'], a['bias'], a['targets'], a['probs'], a['stats'])
    bad_dx = torch.full((n, cin + 1) + sp, 7.0, device="cuda")
    for kw in (dict(targets=None), dict(dx=bad_dx), dict(ws_bytes=nb - 4), dict(ws=None), dict(coef=None),
               dict(dw=[dws[0], None])):
        a = dict(dict(targets=td, dx=None, ws=ws_buf, ws_bytes=None, coef=coef, dw=dws), **kw)
        with pytest.raises(backend.E2Error):
            ctx.multihead_bwd(x, ws, probs, a['targets'], a['coef'], a['dx'], False, a['dw'], dbs, a['ws'],
                              ws_bytes=a['ws_bytes'] if a['ws'] is not None else 0)
    torch.cuda.synchronize()
    for t in probs + dws + dbs + [stats, ws_buf, bad_dx]:
        assert float(t.min()) == 7.0 and float(t.max()) == 7.0


# ---- 2. nets ---------------------------------------------------------------------------------------------
class RefM(Ref):
    """tests/test_activations_gpu.py's float64 restatement, with what a multi-task graph adds: the
    split parts, one sparse NLL per head with its own normaliser, the weighted mean of the terms
    (weights read from the node when the reference runs), Errors on one head."""

    def forward(self, x, t, seed=0, counter=0):
        m = self.model
        self.min_pre, self.n_kinked = np.inf, 0
        val, self.L, self.N = {}, {}, {}
        for node in m.nodes.values():
            kind = type(node).__name__
            par = node.parent
            if node is m.input_node:
                val[node] = torch.tensor(np.asarray(x, np.float64))
            elif node is m.target_node:
                val[node] = torch.tensor(np.asarray(t, np.float64))
            elif kind == 'Conv':
                h, w, b = val[par], self.p(node.w), self.p(node.b)
                nd = h.dim() - 2
                y = (F.conv3d if nd == 3 else F.conv2d)(h, w.flip(*range(2, 2 + nd)))
                if any(q != 1 for q in node.pool_shape):
                    y = (F.max_pool3d if nd == 3 else F.max_pool2d)(y, tuple(node.pool_shape))
                assert not node.batch_normalisation
                y = y + b.view((1, -1) + (1,) * nd)
                val[node] = self.drop(node, self.act(node, y), seed, counter)
            elif kind == 'SplitPart':
                val[node] = val[par][:, node.lo:node.hi]
            elif kind == 'Softmax':
                val[node] = torch.softmax(val[par], dim=1)
            elif kind == 'Concat':
                val[node] = torch.cat([val[q] for q in par], dim=1)
            elif kind == 'MultinoulliNLL':
                pr, tg = val[par[0]], val[par[1]]
                C = pr.shape[1]
                classes = torch.arange(C, dtype=tg.dtype).view((1, C) + (1,) * (pr.dim() - 2))
                onehot = (tg == classes).to(pr.dtype)
                self.N[node.name] = int(onehot.sum())
                val[node] = -(onehot * torch.log(pr + EPS)).sum() / (onehot.sum() + EPS)
                self.L[node.name] = float(val[node].detach())
            elif kind == 'AggregateLoss':
                w = node.mixing_weights.get_value().astype(np.float64)
                val[node] = sum(float(w[k]) * val[q] for k, q in enumerate(par)) / len(par)
            elif kind == '_Errors':
                cls = val[node.cls.pred].detach().argmax(dim=1, keepdim=True)
                gt = val[node.target].to(torch.int16).to(cls.dtype)
                self.err = float((gt != cls).double().mean())
                # positions whose two largest probabilities lie within 1e-3: there a float32
                # argmax may differ from the float64 one, and only there
                top = val[node.cls.pred].detach().topk(2, dim=1).values
                self.err_slack = float(((top[:, 0] - top[:, 1]) <= 1e-3).double().sum()) / gt.numel()
            elif kind == 'Classification':
                continue
            else:
                raise NotImplementedError(kind)
        return val[m.loss_node], val[m.prediction_node]


def multi_net(batch=1, classes=(3, 4, 3), weights=W3, drop_head=None, seed=71, dims=3, loss_last=False):
    """net A (dims = 3): Input (b,1,9,26,26), Conv 8 (1,3,3) pool (1,2,2), Conv 8 (3,3,3), one
    (1,1,1) 'lin' head and Softmax per entry of ``classes`` -- 700 positions per item --, the
    target split K ways, the Concat of the softmaxes as prediction, Errors on head 0.
    net B (dims = 2): the same idea on 'b,f,x,y'."""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    K = len(classes)
    if dims == 3:
        inp = nm.Input((batch, 1, 9, 26, 26), 'b,f,z,x,y', name='raw')
        out = nm.Conv(inp, 8, (1, 3, 3), (1, 2, 2))
        out = nm.Conv(out, 8, (3, 3, 3))
        one = (1, 1, 1)
    else:
        inp = nm.Input((batch, 1, 26, 26), 'b,f,x,y', name='raw')
        out = nm.Conv(inp, 8, (3, 3), (2, 2))
        out = nm.Conv(out, 8, (3, 3))
        one = (1, 1)
    sms = [nm.Softmax(nm.Conv(out, c, one, activation_func='lin', name='head%d' % k,
                              dropout_rate=(drop_head[1] if drop_head and drop_head[0] == k else 0)),
                      name='probs%d' % k) for k, c in enumerate(classes)]
    target = nm.Input_like(sms[0], override_f=K, name='target')
    parts = nm.split(target, 'f', n_out=K)
    nlls = [nm.MultinoulliNLL(s, t, target_is_sparse=True, name='nll%d' % k)
            for k, (s, t) in enumerate(zip(sms, parts))]
    loss = nm.AggregateLoss(nlls, mixing_weights=weights, name='loss')
    pred = nm.Concat(sms, name='pred')
    errors = nm.Errors(sms[0], parts[0], target_is_sparse=True)
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=pred,
                          prediction_ext=[pred, errors, loss] if loss_last else [loss, errors, pred])
    model.set_opt_meta_params('Adam', ADAM)
    model._classes = tuple(classes)
    return model


def batch_for(m, seed):
    rng = np.random.RandomState(seed)
    x = rng.rand(*m.input_node.shape.shape).astype(np.float32)
    t = np.empty(m.target_node.shape.shape, np.float32)
    for k, c in enumerate(m._classes):
        tk = rng.randint(0, c, t[:, k].shape).astype(np.float32)
        tk[rng.rand(*tk.shape) < 0.08 + 0.2 * k] = -1            # clearly different counts
        t[:, k] = tk
    t[0, 0].flat[:5] = 9.0                                       # no class of any head
    return x, t


def rel(a, b):
    return relerr(np.asarray(a), b)


NET_A = dict()
NET_B = dict(dims=2, classes=(3, 2), weights=[1.5, 0.5])
NET_18 = dict(classes=(3, 18, 3))
NET_DROP = dict(drop_head=(1, 0.25))
# name, constructor arguments, batch, plan options, fused route?, seed of the batch (chosen on the
# reference alone: RefM asserts that no relu unit sits at its kink)
NETS = [("A_b1", NET_A, 1, {}, True, 82), ("A_b2", NET_A, 2, {}, True, 81), ("B_2d", NET_B, 2, {}, True, 81),
        ("C_option_off", NET_A, 1, dict(fuse_multihead=False), False, 82),
        ("C_18_classes", NET_18, 1, {}, False, 81), ("C_head_dropout", NET_DROP, 1, {}, False, 81)]


def reference_schedule(kw, batch, data_seed, seed=20260):
    """the reference side of the net test on its own (used on the CPU to choose the data seeds)"""
    m = multi_net(batch, **kw)
    x, t = batch_for(m, data_seed)
    ref = RefM(m)
    worst = np.inf
    drops = bool(m.dropout_nodes())
    for c in range(12 if drops else 1):
        ref.loss_and_grads(x, t, seed, c)
        worst = min(worst, ref.min_pre)
    for step in range(3):
        ref.loss_and_grads(x, t, seed, 12 + step)
        worst = min(worst, ref.min_pre)
        ref.adam(**ADAM)
    return worst


@pytest.mark.parametrize("name,kw,batch,opts,fused,data_seed", NETS, ids=[n[0] for n in NETS])
def test_loss_terms_gradients_errors_and_adam_steps_against_float64(name, kw, batch, opts, fused, data_seed):
    """loss, each term_value / n_labelled, prediction, Errors, EVERY parameter gradient -- eager,
    captured and replayed calls -- and three Adam steps against the float64 step"""
    from elektronn2_amd.neuromancer import plan_options
    with plan_options(**opts):
        m = multi_net(batch, **kw)
        nlls = list(m.loss_node.parent)
        assert all(n.term_value is None and n.n_labelled is None for n in nlls)
        x, t = batch_for(m, data_seed)
        ref = RefM(m)
        seed = 20260
        drops = bool(m.dropout_nodes())
        if drops:
            m.set_dropout_seed(seed)
        counter = lambda: m.dropout_state()['counter'] if drops else 0

        def terms_ok():
            for n in nlls:
                assert n.n_labelled == ref.N[n.name], (n.name, n.n_labelled, ref.N[n.name])
                assert close(n.term_value, ref.L[n.name], TOL), (n.name, n.term_value, ref.L[n.name])

        for call in range(3):                                   # eager, capture, replay
            lref, pref = ref.loss_and_grads(x, t, seed, counter())
            loss = float(m.loss(x, t))
            print("%s call %d: loss %.7f ref %.7f terms %s counts %s (kinked closest %.1e)"
                  % (name, call, loss, lref, [float(n.term_value) for n in nlls],
                     [n.n_labelled for n in nlls], ref.min_pre))
            assert close(loss, lref, TOL), (call, loss, lref)
            terms_ok()
            lref, pref = ref.loss_and_grads(x, t, seed, counter())
            assert rel(m.predict(x), pref) < TOL
            lref, pref = ref.loss_and_grads(x, t, seed, counter())
            l2, err, pr = m.predict_ext(x, t)
            assert close(l2, lref, TOL) and rel(pr, pref) < TOL
            # Errors, on every call: equal to the reference's up to one count per position that
            # the REFERENCE has within 1e-3 of a tie (a few of 700 per item; never all of them)
            print("%s call %d: errors %.6f ref %.6f (near ties allow %.6f)"
                  % (name, call, float(err), ref.err, ref.err_slack))
            assert ref.err_slack <= 0.02
            assert abs(float(err) - ref.err) <= ref.err_slack + 1e-6
            ref.loss_and_grads(x, t, seed, counter())
            got = m.gradients(x, t)
            names = list(m.loss_node.all_trainable_params.keys())
            want = ref.grads()
            assert len(got) == len(want) == len(names)
            errs = dict((nme, rel(g, w)) for nme, g, w in zip(names, got, want))
            print("%s call %d: gradients, worst %s" % (name, call, sorted(errs.items(), key=lambda kv: -kv[1])[:3]))
            for nme, g, w in zip(names, got, want):
                assert np.abs(w).max() > 0, nme
                assert errs[nme] < TOL, (call, nme, errs[nme])
        for step in range(3):                                   # Adam: eager, captured, replayed
            lref, _ = ref.loss_and_grads(x, t, seed, counter())
            ref.adam(**ADAM)
            loss = float(m.trainingstep(x, t, optimiser='Adam')[0])
            assert close(loss, lref, TOL), (step, loss, lref)
            terms_ok()
            worst = ('', 0.0)
            for nme, p in m.loss_node.all_trainable_params.items():
                e = rel(p.get_value(), ref.p(p).detach().numpy())
                worst = max(worst, (nme, e), key=lambda kv: kv[1])
                assert e < TOL, (step, nme, e)
            print("%s step %d: loss %.7f ref %.7f, parameters worst %s" % (name, step, loss, lref, worst))
        plan = m.optimisers['Adam'].step.func
        assert plan._graphs, "the step was not captured"
        assert (m.loss_node._fused_heads(plan) is not None) == fused
        assert plan._labelled_count() is None
        assert m.prediction_node.shape.shape[1] == sum(m._classes)


@pytest.mark.parametrize("opts", [{}, dict(fuse_multihead=False)], ids=["fused", "generic"])
def test_readers_of_the_probabilities_come_behind_the_launch_that_writes_them(opts):
    """a prediction_ext list that names the Concat and Errors BEFORE the loss: the forward launch
    stands at the last softmax, so both read this call's probabilities (the buffers start as NaN
    and every call has another batch: a read of anything else would show)"""
    from elektronn2_amd.neuromancer import plan_options
    with plan_options(debug_poison=True, **opts):
        m = multi_net(loss_last=True)
        ref = RefM(m)
        for call, seed in enumerate((82, 83, 84)):               # eager, captured, replayed:
            x, t = batch_for(m, seed)                            # another batch each time
            lref, pref = ref.loss_and_grads(x, t)
            pr, err, loss = m.predict_ext(x, t)
            assert close(loss, lref, TOL) and rel(pr, pref) < TOL, call
            assert abs(float(err) - ref.err) <= ref.err_slack + 1e-6, call


def _entry_points_of_one_eager_step(m, x, t, monkeypatch):
    """as tests/test_lrn_gpu.py records them"""
    from elektronn2_amd import backend
    from elektronn2_amd.neuromancer import plan_options
    calls = []
    orig = backend._chk
    with plan_options(graph=False):
        m.trainingstep(x, t, optimiser='Adam')              # builds the plan, tunes
        m.trainingstep(x, t, optimiser='Adam')
        monkeypatch.setattr(backend, '_chk', lambda rc, what: (calls.append(what), orig(rc, what))[1])
        m.trainingstep(x, t, optimiser='Adam')
        monkeypatch.setattr(backend, '_chk', orig)
    skip = ('e2_event', 'e2_stream', 'e2_last_launch', 'e2_set_', 'e2_conv_last_zero_fill')
    return [c[:-len('_parts')] if c.endswith('_parts') else c for c in calls if not c.startswith(skip)]


def test_launch_lists_of_the_fused_and_the_generic_route(monkeypatch):
    from elektronn2_amd.neuromancer import plan_options
    m = multi_net()
    x, t = batch_for(m, 81)
    fused = _entry_points_of_one_eager_step(m, x, t, monkeypatch)
    print("fused:", fused)
    for name in ('e2_multihead_fwd', 'e2_nll_mix', 'e2_multihead_bwd'):
        assert fused.count(name) == 1, name
    assert not any(c.startswith(('e2_head_', 'e2_softmax_nll', 'e2_nll_multi')) for c in fused)
    with plan_options(fuse_multihead=False):
        g = multi_net()
        generic = _entry_points_of_one_eager_step(g, x, t, monkeypatch)
    print("generic:", generic)
    for name in ('e2_nll_multi_fwd', 'e2_nll_mix', 'e2_nll_multi_bwd'):
        assert generic.count(name) == 1, name
    assert not any(c.startswith(('e2_head_', 'e2_softmax_nll', 'e2_multihead')) for c in generic)
    # no conv launch for the head nodes: the fused step is the generic step without the launches
    # of three (1,1,1) 'lin' convs (forward, weight gradient, data gradient, bias passes)
    convs = lambda calls: [c for c in calls if c.startswith(('e2_conv', 'e2_pool_bias_act', 'e2_bias_act'))]
    trunk = convs(fused)
    assert len(convs(generic)) >= len(trunk) + 3 * 3
    # ... and what is left is the step of the same trunk under ONE head of the existing route
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(71)
    inp = nm.Input((1, 1, 9, 26, 26), 'b,f,z,x,y', name='raw')
    out = nm.Conv(nm.Conv(inp, 8, (1, 3, 3), (1, 2, 2)), 8, (3, 3, 3))
    sm = nm.Softmax(nm.Conv(out, 3, (1, 1, 1), activation_func='lin'))
    tg = nm.Input_like(sm, override_f=1, name='target')
    single = nm.model_manager.getmodel()
    single.designate_nodes(input_node=inp, target_node=tg, prediction_node=sm,
                           loss_node=nm.AggregateLoss(nm.MultinoulliNLL(sm, tg, target_is_sparse=True)))
    single.set_opt_meta_params('Adam', ADAM)
    one = _entry_points_of_one_eager_step(single, x, t[:, :1], monkeypatch)
    print("one head:", one)
    assert one.count('e2_head_fwd') == 1 and one.count('e2_head_bwd') == 1
    assert convs(one) == trunk


def test_a_split_part_that_needs_a_gradient_is_refused_when_the_step_is_planned():
    """parts of a Conv's output on the loss path: outside this work, and said so"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(3)
    inp = nm.Input((1, 1, 3, 12, 12), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 6, (1, 3, 3), activation_func='lin')
    sms = [nm.Softmax(p) for p in nm.split(out, n_out=2)]
    target = nm.Input_like(sms[0], override_f=2, name='target')
    nlls = [nm.MultinoulliNLL(s, t, target_is_sparse=True) for s, t in zip(sms, nm.split(target, n_out=2))]
    m = nm.model_manager.getmodel()
    m.designate_nodes(input_node=inp, target_node=target, loss_node=nm.AggregateLoss(nlls),
                      prediction_node=sms[0])
    x = np.random.rand(1, 1, 3, 12, 12).astype(np.float32)
    t = np.random.randint(0, 3, (1, 2, 3, 10, 10)).astype(np.float32)
    with pytest.raises(NotImplementedError, match="needs a gradient"):
        m.trainingstep(x, t, optimiser='Adam')


# ---- 3. the model protocol ---------------------------------------------------------------------------------
def _batches(m, n, seed=90):
    return [batch_for(m, seed + i) for i in range(n)]


def _params(m):
    return [p.get_value() for p in m.loss_node.all_trainable_params.values()]


def test_new_mixing_weights_reach_the_next_replayed_step_without_a_new_capture():
    m = multi_net()
    x, t = batch_for(m, 82)
    ref = RefM(m)
    for _ in range(2):                                       # eager, capture
        lref, _ = ref.loss_and_grads(x, t)
        ref.adam(**ADAM)
        assert close(m.trainingstep(x, t, optimiser='Adam')[0], lref, TOL)
    plan = m.optimisers['Adam'].step.func
    graphs = list(plan._graphs)
    before = float(lref)
    m.loss_node.params['mixing_weights'].set_value(np.array([0.2, 2.5, 0.3], np.float32))
    lref, _ = ref.loss_and_grads(x, t)                       # (RefM reads the node's weights)
    ref.adam(**ADAM)
    loss = float(m.trainingstep(x, t, optimiser='Adam')[0])
    print("loss %.7f ref %.7f (before the new weights %.7f)" % (loss, lref, before))
    assert abs(lref - before) > 0.05 * before and close(loss, lref, TOL)
    assert plan._graphs == graphs, "the step was captured again"
    for nme, p in m.loss_node.all_trainable_params.items():
        assert rel(p.get_value(), ref.p(p).detach().numpy()) < TOL, nme


def test_graph_replay_equals_eager_for_three_steps():
    runs = []
    for use_graph in (True, False):
        m = multi_net()
        bs = _batches(m, 3)
        opt = m.optimisers['Adam']
        opt.step.compile()
        opt.step.func.use_graph = use_graph
        assert all(n.term_value is None and n.n_labelled is None for n in m.loss_node.parent)
        losses = [float(m.trainingstep(x, t, optimiser='Adam')[0]) for x, t in bs]
        assert bool(opt.step.func._graphs) == use_graph
        runs.append((losses, _params(m)))
    (lg, pg), (le, pe) = runs
    for a, b in zip(lg, le):
        assert close(a, b, 1e-5), (lg, le)
    for a, b in zip(pg, pe):
        assert rel(a, b) < 1e-4


def test_trainingsteps_from_a_ring_returns_the_losses_of_single_steps():
    a = multi_net()
    bs = _batches(a, 3)
    single = [float(a.trainingstep(*bs[i % 3], optimiser='Adam')[0]) for i in range(5)]
    c = multi_net()
    for i in range(2):                                       # eager + capture (builds the plan)
        c.trainingstep(*bs[i], optimiser='Adam')
    pl = c.optimisers['Adam'].step.func
    ring = torch.empty((3, pl.input_arena.numel()), device='cuda')
    for i in range(3):                                       # the step after the two above reads slot 0
        for n, v in zip(c.loss_node.input_nodes, bs[(2 + i) % 3]):
            o, cnt = pl.input_slices[n]
            ring[i, o:o + cnt] = dev(v).reshape(-1)
    losses, tsec = c.trainingsteps(3, optimiser='Adam', ring=ring)
    assert len(losses) == 3
    for u, v in zip(single[2:5], losses):
        assert close(float(v), u, 1e-5), (single, list(losses))
    for u, v in zip(_params(a), _params(c)):
        assert rel(v, u) < 1e-4


def test_checkpoint_after_two_steps_resumes_to_the_same_third_step(tmp_path):
    from elektronn2_amd.neuromancer.model import modelload
    a = multi_net()
    x, t = batch_for(a, 81)
    for _ in range(2):
        a.trainingstep(x, t, optimiser='Adam')
    f = str(tmp_path / "multi.mdl")
    a.save(f)
    saved = _params(a)
    third = float(a.trainingstep(x, t, optimiser='Adam')[0])
    end_p = _params(a)
    b = multi_net(seed=99)                                   # other weights, nothing on the device
    modelload(f, b)
    for v, p in zip(saved, _params(b)):
        assert np.array_equal(v, p)                          # bit-equal
    got = float(b.trainingstep(x, t, optimiser='Adam')[0])
    assert close(got, third, 2e-6), (third, got)             # tests/test_checkpoint.py:171-185
    for v, p in zip(end_p, _params(b)):
        assert np.abs(v - p).max() <= 1e-5 * np.abs(v).max()
    c = modelload(f)                                         # the graph rebuilt from the file alone
    assert c.loss_node.multi_nll and len(c.loss_node.parent) == 3
    assert np.allclose(c.loss_node.params['mixing_weights'].get_value(), W3)
    b2 = multi_net(seed=98)
    modelload(f, b2)
    assert close(float(c.loss(x, t)), float(b2.loss(x, t)), 1e-6)


@pytest.fixture()
def process_bf16():
    import elektronn2_amd
    elektronn2_amd.set_mfma_dtype('bf16')
    yield
    elektronn2_amd.set_mfma_dtype('f32')


def test_one_bf16_step_stays_close_to_the_float64_loss(process_bf16):
    """tests/test_bf16_gpu.py:145: a small net's loss in bf16 operand mode within 1e-2"""
    m = multi_net()
    x, t = batch_for(m, 82)
    lref, _ = RefM(m).loss_and_grads(x, t)
    loss = float(m.trainingstep(x, t, optimiser='Adam')[0])
    print("bf16 loss %.7f, float64 of the f32 net %.7f" % (loss, lref))
    assert np.isfinite(loss) and abs(loss - lref) < 1e-2 * abs(lref)
