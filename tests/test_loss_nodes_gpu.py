"""EuclideanDistance / RampLoss / BetaNLL / OneHot and the mean of a loss map on the GPU
(csrc/loss_map.hip, csrc/loss_elem.hip; loss.py:96-138, 890-950, 1104-1212, 1346-1363).

The reference of every comparison is the float64 torch-CPU restatement of
tests/test_loss_nodes_host.py (pinned there to plain loops), differentiated by autograd, on the
float32 inputs the kernels saw.  Bounds are the project's own (tests/test_regression_loss_gpu.py:
24-26): ops at 2e-5 of the reference's largest magnitude, a loss value at 1e-5 relative, whole
steps -- loss, every gradient, parameters after Adam -- at 1e-4; counts and one-hot outputs exact.
Every operand and every output of the op tests is a strided view inside NaN-filled watched storage
(tests/strided_views.py, the VIEWS of tests/test_dropout_gpu.py): no bit around a view may change."""
import numpy as np
import pytest
import torch

import strided_views as SV
from test_activations_gpu import ADAM
from test_dropout_gpu import VIEWS, SHAPES
from test_regression_loss_gpu import (RefL, TOL, TOL_LOSS, TOL_STEP, rel, dev, bits, t64, close, _done,
                                      _trunk, is_masked)
from test_regression_loss_host import ref_squared, ref_binary, ref_aggregate
from test_loss_nodes_host import (ref_fdist, ref_ramp, ref_beta, ref_onehot, fdist_inputs, ramp_inputs,
                                  ramp_gap, beta_inputs, grads_of)

pytestmark = pytest.mark.gpu
f32 = np.float32

# features 1, 2, 3, 5, 7, 17; row widths 1, 3, 4, 5, 7, 8, 13, 16, 34; the last: 7040 positions = 4 slab rows
OP_SHAPES = SHAPES + [(1, 17, 1, 6, 4), (2, 2, 2, 3, 5), (1, 3, 4, 40, 44)]
HOW = ["dense", "frame111", "cslice", "odd_base", "cslice_frame", "padded_rows", "crop", "mixed"]
MIX = ["cslice", "frame111", "odd_base", "dense", "padded_rows", "frame022"]
MARGIN = float(f32(0.5))


def one_feature(shape):
    return (shape[0], 1) + tuple(shape[2:])


class Watched(object):
    """views inside NaN-filled storage; ``check`` compares every bit outside the views (and, for
    the views named read-only, inside) with what it was"""

    def __init__(self, how):
        self.how, self.k, self.items = how, 0, []

    def place(self, shape, data=None, read_only=False):
        how = MIX[self.k % len(MIX)] if self.how == "mixed" else self.how
        self.k += 1
        if how in SV.GEOMS:
            storage, view, _, mask = SV.make_view(shape, how, 7 + self.k)
        else:
            storage, view = dict(VIEWS)[how](shape)
            storage.fill_(0.0); view.fill_(1.0)
            mask = storage == 0
        storage.fill_(float('nan'))
        if data is not None:
            view.copy_(dev(data))
        if read_only:
            mask = torch.ones_like(mask)
        self.items.append((storage, storage.clone(), mask))
        return view

    def check(self):
        for storage, clone, mask in self.items:
            SV.assert_outside_untouched(storage, clone, mask)


_REF = {}


def cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def seed_of(shape, salt):
    return (salt * 1009 + int(np.dot(shape, [1, 7, 49, 343, 2401]))) % (2 ** 31)


# ---- 1. the kernels through the C ABI ------------------------------------------------------------------
def fdist_ref(shape):
    def make():
        rng = np.random.RandomState(seed_of(shape, 1))
        p, t = fdist_inputs(rng, shape)
        dout = rng.randn(*one_feature(shape)).astype(f32)
        tp, tt = t64(p, True), t64(t, True)
        out = ref_fdist(tp, tt)
        gp, gt = grads_of(out, dout, [tp, tt])
        g0 = (rng.randn(*shape) * max(np.abs(gp).max(), 1e-3)).astype(f32)
        return p, t, dout, out.detach().numpy(), gp, gt, g0
    return cached(("fdist", shape), make)


def ramp_ref(shape):
    def make():
        rng = np.random.RandomState(seed_of(shape, 2))
        lo, big = ramp_inputs(rng, shape, MARGIN)
        assert ramp_gap(lo, big, MARGIN) >= 1e-3
        dout = rng.randn(*one_feature(shape)).astype(f32)
        tl, tb = t64(lo, True), t64(big, True)
        out = ref_ramp(tl, tb, MARGIN)
        gl, gb = grads_of(out, dout, [tl, tb])
        g0 = (rng.randn(*shape) * max(np.abs(gl).max(), 1e-3)).astype(f32)
        return lo, big, dout, out.detach().numpy(), gl, gb, g0
    return cached(("ramp", shape), make)


def _check_pair_bwd(how, shape, launch, ga, gb, g0, sources):
    """the six forms of a two-output backward: both flags equal, both differ, either output NULL"""
    for acc_a, acc_b, want_a, want_b in ((False, False, True, True), (True, True, True, True),
                                         (False, True, True, True), (True, False, True, True),
                                         (True, None, True, False), (None, False, False, True)):
        w = Watched(how)
        src = [w.place(a.shape, a, read_only=True) for a in sources]
        da = w.place(shape, g0) if want_a else None
        db = w.place(shape, g0) if want_b else None
        launch(src, da, db, bool(acc_a), bool(acc_b))
        for view, acc, g in ((da, acc_a, ga), (db, acc_b, gb)):
            if view is None:
                continue
            got = view.cpu().numpy()
            want = (g0.astype(np.float64) if acc else 0.0) + g
            assert np.all(np.isfinite(got)), (shape, acc_a, acc_b)
            assert rel(got, want) < TOL, (shape, acc_a, acc_b, rel(got, want))
        w.check()


@pytest.mark.parametrize("how", HOW)
def test_fdist_through_the_c_abi(ctx, how):
    for shape in OP_SHAPES:
        p, t, dout, out, gp, gt, g0 = fdist_ref(shape)
        w = Watched(how)
        pv, tv = w.place(shape, p, read_only=True), w.place(shape, t, read_only=True)
        ov = w.place(one_feature(shape))
        ctx.fdist_fwd(pv, tv, ov)
        got = ov.cpu().numpy()
        assert np.all(np.isfinite(got)) and rel(got, out) < TOL, (shape, rel(got, out))
        w.check()
        # the backward reads the map the forward stored (float32)
        _check_pair_bwd(how, shape,
                        lambda s, da, db, aa, ab: ctx.fdist_bwd(s[0], s[1], s[2], s[3], da, db, aa, ab),
                        gp, gt, g0, [p, t, got, dout])


@pytest.mark.parametrize("how", HOW)
def test_ramp_through_the_c_abi(ctx, how):
    margin = dev([MARGIN])
    for shape in OP_SHAPES:
        lo, big, dout, out, gl, gb, g0 = ramp_ref(shape)
        w = Watched(how)
        lv, bv = w.place(shape, lo, read_only=True), w.place(shape, big, read_only=True)
        ov = w.place(one_feature(shape))
        ctx.ramp_fwd(lv, bv, margin, ov)
        got = ov.cpu().numpy()
        assert np.all(np.isfinite(got)) and rel(got, out) < TOL, (shape, rel(got, out))
        w.check()
        _check_pair_bwd(how, shape,
                        lambda s, da, db, aa, ab: ctx.ramp_bwd(s[0], s[1], margin, s[2], da, db, aa, ab),
                        gl, gb, g0, [lo, big, dout])
    assert margin.item() == MARGIN


def mix_one(ctx, slab, n_tot, wgt):
    """e2_loss_mix over one slab under the GAUSS_NLL-kind descriptor -> (total, L, count, coef tensor)"""
    from elektronn2_amd import backend
    coef, tl, cnt = (torch.full((8,), -3.0, device='cuda') for _ in range(3))
    out = torch.full((1,), -3.0, device='cuda')
    ctx.loss_mix([backend.loss_term('gauss_nll')], [slab], [n_tot], dev([wgt]), coef, tl, cnt, out)
    return out.item(), tl[0].item(), cnt[0].item(), coef


@pytest.mark.parametrize("how", HOW)
def test_mean_of_a_map_through_the_c_abi(ctx, how):
    wgt = 0.7
    for shape in OP_SHAPES:
        rng = np.random.RandomState(seed_of(shape, 3))
        x = (rng.rand(*shape) * 2).astype(f32)
        n_tot = x.size
        L = float(x.astype(np.float64).mean())
        w = Watched(how)
        xv = w.place(shape, x, read_only=True)
        rows = ctx.loss_partials(xv)
        slab = torch.full((4 * rows + 8,), float('nan'), device='cuda')
        ctx.mean_fwd(xv, slab[:4 * rows])
        assert torch.isnan(slab[4 * rows:]).all() and not torch.isnan(slab[:4 * rows]).any()
        total, tl, cnt, coef = mix_one(ctx, slab[:4 * rows], n_tot, wgt)
        assert close(tl, L, TOL_LOSS) and close(total, wgt * L, TOL_LOSS), (shape, tl, L)
        assert cnt == n_tot and close(coef[0].item(), wgt / n_tot, 1e-6), (shape, cnt, n_tot)
        for acc in (False, True):
            g0 = rng.randn(*shape).astype(f32)
            dv = w.place(shape, g0)
            ctx.mean_bwd(coef[0:1], dv, accumulate=acc)
            c = f32(coef[0].item())
            want = (g0 + c) if acc else np.full(shape, c, f32)
            assert np.array_equal(bits(dv.cpu().numpy()), bits(want)), (shape, acc)
        w.check()


def beta_ref(shape):
    def make():
        rng = np.random.RandomState(seed_of(shape, 4))
        m, c, x = beta_inputs(rng, shape)
        tm, tc = t64(m, True), t64(c, True)
        L = ref_beta(tm, tc, t64(x)).mean()
        wgt = 0.7
        gm, gc = [g.numpy() for g in torch.autograd.grad(wgt * L, [tm, tc])]
        g0 = (rng.randn(*shape) * max(np.abs(gm).max(), 1e-3)).astype(f32)
        return m, c, x, float(L.detach()), wgt, gm, gc, g0
    return cached(("beta", shape), make)


@pytest.mark.parametrize("how", HOW)
def test_beta_nll_through_the_c_abi(ctx, how):
    for shape in OP_SHAPES:
        m, c, x, L, wgt, gm, gc, g0 = beta_ref(shape)
        w = Watched(how)
        mv, cv, xv = (w.place(shape, a, read_only=True) for a in (m, c, x))
        rows = ctx.loss_partials(mv)
        slab = torch.full((4 * rows,), float('nan'), device='cuda')
        ctx.beta_nll_fwd(mv, cv, xv, slab)
        total, tl, cnt, coef = mix_one(ctx, slab, m.size, wgt)
        assert np.isfinite(total) and close(tl, L, TOL_LOSS) and close(total, wgt * L, TOL_LOSS), (shape, tl, L)
        assert cnt == m.size and close(coef[0].item(), wgt / m.size, 1e-6)
        for acc, want_m, want_c in ((False, True, True), (True, True, True), (False, True, False),
                                    (True, False, True)):
            dm = w.place(shape, g0) if want_m else None
            dc = w.place(shape, g0) if want_c else None
            ctx.beta_nll_bwd(mv, cv, xv, coef[0:1], dm, dc, accumulate=acc)
            for view, g in ((dm, gm), (dc, gc)):
                if view is not None:
                    got = view.cpu().numpy()
                    want = (g0.astype(np.float64) if acc else 0.0) + g
                    assert np.all(np.isfinite(got)) and rel(got, want) < TOL, (shape, acc, rel(got, want))
        w.check()


@pytest.mark.parametrize("how", HOW)
def test_onehot_through_the_c_abi(ctx, how):
    for shape in OP_SHAPES:
        n_class = shape[1]
        rng = np.random.RandomState(seed_of(shape, 5))
        ids = rng.randint(0, n_class, one_feature(shape)).astype(f32)
        odd = np.array([-1.0, 2.5, np.nan, n_class, n_class + 3, 0.5, -0.0], f32)
        k = min(ids.size // 2, odd.size)
        ids.flat[rng.permutation(ids.size)[:k]] = odd[:k]
        want = ref_onehot(torch.from_numpy(ids.astype(np.float64)), n_class).numpy().astype(f32)
        w = Watched(how)
        tv = w.place(one_feature(shape), ids, read_only=True)
        ov = w.place(shape)
        ctx.onehot(tv, ov)
        assert np.array_equal(bits(ov.cpu().numpy()), bits(want)), shape
        w.check()


def test_planted_onehot_ids_give_zero_columns(ctx):
    ids = np.array([0, 1, 2, 3, -1, 2.5, np.nan, 4, 1, 0, 3, 3], f32).reshape(1, 1, 1, 2, 6)
    out = torch.full((1, 4, 1, 2, 6), 9.0, device='cuda')
    ctx.onehot(dev(ids), out)
    got = out.cpu().numpy()
    want = (ids == np.arange(4, dtype=f32).reshape(1, 4, 1, 1, 1)).astype(f32)
    assert np.array_equal(bits(got), bits(want))
    assert got.reshape(4, 12)[:, 4:8].sum() == 0 and got.sum() == 8


def test_bad_arguments_are_errors(ctx):
    from elektronn2_amd import backend
    x3 = torch.rand((1, 3, 2, 4, 5), device='cuda')
    x1 = torch.rand((1, 1, 2, 4, 5), device='cuda')
    y3 = torch.rand((1, 3, 2, 4, 6), device='cuda')
    one = dev([1.0])
    slab = torch.zeros(4, device='cuda')
    with pytest.raises(backend.E2Error, match="size mismatch"):
        ctx.fdist_fwd(x3, y3, x1)
    with pytest.raises(backend.E2Error, match="size mismatch"):
        ctx.fdist_fwd(x3, x3, x3)                           # the map has one feature
    with pytest.raises(backend.E2Error, match="no gradient view"):
        ctx.fdist_bwd(x3, x3, x1, x1, None, None)
    with pytest.raises(backend.E2Error, match="size mismatch"):
        ctx.ramp_fwd(x3, x1, one, x1)
    with pytest.raises(backend.E2Error, match="no gradient view"):
        ctx.ramp_bwd(x3, x3, one, x1, None, None)
    with pytest.raises(backend.E2Error, match="size mismatch"):
        ctx.onehot(x3, x3)                                  # the ids have one feature
    with pytest.raises(backend.E2Error, match="size mismatch"):
        ctx.beta_nll_fwd(x3, x3, y3, slab)
    with pytest.raises(backend.E2Error, match="no gradient view"):
        ctx.beta_nll_bwd(x3, x3, x3, one, None, None)
    with pytest.raises(backend.E2Error, match="too small"):
        ctx.mean_fwd(x3, slab[:0])
    with pytest.raises(backend.E2Error, match="too small"):
        ctx.beta_nll_fwd(x3, x3, x3, slab[:0])


# ---- 2. planted values -------------------------------------------------------------------------------------
def test_planted_zero_distance_and_nan(ctx):
    """pred == target over all features: value 0, gradients exactly 0; a NaN in one feature: value 0,
    gradients exactly 0 at that position; the neighbours as the reference; nothing non-finite"""
    rng = np.random.RandomState(11)
    shape = (2, 3, 2, 3, 9)
    p, t = fdist_inputs(rng, shape)
    zero = [(0, 0, 0, 0), (0, 1, 2, 8), (1, 0, 1, 4)]
    nan = [(0, 0, 0, 1), (1, 1, 2, 7)]
    for n, z, y, x in zero:
        p[n, :, z, y, x] = t[n, :, z, y, x]
    p[0, 1, 0, 0, 1] = np.nan
    t[1, 2, 1, 2, 7] = np.nan
    dout = rng.randn(*one_feature(shape)).astype(f32)
    tp, tt = t64(p, True), t64(t, True)
    ref = ref_fdist(tp, tt)
    gp, gt = grads_of(ref, dout, [tp, tt])
    out = torch.full(one_feature(shape), 5.0, device='cuda')
    ctx.fdist_fwd(dev(p), dev(t), out)
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got)) and rel(got, ref.detach().numpy()) < TOL
    for acc in (False, True):
        dp = torch.full(shape, 2.0, device='cuda')
        dt = torch.full(shape, 2.0, device='cuda')
        ctx.fdist_bwd(dev(p), dev(t), out, dev(dout), dp, dt, acc, acc)
        a, b = dp.cpu().numpy(), dt.cpu().numpy()
        base = 2.0 if acc else 0.0
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
        assert rel(a, base + gp) < TOL and rel(b, base + gt) < TOL
        for n, z, y, x in zero + nan:
            assert got[n, 0, z, y, x] == 0
            assert np.all(a[n, :, z, y, x] == f32(base)) and np.all(b[n, :, z, y, x] == f32(base))


def test_planted_ramp_zero_and_nan(ctx):
    """r == 0 exactly (dyadic values): value 0, slope 1/F; NaN: value 0, slope 0; r < 0: slope 0"""
    F = 4
    lo = np.array([0.25, 1.0, -1.0, np.nan], f32).reshape(1, F, 1, 1, 1) * np.ones((1, F, 1, 2, 5), f32)
    big = np.array([0.75, 0.5, 0.0, 0.0], f32).reshape(1, F, 1, 1, 1) * np.ones((1, F, 1, 2, 5), f32)
    out = torch.full((1, 1, 1, 2, 5), 5.0, device='cuda')
    margin = dev([0.5])
    ctx.ramp_fwd(dev(lo), dev(big), margin, out)
    assert np.array_equal(out.cpu().numpy(), np.full((1, 1, 1, 2, 5), 0.25, f32))       # (0 + 1 + 0 + 0) / 4
    dl, db = (torch.full(lo.shape, 9.0, device='cuda') for _ in range(2))
    ctx.ramp_bwd(dev(lo), dev(big), margin, torch.ones_like(out), dl, db)
    a = dl.cpu().numpy()
    assert np.array_equal(a[0, :, 0, 0, 0], np.array([0.25, 0.25, 0.0, 0.0], f32))
    assert np.array_equal(db.cpu().numpy(), -a)
    tl, tb = t64(lo, True), t64(big, True)
    gl, gb = grads_of(ref_ramp(tl, tb, 0.5), np.ones((1, 1, 1, 2, 5), f32), [tl, tb])
    assert np.array_equal(a.astype(np.float64), gl)


def test_past_the_row_cap(ctx):
    """(1,1,9,512,512): 1152 work-groups' worth of elements, the slab is capped at 1024 rows"""
    shape = (1, 1, 9, 512, 512)
    rng = np.random.RandomState(12)
    p, t = fdist_inputs(rng, shape)
    out = torch.empty(shape, device='cuda')
    ctx.fdist_fwd(dev(p), dev(t), out)
    ref = np.abs(t.astype(np.float64) - p.astype(np.float64))
    assert rel(out.cpu().numpy(), ref) < TOL
    assert ctx.loss_partials(out) == 1024
    slab = torch.full((4 * 1024,), float('nan'), device='cuda')
    ctx.mean_fwd(out, slab)
    total, tl, cnt, coef = mix_one(ctx, slab, p.size, 1.0)
    assert close(tl, ref.mean(), TOL_LOSS) and cnt == p.size
    m, c, x = beta_inputs(rng, shape)
    slab.fill_(float('nan'))
    ctx.beta_nll_fwd(dev(m), dev(c), dev(x), slab)
    total, tl, cnt, coef = mix_one(ctx, slab, p.size, 1.0)
    L = float(ref_beta(t64(m), t64(c), t64(x)).mean())
    assert close(tl, L, TOL_LOSS) and cnt == p.size, (tl, L)
    dm, dc = torch.empty(shape, device='cuda'), torch.empty(shape, device='cuda')
    ctx.beta_nll_bwd(dev(m), dev(c), dev(x), coef[0:1], dm, dc)
    tm, tc = t64(m, True), t64(c, True)
    gm, gc = [g.numpy() for g in torch.autograd.grad(ref_beta(tm, tc, t64(x)).mean(), [tm, tc])]
    assert rel(dm.cpu().numpy(), gm) < TOL and rel(dc.cpu().numpy(), gc) < TOL


# ---- 3. reproducibility -------------------------------------------------------------------------------------
def test_slab_sums_are_bit_reproducible(ctx):
    rng = np.random.RandomState(13)
    shape = (2, 3, 20, 64, 66)
    m, c, x = (dev(a) for a in beta_inputs(rng, shape))
    d = dev(np.abs(rng.randn(*one_feature(shape))))
    s1 = torch.empty(4 * ctx.loss_partials(m), device='cuda')
    s2 = torch.empty(4 * ctx.loss_partials(d), device='cuda')
    assert s1.numel() == 4 * 248 and s2.numel() == 4 * 83
    from elektronn2_amd import backend
    terms = [backend.loss_term('gauss_nll')] * 2
    seen = []
    for run in range(3):
        coef, tl, cnt = (torch.zeros(8, device='cuda') for _ in range(3))
        out = torch.zeros(1, device='cuda')
        s1.fill_(float(run)); s2.fill_(float(run))          # (needs no zero fill: every row is stored)
        ctx.beta_nll_fwd(m, c, x, s1)
        ctx.mean_fwd(d, s2)
        ctx.loss_mix(terms, [s1, s2], [m.numel(), d.numel()], dev([1.0, 0.25]), coef, tl, cnt, out)
        seen.append((bits(out.cpu().numpy()).tolist(), bits(tl.cpu().numpy()).tolist(),
                     bits(s1.cpu().numpy()).tolist(), bits(s2.cpu().numpy()).tolist()))
        assert cnt[0].item() == m.numel() and cnt[1].item() == d.numel()
    assert seen[0] == seen[1] == seen[2]


# ---- 4. nodes on every layout ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tags,shape", [('b,f,z,x,y', (2, 3, 2, 5, 6)), ('b,f,x,y', (2, 3, 8, 9)),
                                        ('b,f,y,x', (2, 3, 8, 9)), ('b,f', (4, 5))])
def test_nodes_compute_on_every_layout(tags, shape):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    rng = np.random.RandomState(14)
    a, b = nm.Input(shape, tags, name='a'), nm.Input(shape, tags, name='b')
    ed = nm.EuclideanDistance(a, b)
    rl = nm.RampLoss(a, b, margin=0.5)
    oh = nm.OneHot(nm.Input(shape[:1] + (1,) + shape[2:], tags, name='ids'), shape[1])
    loss = nm.AggregateLoss([ed, rl], mixing_weights=[1.0, 0.5])
    xa, xb = ramp_inputs(rng, shape, 0.5)
    ids = rng.randint(0, shape[1], shape[:1] + (1,) + shape[2:]).astype(f32)
    got = ed(xa, xb)
    want = ref_fdist(t64(xa), t64(xb)).numpy()
    assert got.shape == want.shape and rel(got, want) < TOL
    assert rel(rl(xa, xb), ref_ramp(t64(xa), t64(xb), 0.5).numpy()) < TOL
    assert np.array_equal(oh(ids), ref_onehot(t64(ids), shape[1]).numpy().astype(f32))
    total = float(ref_aggregate([ref_fdist(t64(xa), t64(xb)), ref_ramp(t64(xa), t64(xb), 0.5)], [1.0, 0.5]))
    assert close(float(loss(xa, xb)), total, TOL_LOSS)
    assert ed.n_labelled == want.size and close(ed.term_value, want.mean(), TOL_LOSS)


# ---- 5. nets against a float64 step ---------------------------------------------------------------------------
class RefN(RefL):
    """tests/test_regression_loss_gpu.py's float64 restatement of a graph with the nodes of this
    pull request.  Asserts on its OWN values that the case is well-posed: no ramp argument and no
    distance within 1e-6 of its kink."""

    def forward(self, feed, seed=0, counter=0):
        import torch.nn.functional as F
        m = self.model
        self.min_pre, self.n_kinked = np.inf, 0
        self.max_sig_pre, self.margin_gap = 0.0, np.inf
        self.min_conc, self.terms = np.inf, {}
        val = {}
        for node in m.nodes.values():
            kind = type(node).__name__
            par = node.parent
            if kind == 'Input':
                if node.name in feed:
                    val[node] = t64(feed[node.name])
            elif kind == 'Conv':
                y = F.conv3d(val[par], self.p(node.w).flip(2, 3, 4)) + self.p(node.b).view(1, -1, 1, 1, 1)
                assert not node.batch_normalisation and all(q == 1 for q in node.pool_shape)
                if node.activation_func == 'sigmoid':
                    self.max_sig_pre = max(self.max_sig_pre, float(y.detach().abs().max()))
                val[node] = self.act(node, y)
            elif kind == 'EuclideanDistance':
                val[node] = ref_fdist(val[par[0]], val[par[1]])
                self.margin_gap = min(self.margin_gap, float(val[node].detach().min()))
            elif kind == 'RampLoss':
                mg = float(f32(node.margin.get_value()))
                r = (val[par[0]] - val[par[1]] + mg).detach()
                self.margin_gap = min(self.margin_gap, float(r.abs().min()))
                val[node] = ref_ramp(val[par[0]], val[par[1]], mg)
            elif kind == 'BetaNLL':
                self.min_conc = min(self.min_conc, float(val[par[1]].detach().min()))
                val[node] = ref_beta(val[par[0]], val[par[1]], val[par[2]])
            elif kind == 'OneHot':
                val[node] = ref_onehot(val[par], node.n_class)
            elif kind == 'SquaredLoss':
                assert node.margin is None and node.scale_correction is None
                val[node] = ref_squared(val[par[0]], val[par[1]])
            elif kind == 'BinaryNLL':
                val[node] = ref_binary(val[par[0]], val[par[1]], node.subtract_label_entropy)
            elif kind == 'AggregateLoss':
                w = np.asarray(node.mixing_weights.get_value(), f32).astype(np.float64)
                val[node] = ref_aggregate([val[q] for q in par], w)
                for q in par:
                    masked = type(q).__name__ in ('SquaredLoss', 'BinaryNLL')
                    count = int((~is_masked(val[q.parent[1]])).sum()) if masked else val[q].numel()
                    self.terms[q.name] = (float(val[q].detach().mean()), count)
            else:
                raise NotImplementedError(kind)
        return val[m.loss_node], val[m.prediction_node]


def _rand(rng, node, batch):
    return rng.rand(*((batch,) + tuple(node.shape.shape[1:]))).astype(f32)


def net_a(batch=1, seed=71):
    """a 3-feature 'lin' head under AggregateLoss(EuclideanDistance(head, target))"""
    from elektronn2_amd import neuromancer as nm
    inp, out = _trunk(nm, batch, seed)
    head = nm.Conv(out, 3, (1, 1, 1), activation_func='lin', name='head')
    t = nm.Input_like(head, name='target')
    loss = nm.AggregateLoss(nm.EuclideanDistance(head, t, name='dist'), name='loss')
    return _done(nm, inp, loss, head)


def feed_a(m, seed):
    rng = np.random.RandomState(seed)
    return dict(raw=rng.rand(*m.nodes['raw'].shape.shape).astype(f32),
                target=rng.randn(*m.nodes['target'].shape.shape).astype(f32))


def net_b(batch=1, seed=72, margin=0.5):
    """a triplet: three Inputs through one trunk with SHARED w / b, two distances from the anchor,
    the hinge between them, mixed with a SquaredLoss on the anchor's embedding: the anchor branch
    receives gradient from both distances and from the squared term"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    sh = (batch, 1, 5, 14, 14)
    xa, xp, xn = (nm.Input(sh, 'b,f,z,x,y', name=k) for k in ('raw', 'pos', 'neg'))
    c1 = nm.Conv(xa, 6, (1, 3, 3), name='c1')
    ea = nm.Conv(c1, 3, (3, 3, 3), activation_func='tanh', name='emb')
    ep, en = (nm.Conv(nm.Conv(x, 6, (1, 3, 3), w=c1.w, b=c1.b, name='c1_' + k), 3, (3, 3, 3),
                      activation_func='tanh', w=ea.w, b=ea.b, name='emb_' + k)
              for x, k in ((xp, 'pos'), (xn, 'neg')))
    near = nm.EuclideanDistance(ea, ep, name='near')
    far = nm.EuclideanDistance(ea, en, name='far')
    ramp = nm.RampLoss(near, far, margin=margin, name='ramp')
    t = nm.Input_like(ea, name='target')
    loss = nm.AggregateLoss([ramp, nm.SquaredLoss(ea, t)], mixing_weights=[1.0, 0.5], name='loss')
    return _done(nm, xa, loss, ea)


def feed_b(m, seed):
    rng = np.random.RandomState(seed)
    sh = tuple(m.nodes['raw'].shape.shape)
    t = (rng.randn(*m.nodes['target'].shape.shape) * 0.3).astype(f32)
    t.flat[rng.permutation(t.size)[: t.size // 4]] = -666.0
    return dict(raw=rng.rand(*sh).astype(f32), pos=rng.rand(*sh).astype(f32), neg=rng.rand(*sh).astype(f32),
                target=t)


def net_c(batch=1, seed=73):
    """a 'sigmoid' mode head and a 'soft+' concentration head (bias 4: c > 2.1 throughout, asserted
    on the reference) on one trunk under a BetaNLL"""
    from elektronn2_amd import neuromancer as nm
    inp, out = _trunk(nm, batch, seed)
    mode = nm.Conv(out, 2, (1, 1, 1), activation_func='sigmoid', name='mode')
    conc = nm.Conv(out, 2, (1, 1, 1), activation_func='soft+', b=np.full((2,), 4.0, f32), name='conc')
    t = nm.Input_like(mode, name='target')
    loss = nm.AggregateLoss(nm.BetaNLL(mode, conc, t), name='loss')
    return _done(nm, inp, loss, mode)


def feed_c(m, seed):
    rng = np.random.RandomState(seed)
    t = rng.rand(*m.nodes['target'].shape.shape)
    t.flat[rng.permutation(t.size)[: t.size // 10]] = rng.randint(0, 2, t.size // 10)
    return dict(raw=rng.rand(*m.nodes['raw'].shape.shape).astype(f32), target=t.astype(f32))


def net_d(batch=1, seed=74):
    """BinaryNLL('sigmoid' head with n_class features, OneHot(class ids, n_class))"""
    from elektronn2_amd import neuromancer as nm
    inp, out = _trunk(nm, batch, seed)
    head = nm.Conv(out, 3, (1, 1, 1), activation_func='sigmoid', name='head')
    t = nm.Input_like(head, override_f=1, name='target')
    loss = nm.AggregateLoss(nm.BinaryNLL(head, nm.OneHot(t, 3)), name='loss')
    return _done(nm, inp, loss, head)


def feed_d(m, seed):
    rng = np.random.RandomState(seed)
    t = rng.randint(0, 3, m.nodes['target'].shape.shape).astype(f32)
    t.flat[rng.permutation(t.size)[: t.size // 8]] = -1.0   # unlabelled: a column of zeros
    return dict(raw=rng.rand(*m.nodes['raw'].shape.shape).astype(f32), target=t)


def args_of(m, feed):
    return [feed[n.name] for n in m.loss_node.input_nodes]


# name, constructor, feed, seed of the batch (chosen on the reference alone, on the CPU: RefN's assertions
# hold at both batch sizes over all steps, no kinked unit within 1e-5 of its kink for the triplet)
NETS = [("a_distance", net_a, feed_a, 82), ("b_triplet", net_b, feed_b, 126), ("c_beta", net_c, feed_c, 81),
        ("d_onehot", net_d, feed_d, 81)]


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("name,make,feeder,data_seed", NETS, ids=[n[0] for n in NETS])
def test_loss_gradients_and_adam_steps_against_float64(name, make, feeder, data_seed, batch):
    """loss, prediction, EVERY parameter gradient -- eager, captured and replayed calls -- and three
    Adam steps against float64 autograd; the terms as the nodes show them"""
    m = make(batch)
    feed = feeder(m, data_seed)
    args = args_of(m, feed)
    ref = RefN(m)
    for call in range(3):                                   # eager, capture, replay
        lref, pref = ref.loss_and_grads(feed)
        if name == "c_beta":
            assert ref.min_conc > 2.1, ref.min_conc
        loss = float(m.loss(*args))
        print("%s b%d call %d: loss %.7f ref %.7f (kink gap %.1e, min c %.2f)"
              % (name, batch, call, loss, lref, ref.margin_gap, ref.min_conc))
        assert close(loss, lref, TOL_STEP), (call, loss, lref)
        assert rel(m.predict(feed['raw']), pref) < TOL_STEP
        got = m.gradients(*args)
        names = list(m.loss_node.all_trainable_params.keys())
        want = ref.grads()
        assert len(got) == len(want) == len(names)
        for nme, g, w in zip(names, got, want):
            assert np.abs(w).max() > 0, nme
            assert rel(g, w) < TOL_STEP, (call, nme, rel(g, w))
        for n in m.loss_node.parent:
            L, count = ref.terms[n.name]
            assert close(n.term_value, L, TOL_LOSS), (n.name, n.term_value, L)
            assert n.n_labelled == count, (n.name, n.n_labelled, count)
    for step in range(3):                                   # Adam: eager, captured, replayed
        lref, _ = ref.loss_and_grads(feed)
        ref.adam(**ADAM)
        loss = float(m.trainingstep(*args, optimiser='Adam')[0])
        assert close(loss, lref, TOL_STEP), (step, loss, lref)
        for nme, p in m.loss_node.all_trainable_params.items():
            e = rel(p.get_value(), ref.p(p).detach().numpy())
            assert e < TOL_STEP, (step, nme, e)
    assert m.optimisers['Adam'].step.func._graphs, "the step was not captured"


def test_plan_of_the_triplet_net():
    """the map nodes are materialised with one feature and a gradient of their own; the aggregate
    owns the slab of a map term; the anchor's gradient buffer has three writers"""
    m = net_b()
    m.gradients(*args_of(m, feed_b(m, 81)))
    plan = m._grad_func.func
    agg, ramp = m.loss_node, m.nodes['ramp']
    assert agg.elementwise and plan.scratch[ramp, 'agg'] == (agg, 0)
    for k in ('near', 'far', 'ramp'):
        assert tuple(plan.out[m.nodes[k]].shape) == (1, 1, 3, 10, 10)
        assert tuple(plan.grad[m.nodes[k]].shape) == (1, 1, 3, 10, 10)
    assert plan.scratch[ramp, 'partials'].numel() == 4 * plan.ctx.loss_partials(plan.out[ramp])
    assert plan.scratch[ramp, 'n_tot'] == 300
    assert (m.nodes['near'], 'partials') not in plan.scratch          # not a term: no slab
    assert plan._loss_dev() is plan.scratch[agg, 'loss']


# ---- 6. plumbing, once each on the triplet net --------------------------------------------------------------
def test_margin_is_read_in_place_by_a_captured_plan():
    """after set_value the next REPLAY of the captured plans follows the new margin"""
    m = net_b()
    feed = feed_b(m, 81)
    args = args_of(m, feed)
    for _ in range(3):
        m.gradients(*args)
        m.loss(*args)
    gplan, lplan = m._grad_func.func, m.loss_node._output_func.func
    graphs = (list(gplan._graphs), list(lplan._graphs))
    assert all(graphs)
    seen = []
    for mg in (0.125, 2.0):
        m.nodes['ramp'].params['margin'].set_value(f32(mg))
        ref = RefN(m)
        lref, _ = ref.loss_and_grads(feed)
        assert close(float(m.loss(*args)), lref, TOL_STEP)
        for nme, g, w in zip(m.loss_node.all_trainable_params.keys(), m.gradients(*args), ref.grads()):
            assert rel(g, w) < TOL_STEP, (mg, nme, rel(g, w))
        assert close(m.nodes['ramp'].term_value, ref.terms['ramp'][0], TOL_LOSS)
        seen.append(lref)
        assert (list(gplan._graphs), list(lplan._graphs)) == graphs          # no new capture
    assert abs(seen[0] - seen[1]) > 1e-3 * abs(seen[1])


def test_several_steps_in_one_graph_equal_single_steps():
    """trainingsteps(3, ring) against three single steps: losses 1e-5, parameters 1e-4"""
    a = net_b()
    feeds = [feed_b(a, 90 + i) for i in range(3)]
    A = lambda mm, i: args_of(mm, feeds[i % 3])
    sync = [float(a.trainingstep(*A(a, i), optimiser='Adam')[0]) for i in range(5)]
    c = net_b()
    for i in range(2):                                       # eager + capture (builds the plan)
        c.trainingstep(*A(c, i), optimiser='Adam')
    pl = c.optimisers['Adam'].step.func
    ring = torch.empty((3, pl.input_arena.numel()), device='cuda')
    for i in range(3):
        for n in c.loss_node.input_nodes:
            o, cnt = pl.input_slices[n]
            ring[i, o:o + cnt] = dev(feeds[(2 + i) % 3][n.name]).reshape(-1)
    losses, tsec = c.trainingsteps(3, optimiser='Adam', ring=ring)
    assert len(losses) == 3
    for u, v in zip(sync[2:5], losses):
        assert close(float(v), u, 1e-5), (sync, list(losses))
    for pa, pc in zip(a.loss_node.all_trainable_params.values(), c.loss_node.all_trainable_params.values()):
        assert rel(pc.get_value(), pa.get_value()) < 1e-4


def test_checkpoint_after_two_steps_resumes_to_the_same_third_step(tmp_path):
    from elektronn2_amd.neuromancer.model import modelload
    a = net_b()
    feed = feed_b(a, 81)
    args = args_of(a, feed)
    a.nodes['ramp'].params['margin'].set_value(f32(0.75))
    for _ in range(2):
        a.trainingstep(*args, optimiser='Adam')
    f = str(tmp_path / "triplet.mdl")
    a.save(f)
    saved = [p.get_value() for p in a.loss_node.all_trainable_params.values()]
    third = float(a.trainingstep(*args, optimiser='Adam')[0])
    end_p = [p.get_value() for p in a.loss_node.all_trainable_params.values()]
    b = net_b(seed=99)                                       # other weights, nothing on the device
    modelload(f, b)
    for v, p in zip(saved, b.loss_node.all_trainable_params.values()):
        assert np.array_equal(v, p.get_value())              # bit-equal
    assert float(b.nodes['ramp'].params['margin'].get_value()) == 0.75
    got = float(b.trainingstep(*args, optimiser='Adam')[0])
    assert close(got, third, 2e-6), (third, got)
    for v, p in zip(end_p, b.loss_node.all_trainable_params.values()):
        assert np.abs(v - p.get_value()).max() <= 1e-5 * np.abs(v).max()
    c = modelload(f)                                         # the graph rebuilt from the file alone
    assert [type(n).__name__ for n in c.loss_node.parent] == ['RampLoss', 'SquaredLoss']
    assert float(c.nodes['ramp'].params['margin'].get_value()) == 0.75
    assert c.nodes['emb_pos'].w is c.nodes['emb'].w
    b2 = net_b(seed=98)
    modelload(f, b2)
    assert close(float(c.loss(*args_of(c, feed))), float(b2.loss(*args)), 1e-6)


@pytest.fixture()
def process_bf16():
    import elektronn2_amd
    elektronn2_amd.set_mfma_dtype('bf16')
    yield
    elektronn2_amd.set_mfma_dtype('f32')


def test_bf16_mode_keeps_the_loss_kernels_in_f32(process_bf16):
    """one gradient evaluation of the triplet net in bf16 operand mode: the loss and the gradients the
    loss kernels wrote, against the restatement on the float32 embeddings the DEVICE produced"""
    m = net_b()
    feed = feed_b(m, 81)
    m.gradients(*args_of(m, feed))
    plan = m._grad_func.func
    torch.cuda.synchronize()
    emb = [t64(plan.out[m.nodes[k]].detach().cpu().numpy(), True) for k in ('emb', 'emb_pos', 'emb_neg')]
    near, far = ref_fdist(emb[0], emb[1]), ref_fdist(emb[0], emb[2])
    ramp = ref_ramp(near, far, 0.5)
    total = ref_aggregate([ramp, ref_squared(emb[0], t64(feed['target']))], [1.0, 0.5])
    assert float((near - far + 0.5).detach().abs().min()) >= 1e-6
    g = [x.numpy() for x in torch.autograd.grad(total, emb)]
    assert close(plan._loss_dev().item(), float(total.detach()), TOL_LOSS)
    for k, want in zip(('emb', 'emb_pos', 'emb_neg'), g):
        assert rel(plan.grad[m.nodes[k]].detach().cpu().numpy(), want) < TOL, k
    assert close(m.nodes['ramp'].term_value, float(ramp.detach().mean()), TOL_LOSS)
