"""SquaredLoss / AbsLoss / BinaryNLL / GaussianNLL / mixed AggregateLoss, host side (no GPU).

``ref_squared`` / ``ref_abs`` / ``ref_binary`` / ``ref_gauss`` / ``ref_aggregate`` restate the
reference's lines (loss.py:829-887, 953-1011, 1014-1101, 1215-1276, 1346-1363) in float64 torch,
written from the formulas: the element-wise array times n_tot / (n_lab + 1), the mask set to zero,
the plain means.  They are the reference of every GPU comparison (tests/test_regression_loss_gpu.py).
Here they are checked against the closed forms of include/e2hip.h ("element-wise losses") at 1e-12;
then the nodes are constructed without a device and the C ABI is checked for the new entries.

T.isclose(t, -666.0) is read as |t + 666| <= atol + rtol * 666 with Theano's defaults rtol = 1e-5,
atol = 1e-8 (Theano cannot be imported where this is developed: pinned by reading alone)."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5
MASK_TOL = 1e-8 + 1e-5 * 666.0


# ---- the float64 restatement -------------------------------------------------------------------------
def is_masked(t):
    return (t + 666.0).abs() <= MASK_TOL


def xlogy0(x, y):
    """x log y, 0 where x == 0 (and no gradient there)"""
    safe = torch.where(x == 0, torch.ones_like(y), y)
    return torch.where(x == 0, torch.zeros_like(x), x * torch.log(safe))


def _scale(pred, mask):
    n_lab = (~mask).sum().to(pred.dtype)
    return pred.numel() / (n_lab + 1), n_lab


def ref_squared(pred, target, margin=None, scale_correction=None):
    """loss.py:1075-1096: the node's output (mean over 'f' = axis 1, kept)"""
    mask = is_masked(target)
    scale, _ = _scale(pred, mask)
    if margin is not None:
        diff = target - pred
        out = scale * 0.5 * diff ** 2 * (diff.abs() >= margin).to(pred.dtype) - margin
    else:
        out = scale * 0.5 * (target - pred) ** 2
    if scale_correction is not None:
        out = out * (scale_correction / (target.abs() + scale_correction))
    out = torch.where(mask, torch.zeros_like(out), out)
    return out.mean(dim=1, keepdim=True)


def ref_abs(pred, target, margin=None, scale_correction=None):
    """loss.py:1256-1275"""
    mask = is_masked(target)
    scale, _ = _scale(pred, mask)
    if margin is not None:
        diff = target - pred
        out = scale * diff.abs() * (diff.abs() >= margin).to(pred.dtype) - margin
    else:
        out = scale * (target - pred).abs()
    if scale_correction is not None:
        out = out * (scale_correction * target.abs() + 1.0)
    out = torch.where(mask, torch.zeros_like(out), out)
    return out.mean(dim=1, keepdim=True)


def ref_binary(pred, target, subtract_label_entropy=False):
    """loss.py:994-1010"""
    mask = is_masked(target)
    scale, _ = _scale(pred, mask)
    out = -xlogy0(target, pred + EPS) - xlogy0(1.0 - target, 1.0 - pred + EPS)
    if subtract_label_entropy:
        out = out + (-xlogy0(target, target + EPS) - xlogy0(1.0 - target, 1.0 - target + EPS))
    out = torch.where(mask, torch.zeros_like(out), out)
    return out * scale


def ref_gauss(mu, sig, target, sig_is_log=False):
    """loss.py:877-887"""
    if sig_is_log:
        log_sig, sig = sig, torch.exp(sig)
    else:
        log_sig = torch.log(sig)
    return 0.5 * np.log(2 * np.pi) + log_sig + 0.5 * ((target - mu) / sig) ** 2


def ref_aggregate(outputs, mixing_weights):
    """loss.py:1357-1363: mean over the terms of (mean of each term's output) * weight"""
    means = torch.stack([o.mean() for o in outputs])
    return (means * torch.as_tensor(np.asarray(mixing_weights, np.float64))).mean()


def n_labelled(target):
    return int((~is_masked(torch.as_tensor(np.asarray(target, np.float64)))).sum())


# ---- the closed forms of the table (numpy float64) -----------------------------------------------------
def closed_squared(p, t, margin=None, sc=None, absloss=False):
    m = ~(np.abs(t + 666.0) <= MASK_TOL)
    n_lab, n_tot = m.sum(), p.size
    d = t - p
    g = (np.abs(d) >= margin).astype(np.float64) if margin is not None else np.ones_like(d)
    if sc is None:
        c = np.ones_like(d)
    else:
        c = sc * np.abs(t) + 1.0 if absloss else sc / (np.abs(t) + sc)
    l = (np.abs(d) if absloss else 0.5 * d * d) * g * c
    L = (l * m).sum() / (n_lab + 1)
    if margin is not None:
        L -= margin * (c * m).sum() / n_tot
    slope = -np.sign(d) if absloss else -d
    return L, slope * g * c * m / (n_lab + 1), n_lab


def closed_binary(p, t, entropy=False):
    m = ~(np.abs(t + 666.0) <= MASK_TOL)
    n_lab = m.sum()
    t = np.where(m, t, 0.5)                       # (masked elements: any valid value, dropped below)
    xl = lambda x, y: np.where(x == 0, 0.0, x * np.log(np.where(x == 0, 1.0, y)))
    l = -xl(t, p + EPS) - xl(1 - t, 1 - p + EPS)
    if entropy:
        l = l - xl(t, t + EPS) - xl(1 - t, 1 - t + EPS)
    g = -t / (p + EPS) + (1 - t) / (1 - p + EPS)
    return (l * m).sum() / (n_lab + 1), g * m / (n_lab + 1), n_lab


def closed_gauss(mu, sig, t, sig_is_log=False):
    n = mu.size
    s = np.exp(sig) if sig_is_log else sig
    ls = sig if sig_is_log else np.log(sig)
    L = (0.5 * np.log(2 * np.pi) + ls + 0.5 * ((t - mu) / s) ** 2).sum() / n
    dmu = -(t - mu) / s ** 2 / n
    dsig = (1 - (t - mu) ** 2 / s ** 2) / n if sig_is_log else (1 / s - (t - mu) ** 2 / s ** 3) / n
    return L, dmu, dsig


def _data(rng, shape=(2, 3, 4, 5, 6)):
    p = rng.rand(*shape) * 0.9 + 0.05
    t = rng.rand(*shape)
    t.flat[rng.permutation(t.size)[: t.size // 4]] = -666.0
    t.flat[3] = -666.004                        # inside the tolerance
    t.flat[5] = -666.01                         # outside
    return p, t


def _grad(value, *leaves):
    return [g.numpy() for g in torch.autograd.grad(value, leaves)]


OPTS = list(itertools.product([None, 0.3], [None, 0.7]))


# ---- 1. restatement == closed forms --------------------------------------------------------------------
@pytest.mark.parametrize("absloss", [False, True], ids=["squared", "abs"])
@pytest.mark.parametrize("margin,sc", OPTS)
def test_restated_squared_and_abs_equal_the_closed_forms(absloss, margin, sc):
    rng = np.random.RandomState(1)
    p, t = _data(rng)
    t = np.where(np.abs(t + 666) < 1, t, t * 3 - 1)            # (targets beyond [0, 1] too)
    tp = torch.tensor(p, requires_grad=True)
    out = (ref_abs if absloss else ref_squared)(tp, torch.tensor(t), margin, sc)
    assert tuple(out.shape) == (2, 1, 4, 5, 6)
    total = ref_aggregate([out], [1.0])
    L, dp, n_lab = closed_squared(p, t, margin, sc, absloss)
    assert n_lab == n_labelled(t) and 0 < n_lab < p.size
    assert abs(float(total.detach()) - L) <= 1e-12 * max(1.0, abs(L))
    assert np.abs(_grad(total, tp)[0] - dp).max() <= 1e-12


@pytest.mark.parametrize("entropy", [False, True])
def test_restated_binary_nll_equals_the_closed_form(entropy):
    rng = np.random.RandomState(2)
    p, t = _data(rng)
    t.flat[5] = 0.5                                            # (Bernoulli targets lie in [0, 1])
    t.flat[7:12] = [0.0, 1.0, 0.0, 1.0, 0.3]
    p.flat[7:12] = [0.0, 1.0, 1.0, 0.0, 0.5]                   # the xlogy0 zero branches
    tp = torch.tensor(p, requires_grad=True)
    out = ref_binary(tp, torch.tensor(t), entropy)
    assert tuple(out.shape) == p.shape
    total = ref_aggregate([out], [1.0])
    L, dp, n_lab = closed_binary(p, t, entropy)
    assert abs(float(total.detach()) - L) <= 1e-12 * max(1.0, abs(L))
    g = _grad(total, tp)[0]
    assert np.all(np.isfinite(g)) and np.abs(g - dp).max() <= 1e-12 * np.abs(dp).max()


@pytest.mark.parametrize("sig_is_log", [False, True])
def test_restated_gaussian_nll_equals_the_closed_form(sig_is_log):
    rng = np.random.RandomState(3)
    shape = (2, 3, 4, 5, 6)
    mu, t = rng.randn(*shape), rng.randn(*shape)
    sig = rng.uniform(-3, 3, shape) if sig_is_log else rng.uniform(0.05, 3, shape)
    tm, ts = torch.tensor(mu, requires_grad=True), torch.tensor(sig, requires_grad=True)
    total = ref_aggregate([ref_gauss(tm, ts, torch.tensor(t), sig_is_log)], [1.0])
    L, dmu, dsig = closed_gauss(mu, sig, t, sig_is_log)
    assert abs(float(total.detach()) - L) <= 1e-12 * max(1.0, abs(L))
    gm, gs = _grad(total, tm, ts)
    assert np.abs(gm - dmu).max() <= 1e-12 * np.abs(dmu).max()
    assert np.abs(gs - dsig).max() <= 1e-12 * np.abs(dsig).max()


def test_restated_aggregate_equals_the_weighted_mean_of_the_terms():
    rng = np.random.RandomState(4)
    p, t = _data(rng)
    t.flat[5] = 0.5
    q = rng.randn(2, 1, 4, 5, 6)
    u = rng.randn(2, 1, 4, 5, 6)
    u.flat[::5] = -666.0
    w = [1.0, 0.25, 2.0]
    tp, tq = torch.tensor(p, requires_grad=True), torch.tensor(q, requires_grad=True)
    total = ref_aggregate([ref_binary(tp, torch.tensor(t)), ref_squared(tq, torch.tensor(u), 0.3, 0.7),
                           ref_abs(tq, torch.tensor(u))], w)
    Lb, db, _ = closed_binary(p, t)
    Ls, ds, _ = closed_squared(q, u, 0.3, 0.7)
    La, da, _ = closed_squared(q, u, absloss=True)
    want = (w[0] * Lb + w[1] * Ls + w[2] * La) / 3
    assert abs(float(total.detach()) - want) <= 1e-12 * abs(want)
    gp, gq = _grad(total, tp, tq)
    assert np.abs(gp - w[0] / 3 * db).max() <= 1e-12 * np.abs(db).max()
    assert np.abs(gq - (w[1] / 3 * ds + w[2] / 3 * da)).max() <= 1e-12


def test_all_masked_target_gives_zero_loss_and_gradient():
    p = torch.rand(1, 2, 1, 3, 4, dtype=torch.float64, requires_grad=True)
    t = torch.full((1, 2, 1, 3, 4), -666.0, dtype=torch.float64)
    for out in (ref_squared(p, t, 0.5, 0.7), ref_abs(p, t), ref_binary(p, t, True)):
        total = ref_aggregate([out], [1.0])
        # (the margin is subtracted before the mask is applied: masked elements are zero all the same)
        assert float(total.detach()) == 0.0
        assert np.all(_grad(total, p)[0] == 0)


# ---- 2. node construction without a device -----------------------------------------------------------------
def _heads():
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    inp = nm.Input((1, 1, 5, 12, 12), 'b,f,z,x,y', name='raw')
    trunk = nm.Conv(inp, 4, (1, 3, 3))
    a = nm.Conv(trunk, 3, (1, 1, 1), activation_func='sigmoid', name='head_a')
    b = nm.Conv(trunk, 1, (1, 1, 1), activation_func='lin', name='head_b')
    s = nm.Conv(trunk, 1, (1, 1, 1), activation_func='soft+', name='head_s')
    return nm, inp, trunk, a, b, s


def test_nodes_have_the_reference_signatures_names_shapes_and_params():
    nm, inp, trunk, a, b, s = _heads()
    ta, tb = nm.Input_like(a, name='ta'), nm.Input_like(b, name='tb')
    se = nm.SquaredLoss(b, tb)
    assert se.name == 'se' and not se.params and se.margin is None and se.scale_correction is None
    assert tuple(se.shape.shape) == (1, 1, 5, 10, 10)
    se3 = nm.SquaredLoss(a, ta, margin=0.5, scale_correction=2.0)
    assert tuple(se3.shape.shape) == (1, 1, 5, 10, 10)           # the 'f' axis becomes 1
    assert set(se3.params) == {'margin', 'scale_correction'}
    assert float(se3.params['margin'].get_value()) == 0.5
    assert float(se3.params['scale_correction'].get_value()) == 2.0
    assert not se3.params['margin'].apply_train and not se3.params['scale_correction'].apply_train
    zero = nm.SquaredLoss(b, tb, margin=0, scale_correction=0.0)   # falsy means none (loss.py:1045)
    assert zero.margin is None and zero.scale_correction is None and not zero.params
    ab = nm.AbsLoss(b, tb, margin=0.25)
    assert ab.name == 'absloss' and isinstance(ab, nm.SquaredLoss) and set(ab.params) == {'margin'}
    assert tuple(ab.shape.shape) == (1, 1, 5, 10, 10)
    bn = nm.BinaryNLL(a, ta, subtract_label_entropy=True)
    assert bn.name == 'binary_nll' and bn.subtract_label_entropy is True
    assert tuple(bn.shape.shape) == (1, 3, 5, 10, 10)            # the prediction's shape
    g = nm.GaussianNLL(b, s, tb, sig_is_log=False)
    assert g.name == 'g_nll' and tuple(g.shape.shape) == (1, 1, 5, 10, 10)
    assert list(g.parent) == [b, s, tb]
    for n in (se, ab, bn, g):
        assert n.term_value is None and n.n_labelled is None     # nothing has run
    agg = nm.AggregateLoss([bn, se, ab], mixing_weights=[1.0, 0.25, 2.0])
    assert agg.elementwise and tuple(agg.shape.shape) == (1,)
    mw = agg.params['mixing_weights']
    assert not mw.apply_train and np.allclose(mw.get_value(), [1.0, 0.25, 2.0])
    one = nm.AggregateLoss(g)
    assert one.elementwise and np.allclose(one.params['mixing_weights'].get_value(), [1.0])
    # positional arguments in the reference's order
    import inspect
    sig = lambda c: list(inspect.signature(c.__init__).parameters)[1:]
    assert sig(nm.SquaredLoss) == ['pred', 'target', 'margin', 'scale_correction', 'name', 'print_repr']
    assert sig(nm.AbsLoss) == sig(nm.SquaredLoss)
    assert sig(nm.BinaryNLL) == ['pred', 'target', 'subtract_label_entropy', 'name', 'print_repr']
    assert sig(nm.GaussianNLL) == ['mu', 'sig', 'target', 'sig_is_log', 'name', 'print_repr']


def test_construction_errors():
    nm, inp, trunk, a, b, s = _heads()
    ta, tb = nm.Input_like(a, name='ta'), nm.Input_like(b, name='tb')
    with pytest.raises(ValueError, match="target must have the prediction's shape"):
        nm.SquaredLoss(a, tb)
    with pytest.raises(ValueError, match="target must have the prediction's shape"):
        nm.AbsLoss(b, ta)
    with pytest.raises(ValueError, match="target must have the prediction's shape"):
        nm.BinaryNLL(a, tb)
    with pytest.raises(ValueError, match="sig must have the prediction's shape"):
        nm.GaussianNLL(b, a, tb)
    with pytest.raises(ValueError, match="target must have the prediction's shape"):
        nm.GaussianNLL(b, s, ta)
    sa = nm.Input((1, 4, 3, 5, 5), 'b,s,f,x,y', name='samples')
    st = nm.Input_like(sa, name='samples_t')
    for make in (lambda: nm.BinaryNLL(sa, st), lambda: nm.SquaredLoss(sa, st),
                 lambda: nm.GaussianNLL(sa, sa, st)):
        with pytest.raises(NotImplementedError, match="'s' sample axis"):
            make()
    terms = [nm.SquaredLoss(b, tb) for _ in range(9)]
    with pytest.raises(ValueError, match="at most 8"):
        nm.AggregateLoss(terms)
    assert nm.AggregateLoss(terms[:8]).elementwise
    with pytest.raises(ValueError, match="Mismatch"):
        nm.AggregateLoss(terms[:2], mixing_weights=[1.0])
    lin2 = nm.Conv(trunk, 2, (1, 1, 1), activation_func='lin')
    probs = nm.Softmax(lin2)
    tc = nm.Input_like(probs, override_f=1, name='tc')
    nll = nm.MultinoulliNLL(probs, tc, target_is_sparse=True)
    with pytest.raises(NotImplementedError, match="take no scale"):
        nm.AggregateLoss([nll, terms[0]])
    with pytest.raises(NotImplementedError, match="take no scale"):
        nm.AggregateLoss([nll, nll])
    with pytest.raises(NotImplementedError):
        nm.AggregateLoss([b])
    single = nm.AggregateLoss(nll)                       # the untouched form still constructs
    assert not single.elementwise and list(single.parent) == [nll]


def test_new_nodes_are_exported_and_found_by_modelload():
    from elektronn2_amd import neuromancer as nm
    from elektronn2_amd.neuromancer import loss as loss_mod
    for k in ('SquaredLoss', 'AbsLoss', 'BinaryNLL', 'GaussianNLL'):
        assert getattr(nm, k) is getattr(loss_mod, k) and k in loss_mod.__all__


def test_descriptors_of_a_model_with_the_new_nodes_serialise():
    nm, inp, trunk, a, b, s = _heads()
    ta, tb = nm.Input_like(a, name='ta'), nm.Input_like(b, name='tb')
    agg = nm.AggregateLoss([nm.BinaryNLL(a, ta), nm.SquaredLoss(b, tb, margin=0.5, scale_correction=2.0),
                            nm.GaussianNLL(b, s, tb, sig_is_log=True)], mixing_weights=[1.0, 0.25, 2.0])
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=ta, loss_node=agg, prediction_node=a)
    import json
    d = json.loads(json.dumps(model.serialise()))
    by = dict((n[0], n) for n in d["nodes"])
    assert by['se'][1] == 'SquaredLoss' and by['se'][3]['margin'] == 0.5
    assert by['g_nll'][3]['sig_is_log'] is True
    assert by[agg.name][1] == 'AggregateLoss'


# ---- 3. C ABI -----------------------------------------------------------------------------------------
def test_header_declares_and_backend_binds_the_new_entries():
    from elektronn2_amd import backend
    src = open(os.path.join(ROOT, "include", "e2hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s in ("e2_loss_partials", "e2_loss_fwd", "e2_loss_mix", "e2_loss_bwd"):
        assert re.search(r"\b%s\s*\(" % s, plain), s
        assert s in backend.EXPORTED_SYMBOLS, s
        assert hasattr(backend.lib(), s)
    assert re.search(r"#define\s+E2_MAX_LOSS_TERMS\s+8\b", plain)
    m = re.search(r"enum\s*\{\s*E2_LOSS_SQUARED\s*=\s*0\s*,\s*E2_LOSS_ABS\s*,\s*E2_LOSS_BINARY_NLL\s*,"
                  r"\s*E2_LOSS_GAUSS_NLL\s*\}", plain)
    assert m, "the E2_LOSS_* enum"
    assert backend.LOSS == {"squared": 0, "abs": 1, "binary_nll": 2, "gauss_nll": 3}
    assert backend.MAX_LOSS_TERMS == 8
    from elektronn2_amd.neuromancer import loss as loss_mod
    assert loss_mod.MAX_LOSS_TERMS == 8
    # the descriptor mirrors e2_loss_term field by field
    fields = [f[0] for f in backend.LossTerm._fields_]
    assert fields == ['kind', 'margin', 'scale_correction', 'subtract_label_entropy', 'sig_is_log']
    t = backend.loss_term('binary_nll', subtract_label_entropy=True)
    assert t.kind == 2 and t.subtract_label_entropy == 1 and not t.margin and not t.scale_correction
    with pytest.raises(ValueError):
        backend.loss_term('hinge')
