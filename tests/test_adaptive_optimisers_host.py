"""AdaGrad / AdaDelta updates (csrc/arena_ops.hip adagrad_kernel, adadelta_kernel;
optimiser.py:168-214, :222-264 of the reference), host side (no GPU): what
tests/test_adaptive_optimisers_gpu.py compares the kernels with, and the evidence that its rule can
see what they compute.  Method and helpers of tests/test_optimiser_host.py.

* ``adagrad_ref`` / ``adadelta_ref``: float64, element-wise restatements over a per-element
  multiplier and the gradient scale gs, each with the sum of the absolute values of the terms
  that are summed.  They are pinned against a second restatement of another form: a plain loop,
  parameter by parameter, over the reference's own expressions -- with init_func's and the step's
  two ``h += g^2`` for AdaGrad's first call.
* AdaGrad's rules beyond the expressions: the first step (t == 0) adds 2 g^2; the weight decay
  takes r = (multiplier != 0), never the multiplier (the reference has no apply_reg > 1 branch
  there); an element whose h' is 0 is left as it is (the reference divides by sqrt(0)).
* ``CASES``: the table of tests/test_optimiser_host.py (segment counts 1 .. 1024, lengths with and
  without a scalar tail and beyond one grid sweep, t0 0 .. 999, both wd, every gradient scaling,
  zero_g both ways) with inputs of their own: every non-zero |g gs| in [1e-6, 1e2], so that
  g'^2 is a normal float32 number and h' == 0 means the same in float32 and float64; exact zeros
  of g planted on h = 0 and on h > 0; multipliers 0, 1, 3, 0.5 in turn and 2.5 on the last segment.
* the acceptance rule: |got - ref| <= tolerance * sum |terms|, element by element.
* ``YARD``: the worst ratio of a float32 NumPy restatement in the kernels' operation order against
  the float64 one over CASES, per kernel and output, measured here without any kernel; the
  tolerance of an output is 4 x its yardstick (the margin of tests/test_optimiser_host.py: it
  absorbs differences in fusion and operation order), ``TOL`` the largest of them.
* mutants of the float32 restatements, each of which must break the rule a hundredfold somewhere.
* the host API: four optimisers per model (two of them made on first use), the shared meta
  parameters, the state dicts through save / modelload before any step, the fall-back to SGD for a
  name that is none of the four."""
import functools
import logging

import numpy as np
import pytest

import test_optimiser_host as H
from test_optimiser_host import CASES, CASE_IDS, F

EPS = 1e-5                                   # AdaDelta's epsilon, inside both roots
G_LO, G_HI = 1e-6, 1e2                       # every non-zero |g gs|
MULTS = (0.0, 1.0, 3.0, 0.5)
MUTANT_FACTOR = H.MUTANT_FACTOR


# ---- the float64 restatements ----------------------------------------------------------------------
def adagrad_ref(p, g, h, mult, hyp, t0, gs=1.0):
    """-> ({p, h}, {p, h}: the sum of the absolute terms of each).  ``mult``: the multiplier of
    every element, of which only (mult != 0) is used; ``t0``: the steps taken before this one"""
    p, g, h, mult = H._f64(p, g, h, mult)
    lr, wd = hyp['lr'], hyp['wd']
    g = g * gs
    c = 2.0 if t0 == 0 else 1.0
    nh = h + c * g * g
    r = (mult != 0).astype(np.float64)
    live = nh != 0
    a = np.zeros_like(nh)
    a[live] = lr / np.sqrt(nh[live])
    new_p = p - a * (g + wd * r * p)
    terms = dict(p=np.abs(p) + np.abs(new_p) + a * (np.abs(g) + wd * r * np.abs(p)),
                 h=np.abs(h) + c * g * g)
    return dict(p=new_p, h=nh), terms


def adadelta_ref(p, g, s, d, mult, hyp, gs=1.0):
    """-> ({p, s, d}, {p, s, d}: the sum of the absolute terms of each)"""
    p, g, s, d, mult = H._f64(p, g, s, d, mult)
    lr, mom, wd = hyp['lr'], hyp['mom'], hyp['wd']
    g = g * gs
    ns = mom * s + (1.0 - mom) * g * g
    direction = g * np.sqrt(d + EPS) / np.sqrt(s + EPS)
    nd = mom * d + (1.0 - mom) * direction * direction
    new_p = p - lr * (direction + wd * mult * p)
    terms = dict(p=np.abs(p) + np.abs(new_p) + lr * np.abs(direction) + lr * wd * mult * np.abs(p),
                 s=np.abs(mom * s) + (1.0 - mom) * g * g,
                 d=np.abs(mom * d) + (1.0 - mom) * direction * direction)
    return dict(p=new_p, s=ns, d=nd), terms


# ---- the second form: the reference's expressions, parameter by parameter -----------------------------
def adagrad_loop(c):
    """optimiser.py:185-214 over the segments of case ``c``: the first call (t0 == 0) runs
    init_func's ``h + square(g)`` and then the step's; where the new h is 0 the parameter is put
    back (the departure)"""
    lr, wd = c['h']['lr'], c['h']['wd']
    out_p, out_h = [], []
    for k, apply_reg in enumerate(c['seg_reg']):
        sl = slice(c['seg_off'][k], c['seg_off'][k + 1])
        p, g, h = H._f64(c['p'][sl], c['g'][sl], c['hs'][sl])
        g = g * c['gs']                                      # (the gradient the step is handed)
        if c['t0'] == 0:                                     # init_func
            h = h + np.square(g)
        new_h = h + np.square(g)
        with np.errstate(divide='ignore', invalid='ignore'):
            if apply_reg:
                new_p = p - lr / np.sqrt(new_h) * (g + wd * p)
            else:
                new_p = p - lr / np.sqrt(new_h) * g
        new_p[new_h == 0] = p[new_h == 0]
        out_p.append(new_p)
        out_h.append(new_h)
    return dict(p=np.concatenate(out_p), h=np.concatenate(out_h))


def adadelta_loop(c):
    """optimiser.py:241-259 over the segments of case ``c``"""
    lr, mom, wd = c['h']['lr'], c['h']['mom'], c['h']['wd']
    epsilon = 1e-5
    out = dict(p=[], s=[], d=[])
    for k, multiplier in enumerate(c['seg_reg']):
        sl = slice(c['seg_off'][k], c['seg_off'][k + 1])
        p, g, s, d = H._f64(c['p'][sl], c['g'][sl], c['s'][sl], c['d'][sl])
        g = g * c['gs']
        new_s = mom * s + (1.0 - mom) * np.square(g)
        direction = (g * np.sqrt(d + epsilon) / np.sqrt(s + epsilon))
        new_d = mom * d + (1 - mom) * np.square(direction)
        # (the reference's two decaying branches are one expression over the table's value, which
        # variables.reg_multiplier sets to 1 wherever apply_reg is not above 1)
        if multiplier:
            new_p = p - lr * (direction + wd * p * float(multiplier))
        else:
            new_p = p - lr * direction
        out['p'].append(new_p)
        out['s'].append(new_s)
        out['d'].append(new_d)
    return dict((k, np.concatenate(v)) for k, v in out.items())


# ---- the float32 restatements, in the kernels' operation order -------------------------------------
ADAGRAD_MUTANTS = ['no_doubling', 'always_doubling', 'mult_for_r', 'gs_after_square', 'update_at_h0',
                   'no_wd', 'mult_shift4']
ADADELTA_MUTANTS = ['dir_new_s', 'dir_new_d', 'eps_outside', 'no_wd', 'mult_shift4']


def adagrad_f32(p, g, h, mult, hyp, t0, gdiv=None, gmul=1.0, mutant=None):
    """adagrad_kernel's arithmetic, one rounding per operation -> {p, h}"""
    p, g, h = (np.asarray(v, F) for v in (p, g, h))
    lr, wd = F(hyp['lr']), F(hyp['wd'])
    gs = H._gs_f32(gdiv, gmul, None)
    c = F(2) if t0 == 0 else F(1)
    if mutant == 'no_doubling':
        c = F(1)
    elif mutant == 'always_doubling':
        c = F(2)
    mm = H._mult_f32(mult, 1.0, mutant)                     # ('no_wd', 'mult_shift4')
    rw = mm * wd if mutant == 'mult_for_r' else np.where(mm != 0, wd, F(0)).astype(F)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        raw = g
        if gs != F(1):
            g = g * gs
        gg = (raw * raw) * gs if mutant == 'gs_after_square' else g * g
        nh = h + c * gg
        new_p = p - lr / np.sqrt(nh) * np.where(rw != 0, g + rw * p, g)
        if mutant != 'update_at_h0':
            new_p = np.where(nh != 0, new_p, p)
    assert new_p.dtype == nh.dtype == F
    return dict(p=new_p, h=nh)


def adadelta_f32(p, g, s, d, mult, hyp, gdiv=None, gmul=1.0, mutant=None):
    """adadelta_kernel's arithmetic, one rounding per operation -> {p, s, d}"""
    p, g, s, d = (np.asarray(v, F) for v in (p, g, s, d))
    lr, mom, eps = F(hyp['lr']), F(hyp['mom']), F(EPS)
    gs = H._gs_f32(gdiv, gmul, None)
    mu = H._mult_f32(mult, hyp['wd'], mutant)               # ('no_wd', 'mult_shift4')
    with np.errstate(invalid='ignore', over='ignore'):
        if gs != F(1):
            g = g * gs
        ns = mom * s + (F(1) - mom) * g * g
        if mutant == 'eps_outside':
            direction = g * (np.sqrt(d) + eps) / (np.sqrt(s) + eps)
        elif mutant == 'dir_new_s':
            direction = g * np.sqrt(d + eps) / np.sqrt(ns + eps)
        else:
            direction = g * np.sqrt(d + eps) / np.sqrt(s + eps)
        if mutant == 'dir_new_d':
            first = mom * d + (F(1) - mom) * direction * direction
            direction = g * np.sqrt(first + eps) / np.sqrt(s + eps)
        nd = mom * d + (F(1) - mom) * direction * direction
        new_p = p - lr * np.where(mu != 0, direction + mu * p, direction)
    assert new_p.dtype == ns.dtype == nd.dtype == F
    return dict(p=new_p, s=ns, d=nd)


# ---- the cases -------------------------------------------------------------------------------------
def segment_table(n_seg, n):
    """the offsets of H.segment_table; multipliers 0, 1, 3, 0.5 in turn, the last one 2.5"""
    off, _ = H.segment_table(n_seg, n)
    reg = np.array([MULTS[k % 4] for k in range(n_seg)], np.float32)
    reg[-1] = 2.5
    assert (np.diff(reg) != 0).all()
    return off, reg


def draw_gradient(rng, n, gs):
    """float32 g with g gs = +-10^e, e spread over H.DECADES and inside [G_LO, G_HI]; 5 % exactly
    zero, among them elements 1 and 2"""
    k = np.asarray(H.DECADES, np.float64)[rng.randint(0, len(H.DECADES), n)]
    e = k + 0.01 + 0.98 * rng.rand(n)
    e[k == max(H.DECADES)] -= 1.0                            # the top decade ends at G_HI
    g = (np.where(rng.rand(n) < 0.5, -1.0, 1.0) * 10.0 ** e / gs).astype(F)
    g[rng.rand(n) < 0.05] = 0
    g[1:3] = 0
    return g


def draw_state(rng, n, gs, all_zero_g=False):
    """p ~ N(0, 1); g as draw_gradient; h, s, d ~ rand 10^2k with k drawn per element, a fifth of
    each exactly zero; element 1: g = 0 on h = 0, element 2: g = 0 on h > 0"""
    def accum():
        k = np.asarray(H.DECADES, np.float64)[rng.randint(0, len(H.DECADES), n)]
        v = (rng.rand(n) * 10.0 ** (2 * k) + 1e-30).astype(F)
        v[rng.rand(n) < 0.2] = 0
        return v
    g = draw_gradient(rng, n, gs)
    if all_zero_g:
        g[:] = 0
    hs = accum()
    hs[1], hs[2] = 0.0, max(hs[2], F(1e-3))
    return dict(p=rng.randn(n).astype(F), g=g, hs=hs, s=accum(), d=accum())


def check_inputs(c):
    """what the case builder promises: |g gs| in [G_LO, G_HI] or exactly 0, g'^2 a normal float32
    number, and so h' == 0 in float32 exactly where it is in float64: g = 0 on h = 0"""
    g = np.asarray(c['g'], np.float64) * c['gs']
    nz = g != 0
    assert ((np.abs(g[nz]) >= G_LO) & (np.abs(g[nz]) <= G_HI)).all()
    g32 = c['g'] * H._gs_f32(c['gdiv'], c['gmul'], None) if c['gs'] != 1.0 else c['g']
    assert g32.dtype == F and ((g32 * g32)[nz] >= np.finfo(F).tiny).all()
    assert (c['hs'] >= 0).all() and (c['s'] >= 0).all() and (c['d'] >= 0).all()
    dead64 = adagrad_ref(c['p'], c['g'], c['hs'], c['mult'], c['h'], c['t0'], c['gs'])[0]['h'] == 0
    dead32 = adagrad_f32(c['p'], c['g'], c['hs'], c['mult'], c['h'], c['t0'], c['gdiv'], c['gmul'])['h'] == 0
    assert np.array_equal(dead64, dead32) and np.array_equal(dead64, ~nz & (c['hs'] == 0))
    assert dead64[1] and not dead64[2] and c['g'][2] == 0


@functools.lru_cache(maxsize=None)
def case(idx, cus=H.HOST_CUS):
    """the inputs of CASES[idx] (float32 arrays; read-only, shared between the tests)"""
    n_seg, kind, t0, hy, gsc, zero_g = CASES[idx]
    n = H.length(kind, n_seg, cus)
    rng = np.random.RandomState(3000 + idx)
    off, reg = segment_table(n_seg, n)
    gdiv, gmul = H.GSCALES[gsc]
    gs = H.grad_scale(gdiv, gmul)
    c = draw_state(rng, n, gs, all_zero_g=(gdiv == 0.0))
    c.update(n=n, seg_off=off, seg_reg=reg, mult=H.per_element(off, reg), t0=t0, h=H.HYPERS[hy],
             gdiv=gdiv, gmul=gmul, gs=gs, zero_g=bool(zero_g))
    check_inputs(c)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def adagrad_expected(c):
    return adagrad_ref(c['p'], c['g'], c['hs'], c['mult'], c['h'], c['t0'], c['gs'])


def adadelta_expected(c):
    return adadelta_ref(c['p'], c['g'], c['s'], c['d'], c['mult'], c['h'], c['gs'])


# ---- the yardsticks --------------------------------------------------------------------------------
# Worst ratio |float32 restatement - float64 restatement| / sum |terms| over CASES (measured by
# test_float32_yardsticks_are_what_is_recorded_here, no kernel involved), per kernel and output.
# Every term is a product or a sum of terms of one sign, so nothing cancels inside a term and all
# of them come out at a few float32 roundings (2^-24 = 6e-8 each).  AdaDelta's d is the largest:
# its second term is the SQUARE of a direction that has six roundings behind it.
YARD = {('adagrad', 'p'): 1.24e-07, ('adagrad', 'h'): 2.37e-07,
        ('adadelta', 'p'): 1.73e-07, ('adadelta', 's'): 2.41e-07, ('adadelta', 'd'): 5.15e-07}
TOLS = dict((k, 4 * v) for k, v in YARD.items())
TOL = max(TOLS.values())


def tolerance(kernel, output):
    return TOLS[kernel, output]


def accept(kernel, got, ref, terms, what):
    """assert the rule for every output; -> {output: worst ratio}"""
    r = H.ratios(got, ref, terms)
    for k, v in r.items():
        assert v <= tolerance(kernel, k), (what, kernel, k, v, tolerance(kernel, k))
    return r


@functools.lru_cache(maxsize=None)
def _host_run(idx, mutant=None):
    """{(kernel, output): ratio} of the float32 restatements (or of a mutant of those it applies
    to) on case idx"""
    c = case(idx)
    out = {}
    if mutant is None or mutant in ADAGRAD_MUTANTS:
        got = adagrad_f32(c['p'], c['g'], c['hs'], c['mult'], c['h'], c['t0'], c['gdiv'], c['gmul'], mutant)
        for k, v in H.ratios(got, *adagrad_expected(c)).items():
            out['adagrad', k] = v
    if mutant is None or mutant in ADADELTA_MUTANTS:
        got = adadelta_f32(c['p'], c['g'], c['s'], c['d'], c['mult'], c['h'], c['gdiv'], c['gmul'], mutant)
        for k, v in H.ratios(got, *adadelta_expected(c)).items():
            out['adadelta', k] = v
    return out


def test_float32_yardsticks_are_what_is_recorded_here():
    worst = dict.fromkeys(YARD, 0.0)
    for idx in range(len(CASES)):
        for k, v in _host_run(idx).items():
            worst[k] = max(worst[k], v)
    print("float32 restatement against float64, worst ratio per output: %s; TOL %.3e"
          % (", ".join("%s %s %.3e" % (a, b, v) for (a, b), v in sorted(worst.items())), TOL))
    for k, v in worst.items():
        assert v <= YARD[k] <= 1.05 * v, (k, v, YARD[k])
    assert TOL == 4 * max(YARD.values()) and max(YARD.values()) < 16 * 2.0 ** -24     # (no output: 16 roundings)


def test_case_table_covers_what_it_claims():
    cols = list(zip(*CASES))
    assert {0, 1, 999} <= set(cols[2]) and set(cols[0]) >= {1, 1024} and set(cols[3]) == {0, 1}
    assert set(cols[4]) == {0, 1, 2, 3} and set(cols[5]) == {0, 1}
    assert {'4', '7', '1028', 'wrap'} <= set(cols[1])
    assert H.length('wrap', 1, H.HOST_CUS) // 4 > 2 * H.HOST_CUS * 256     # beyond one sweep of either grid
    seen = set()
    for idx in range(len(CASES)):
        c = case(idx)                                      # (check_inputs ran when it was built)
        assert c['seg_off'][-1] == c['n'] and c['mult'].shape == (c['n'],) and len(c['seg_reg']) == CASES[idx][0]
        seen |= set(float(v) for v in c['seg_reg'])
        assert c['g'][1] == 0 and c['hs'][1] == 0 and c['g'][2] == 0 and c['hs'][2] > 0
        if c['gdiv'] == 0.0:
            assert not c['g'].any()
        elif c['n'] > 1000:
            assert 0.03 < (c['g'] == 0).mean() < 0.08
            g = np.abs(c['g'][c['g'] != 0].astype(np.float64) * c['gs'])
            assert g.min() < 1e-5 and g.max() > 10.0       # over the eight decades
            for k in ('hs', 's', 'd'):                     # non-zero state, and zeros in it
                assert 0.1 < (c[k] == 0).mean() < 0.3, k
            dead = (c['g'] == 0) & (c['hs'] == 0)
            assert dead.sum() >= 2 and ((c['g'] == 0) & (c['hs'] > 0)).sum() >= 2
    assert seen == {0.0, 1.0, 3.0, 0.5, 2.5}


def test_restatements_are_the_reference_expressions_parameter_by_parameter():
    """the vectorised float64 restatements against the loops over the reference's own expressions:
    c = 2 IS init_func's pass plus the step's; r IS `if p.apply_reg`"""
    for idx in [i for i, c in enumerate(CASES) if c[1] in ('4', '7', '1028', 'seg4099')]:
        c = case(idx)
        ref, terms = adagrad_expected(c)
        for k, v in H.ratios(adagrad_loop(c), ref, terms).items():
            assert v <= 1e-14, ('adagrad', CASE_IDS[idx], k, v)
        ref, terms = adadelta_expected(c)
        for k, v in H.ratios(adadelta_loop(c), ref, terms).items():
            assert v <= 1e-14, ('adadelta', CASE_IDS[idx], k, v)
    assert any(case(i)['t0'] == 0 for i, c in enumerate(CASES) if c[1] in ('4', '7', '1028', 'seg4099'))


def test_terms_are_the_summands():
    c = case(CASE_IDS.index([i for i in CASE_IDS if 'n1028' in i][0]))
    for ref, terms in (adagrad_expected(c), adadelta_expected(c)):
        for k in ref:
            assert (np.abs(ref[k]) <= terms[k] * (1 + 1e-12)).all(), k
        assert (terms['p'] >= 2 * np.abs(ref['p']) - 1e-300).all()


def test_an_element_without_any_gradient_is_left_alone():
    """h' == 0: p and h come back bit for bit from the float32 restatement, where the reference's
    expression gives NaN (0 / 0) or +-inf"""
    c = case(0)
    got = adagrad_f32(c['p'], c['g'], c['hs'], c['mult'], c['h'], c['t0'], c['gdiv'], c['gmul'])
    dead = (c['g'] == 0) & (c['hs'] == 0)
    assert dead[1]
    assert np.array_equal(got['p'][dead].view(np.int32), c['p'][dead].view(np.int32))
    assert not got['h'][dead].any()
    bad = adagrad_f32(c['p'], c['g'], c['hs'], c['mult'], c['h'], c['t0'], c['gdiv'], c['gmul'], 'update_at_h0')
    assert not np.isfinite(bad['p'][dead]).any()


@pytest.mark.parametrize("mutant", sorted(set(ADAGRAD_MUTANTS + ADADELTA_MUTANTS)))
def test_every_mutant_breaks_the_rule_a_hundredfold(mutant):
    """per kernel the mutant applies to: the worst ratio over CASES is at least 100 x its tolerance"""
    worst = {}
    for idx in range(len(CASES)):
        for (kern, k), v in _host_run(idx, mutant).items():
            v /= tolerance(kern, k)
            if v > worst.get(kern, (0.0,))[0]:
                worst[kern] = (v, k, CASE_IDS[idx])
    print("%s: %s" % (mutant, ", ".join("%s %.3g x its tolerance (%s, %s)" % (kern, v, k, cid)
                                        for kern, (v, k, cid) in sorted(worst.items()))))
    assert set(worst) == set(kern for kern, ms in (('adagrad', ADAGRAD_MUTANTS), ('adadelta', ADADELTA_MUTANTS))
                             if mutant in ms)
    for kern, (v, k, cid) in worst.items():
        assert v >= MUTANT_FACTOR, (mutant, kern, v, k, cid)


# ---- the host API ------------------------------------------------------------------------------------
def test_a_model_has_the_four_optimisers_of_the_reference():
    """all four names are in ``model.optimisers`` and each gives its optimiser; SGD and Adam are
    made with the model and are what a fresh model lists (tests/test_host_logic.py), AdaGrad and
    AdaDelta are made, once, when they are first asked for, and listed from then on"""
    from elektronn2_amd import neuromancer as nm
    m = H.smallest_net()
    for name in ('SGD', 'AdaGrad', 'AdaDelta', 'Adam'):
        assert name in m.optimisers
    assert 'RMSProp' not in m.optimisers and m.optimisers.get('RMSProp') is None
    with pytest.raises(KeyError):
        m.optimisers['RMSProp']
    assert set(m.optimisers) == {'SGD', 'Adam'}
    ag, ad = m.optimisers['AdaGrad'], m.optimisers.get('AdaDelta')
    assert type(ag) is nm.AdaGrad and type(ad) is nm.AdaDelta
    assert m.optimisers['AdaGrad'] is ag and m.optimisers['AdaDelta'] is ad
    assert set(m.optimisers) == {'SGD', 'AdaGrad', 'AdaDelta', 'Adam'}
    assert nm.AdaGrad.step_name == 'AdaGrad' and nm.AdaDelta.step_name == 'AdaDelta'
    for opt in (ag, ad):
        assert set(opt.meta_params) == {'lr', 'mom', 'wd'} and opt.model is m
        assert opt.step.func is None and opt.state_dict() == {}       # nothing planned or allocated yet
    assert ag.hs is None and ag.t == 0.0
    assert ad.squared_accum is None and ad.delta_accum is None


def test_meta_params_are_the_shared_ones():
    m = H.smallest_net()
    m.set_opt_meta_params('AdaDelta', dict(lr=0.25, mom=0.95))
    assert abs(m.lr - 0.25) < 1e-8 and abs(m.optimisers['SGD'].global_lr.get_value() - 0.25) < 1e-8
    assert abs(m.optimisers['Adam'].global_mom.get_value() - 0.95) < 1e-7
    m.set_opt_meta_params('AdaGrad', dict(wd=0.125))
    assert m.wd == 0.125
    for name in ('AdaGrad', 'AdaDelta'):
        with pytest.raises(AttributeError):
            m.set_opt_meta_params(name, dict(beta2=0.5))


def test_state_dicts_survive_load_save_load_before_any_step(tmp_path):
    """as tests/test_checkpoint.py does for Adam and SGD: the state is parked until the first step
    makes the buffers, and save() hands the parked state on"""
    from elektronn2_amd.neuromancer.model import modelload
    a = H.smallest_net()
    n = 64
    rng = np.random.RandomState(12)
    h0, s0, d0 = (rng.rand(n).astype(np.float32) for _ in range(3))
    a.optimisers['AdaGrad'].load_state_dict({'h': h0, 't': 7})
    a.optimisers['AdaDelta'].load_state_dict({'s': s0, 'd': d0})
    f1, f2 = str(tmp_path / "one.mdl"), str(tmp_path / "two.mdl")
    a.save(f1)
    b = modelload(f1, name='b')
    b.save(f2)                                   # load -> save, still no step
    raw = np.load(f2)
    assert {'o/AdaGrad/h', 'o/AdaGrad/t', 'o/AdaDelta/s', 'o/AdaDelta/d'} <= set(raw.files)
    c = modelload(f2, name='c')
    st = c.optimisers['AdaGrad'].state_dict()
    assert float(st['t']) == 7.0 and c.optimisers['AdaGrad'].t == 7.0 and np.array_equal(st['h'], h0)
    st = c.optimisers['AdaDelta'].state_dict()
    assert np.array_equal(st['s'], s0) and np.array_equal(st['d'], d0)
    # the resettable part of repair()
    c.optimisers['AdaGrad'].clear_last_dir()
    c.optimisers['AdaDelta'].clear_last_dir()
    assert c.optimisers['AdaGrad'].t == 0.0
    assert c.optimisers['AdaGrad'].state_dict() == {} and c.optimisers['AdaDelta'].state_dict() == {}
    # a file from before the two optimisers existed: no o/AdaGrad, o/AdaDelta keys
    old = dict((k, raw[k]) for k in raw.files if not k.startswith(('o/AdaGrad', 'o/AdaDelta')))
    f3 = str(tmp_path / "old.mdl")
    with open(f3, 'wb') as fh:
        np.savez(fh, **old)
    d = modelload(f3, name='d')
    assert d.optimisers['AdaGrad'].state_dict() == {} and d.optimisers['AdaGrad'].t == 0.0


class _NoStep(object):
    last_exec_time = 0.0

    def __init__(self):
        self.calls = 0

    def __call__(self, *args, **kwargs):
        self.calls += 1
        return [np.float32(0.5)]


def test_an_unknown_name_still_falls_back_to_sgd(caplog):
    """... and the four names do not: each reaches its own optimiser"""
    m = H.smallest_net()
    stubs = dict((k, _NoStep()) for k in ('SGD', 'AdaGrad', 'AdaDelta', 'Adam'))
    m.optimisers = stubs
    x, t = H.net_batch()
    with caplog.at_level(logging.WARNING):
        m.trainingstep(x, t, optimiser='RMSProp')
    assert "No optimiser 'RMSProp'. Falling back to SGD" in caplog.text
    assert [stubs[k].calls for k in ('SGD', 'AdaGrad', 'AdaDelta', 'Adam')] == [1, 0, 0, 0]
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        for name in ('AdaGrad', 'AdaDelta'):
            m.trainingstep(x, t, optimiser=name)
    assert "Falling back" not in caplog.text
    assert [stubs[k].calls for k in ('SGD', 'AdaGrad', 'AdaDelta', 'Adam')] == [1, 1, 1, 0]


def test_the_plan_asks_one_predicate_whether_a_step_updates():
    """no literal tuple of step names is left where the plan or a node decides what an updating
    step does; adam_pack stays Adam's"""
    import inspect
    from elektronn2_amd.neuromancer import plan, neural
    assert set(plan.UPDATE_STEPS) == {'SGD', 'AdaGrad', 'AdaDelta', 'Adam'}
    for mod in (plan, neural):
        src = inspect.getsource(mod)
        assert "('Adam', 'SGD')" not in src and "('SGD', 'Adam')" not in src
    assert inspect.getsource(plan).count("self.updates_params()") >= 7
    assert inspect.getsource(neural).count("plan.updates_params()") == 3
    assert "self.step != 'Adam'" in inspect.getsource(plan.Plan._plan_fused_update)
