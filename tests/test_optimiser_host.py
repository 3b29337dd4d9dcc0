"""Adam / SGD updates (csrc/arena_ops.hip adam_kernel, sgd_kernel; csrc/update_pack.hip
adam_pack_kernel; optimiser.py:146-160, :301-329 of the reference), host side (no GPU): what
tests/test_optimiser_gpu.py compares the kernels with, and the evidence that its rule can see what
the kernels compute.

* ``adam_ref`` / ``sgd_ref``: a float64, element-wise restatement of both updates over a
  per-element weight-decay multiplier and the gradient scale gs.  ``O.adam_step`` / ``O.sgd_step``
  stay the definition; the restatement is pinned against them segment by segment.
* ``CASES``: inputs in which every term of the update is of the same order -- lr 0.05, wd 0.5,
  gradients and state over eight decades (the eps-dominated and the s-dominated regime of Adam in
  every case), non-zero state, step counters 0 .. 999, segment tables of 1 .. 1024 four-element
  segments whose multipliers differ between neighbours, lengths with and without a scalar tail
  and beyond one sweep of the grids.
* the acceptance rule: |got - ref| <= TOL * sum |terms| element by element, against the terms
  that are SUMMED and not against the result (mom m + (1 - mom) g cancels).
* ``TOL``: 4 x the worst ratio of a float32 NumPy restatement in the kernels' operation order
  against the float64 one, measured here, without any kernel.  p's third term lr |dir| is itself
  a sum that cancels, which puts that yardstick at 1.1e-5; ``TOL_SUMMED`` is the same rule with
  the summands of dir in its place, 1.3e-7 like m, s and d.  The kernels must pass both.
* mutants of the float32 restatement -- no weight decay, multipliers one float4 off, eps outside
  the root, ... -- each of which must break the rule by at least 100 x on some case.
* ``variables.reg_multiplier``: the weight-decay multiplier of a parameter (``apply_reg`` only
  where it is > 1)."""
import functools

import numpy as np
import pytest

from oracle import e2_oracle as O

EPS = 1e-5                                   # EPS_ADAM, inside the root
GDIV_EPS = 1e-5                              # gs = gmul / (gdiv + 1e-5)
F = np.float32


def f32(v):
    return float(np.float32(v))


# float32-representable: the reference gets what the device array holds
HYPERS = [dict(lr=f32(0.05), mom=f32(0.9), b2=f32(0.999), wd=f32(0.5)),
          dict(lr=f32(0.05), mom=f32(0.9), b2=f32(0.999), wd=0.0)]
T0S = [0, 1, 9, 999]
N_SEGS = [1, 2, 3, 1023, 1024]
N_KINDS = ['4', '7', '1024', '1028', 'seg4099', 'wrap']
GSCALES = [(None, 1.0), (None, 0.125), (1234.0, 1.0), (0.0, 1.0)]      # (gdiv, gmul); the last: g = 0
DECADES = [-6, -4, -3, -2, 0, 2]
HOST_CUS = 256


# ---- the float64 restatement ---------------------------------------------------------------------
def bias_factor(t, mom, b2):
    return float(np.sqrt(1.0 - float(b2) ** t) / (1.0 - float(mom) ** t))


def grad_scale(gdiv, gmul):
    return float(gmul) / (float(gdiv) + GDIV_EPS) if gdiv is not None else float(gmul)


def _f64(*a):
    return [np.asarray(v, np.float64) for v in a]


def adam_ref(p, g, m, s, mult, h, fac, gs=1.0):
    """-> ({p, m, s}, {p, m, s}: the sum of the absolute terms of each).  ``mult``: the multiplier
    of every element (0: no decay); ``fac``: the bias factor sqrt(1 - b2^t) / (1 - mom^t)."""
    p, g, m, s, mult = _f64(p, g, m, s, mult)
    lr, mom, b2, wd = h['lr'], h['mom'], h['b2'], h['wd']
    g = g * gs
    nm = mom * m + (1.0 - mom) * g
    ns = b2 * s + (1.0 - b2) * g * g
    direction = fac * nm / np.sqrt(ns + EPS)
    new_p = p - lr * (direction + wd * mult * p)
    decay = lr * wd * mult * np.abs(p)
    terms = dict(p=np.abs(p) + np.abs(new_p) + lr * np.abs(direction) + decay,
                 m=np.abs(mom * m) + np.abs((1.0 - mom) * g),
                 s=np.abs(b2 * s) + np.abs((1.0 - b2) * g * g))
    # the direction is itself built on a sum that cancels: with ITS summands in place of its value
    terms['p_summed'] = np.abs(p) + np.abs(new_p) + lr * fac * terms['m'] / np.sqrt(ns + EPS) + decay
    return dict(p=new_p, m=nm, s=ns), terms


def sgd_ref(p, g, d, mult, h, gs=1.0):
    """-> ({p, d}, {p, d}: the sum of the absolute terms of each)"""
    p, g, d, mult = _f64(p, g, d, mult)
    lr, mom, wd = h['lr'], h['mom'], h['wd']
    g = g * gs
    nd = g + mom * d
    new_p = p - lr * (nd + wd * mult * p)
    decay = lr * wd * mult * np.abs(p)
    terms = dict(p=np.abs(p) + np.abs(new_p) + lr * np.abs(nd) + decay,
                 d=np.abs(g) + np.abs(mom * d))
    terms['p_summed'] = np.abs(p) + np.abs(new_p) + lr * terms['d'] + decay
    return dict(p=new_p, d=nd), terms


def ratios(got, ref, terms):
    """{output: worst |got - ref| / sum |terms|}; anything not finite, or a difference where no
    term is, counts as infinite"""
    out = {}
    for k in terms:
        r = ref[k.split('_')[0]]
        a = np.asarray(got[k.split('_')[0]], np.float64)
        assert a.shape == r.shape, (k, a.shape, r.shape)
        if not np.isfinite(a).all():
            out[k] = float('inf')
            continue
        diff, t = np.abs(a - r), terms[k]
        if (diff[t == 0] != 0).any():
            out[k] = float('inf')
            continue
        nz = t > 0
        out[k] = float((diff[nz] / t[nz]).max()) if nz.any() else 0.0
    return out


def fac_bound(t, mom, b2):
    """1 - b2^t cancels in float32: an inherent relative error of 2^-25 / (1 - b2^t) in the root
    and 2^-24 / (1 - mom^t) in the divisor; x 4 as for TOL"""
    return 4.0 * (2.0 ** -25 / (1.0 - float(b2) ** t) + 2.0 ** -24 / (1.0 - float(mom) ** t))


# ---- the float32 restatements, in the kernels' operation order -------------------------------------
def fac_f32(t, mom, b2):
    one = F(1)
    return np.sqrt(one - np.power(F(b2), F(t))) / (one - np.power(F(mom), F(t)))


def _gs_f32(gdiv, gmul, mutant):
    if mutant == 'gs_ignored':
        return F(1)
    if gdiv is None:
        return F(gmul)
    with np.errstate(divide='ignore'):
        return F(gmul) / (F(gdiv) if mutant == 'gdiv_no_eps' else F(gdiv) + F(1e-5))


def _mult_f32(mult, wd, mutant):
    mult = np.asarray(mult, F)
    if mutant == 'no_wd':
        mult = np.zeros_like(mult)
    elif mutant == 'mult_shift4':                       # the multiplier of the float4 behind
        mult = np.concatenate([mult[4:], mult[-4:]])[:mult.size]
    elif mutant == 'mult_clamp1':
        mult = np.minimum(mult, F(1))
    return mult * F(wd)


def adam_f32(p, g, m, s, mult, h, t0, gdiv=None, gmul=1.0, mutant=None):
    """adam_kernel's arithmetic, one rounding per operation (no contraction) -> ({p, m, s}, fac)"""
    p, g, m, s = (np.asarray(v, F) for v in (p, g, m, s))
    lr, mom, b2 = F(h['lr']), F(h['mom']), F(h['b2'])
    t = t0 + 1 + (1 if mutant == 't_off_by_one' else 0)
    fac = F(1) if mutant == 'fac_one' else fac_f32(t, mom, b2)
    gs = _gs_f32(gdiv, gmul, mutant)
    mu = _mult_f32(mult, h['wd'], mutant)
    with np.errstate(invalid='ignore', over='ignore'):
        if gs != F(1):
            g = g * gs
        nm = mom * m + (F(1) - mom) * g
        ns = b2 * s + (F(1) - b2) * g * g
        if mutant == 'eps_outside':
            direction = fac * nm / (np.sqrt(ns) + F(EPS))
        else:
            direction = fac * nm / np.sqrt(ns + F(EPS))
        direction = np.where(mu != 0, direction + mu * p, direction)
        new_p = p - lr * direction
    assert new_p.dtype == nm.dtype == ns.dtype == F
    return dict(p=new_p, m=nm, s=ns), float(fac)


def sgd_f32(p, g, d, mult, h, gdiv=None, gmul=1.0, mutant=None):
    p, g, d = (np.asarray(v, F) for v in (p, g, d))
    lr, mom = F(h['lr']), F(h['mom'])
    gs = _gs_f32(gdiv, gmul, mutant)
    mu = _mult_f32(mult, h['wd'], mutant)
    with np.errstate(invalid='ignore', over='ignore'):
        if gs != F(1):
            g = g * gs
        nd = g if mutant == 'sgd_no_mom' else g + mom * d
        new_p = p - lr * np.where(mu != 0, nd + mu * p, nd)
    assert new_p.dtype == nd.dtype == F
    return dict(p=new_p, d=nd)


# ---- the cases -------------------------------------------------------------------------------------
def length(kind, n_seg, cus):
    if kind == 'seg4099':
        return 4 * n_seg + 4099
    if kind == 'wrap':                                   # beyond one sweep of SGD's 2 x CUs work-groups
        return 2048 * cus + 1203
    return int(kind)


def _specs():
    """(n_seg, length kind, t0, hyper set, gradient scaling, zero_g): every (n_seg, length) pair
    that fits -- all but the last segment are four elements long --, twice, with the other
    choices cycled so that each value meets each length"""
    pairs = [(ns, k) for k in N_KINDS for ns in N_SEGS if length(k, ns, HOST_CUS) >= 4 * (ns - 1) + 1]
    out = []
    for rnd in range(2):
        for i, (ns, k) in enumerate(pairs):
            j = i + 3 * rnd
            out.append((ns, k, T0S[(j + rnd) % 4], (i + rnd) % 2, (j // 2 + 2 * rnd + i) % 4, (j + i // 4) % 2))
    return out


CASES = _specs()
CASE_IDS = ["seg%d_n%s_t%d_h%d_gs%d_z%d" % c for c in CASES]


def segment_table(n_seg, n):
    """offsets (n_seg + 1), multipliers (n_seg): four-element segments, the last takes the rest;
    multipliers 0, 1, 2 + (k mod 7) in turn, the last one 2.5"""
    off = np.concatenate([4 * np.arange(n_seg), [n]]).astype(np.int64)
    reg = np.array([(0.0, 1.0, 2.0 + (k % 7))[k % 3] for k in range(n_seg)], np.float32)
    reg[-1] = 2.5
    assert (np.diff(off) > 0).all() and (np.diff(reg) != 0).all()
    return off, reg


def per_element(off, reg):
    return np.repeat(np.asarray(reg, np.float64), np.diff(off))


def draw_state(rng, n, zero_g=False):
    """p ~ N(0, 1); g, m, d ~ randn 10^k and s ~ rand 10^2k with k drawn per element; 5 % of the
    gradients exactly zero (all of them: ``zero_g``)"""
    k = np.asarray(DECADES, np.float64)[rng.randint(0, len(DECADES), n)]
    g = rng.randn(n) * 10.0 ** k
    g[rng.rand(n) < 0.05] = 0.0
    if zero_g:
        g[:] = 0.0
    return dict(p=rng.randn(n).astype(F), g=g.astype(F), m=(rng.randn(n) * 10.0 ** k).astype(F),
                d=(rng.randn(n) * 10.0 ** k).astype(F), s=(rng.rand(n) * 10.0 ** (2 * k)).astype(F))


@functools.lru_cache(maxsize=None)
def case(idx, cus=HOST_CUS):
    """the inputs of CASES[idx] (float32 arrays; read-only, shared between the tests)"""
    n_seg, kind, t0, hy, gsc, zero_g = CASES[idx]
    n = length(kind, n_seg, cus)
    rng = np.random.RandomState(1000 + idx)
    off, reg = segment_table(n_seg, n)
    gdiv, gmul = GSCALES[gsc]
    c = draw_state(rng, n, zero_g=(gdiv == 0.0))
    c.update(n=n, seg_off=off, seg_reg=reg, mult=per_element(off, reg), t0=t0, h=HYPERS[hy],
             gdiv=gdiv, gmul=gmul, gs=grad_scale(gdiv, gmul), zero_g=bool(zero_g))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def adam_expected(c, fac):
    return adam_ref(c['p'], c['g'], c['m'], c['s'], c['mult'], c['h'], fac, c['gs'])


def sgd_expected(c):
    return sgd_ref(c['p'], c['g'], c['d'], c['mult'], c['h'], c['gs'])


# ---- the yardsticks --------------------------------------------------------------------------------
# Worst ratio |float32 restatement - float64 restatement| / sum |terms| over CASES (measured by
# test_float32_yardsticks_are_what_is_recorded_here, no kernel involved), per output.  'p' is
# measured against |p_old| + |p_new| + lr |dir| + lr mult |p_old|.  Its third term is no summand
# but a sum that cancels (Adam: dir = fac (mom m + (1 - mom) g) / root; SGD: dir = g + mom d), so
# where it cancels the float32 error of p is 1e-5 of these terms and the yardstick is set by the
# rarest cancellation in the table: 90 times the others.  'p_summed' takes the summands of dir
# in place of dir and comes out where m, s and d do.
YARD = dict(p=1.14e-05, m=1.17e-07, s=1.18e-07, d=1.17e-07, p_summed=1.34e-07)
# 4 x the worst ratio.  The margin is for the device's powf, sqrtf and division, which are not
# correctly rounded, and for the contraction of a * b + c into one fma.  TOL is the rule with the
# terms as first listed; TOL_SUMMED holds m, s, d -- the same terms, so TOL a fortiori -- and p
# against its summands.  A kernel has to pass both.
TOL = 4 * max(YARD[k] for k in 'pmsd')
TOL_SUMMED = 4 * max(YARD[k] for k in ('p_summed', 'm', 's', 'd'))
MUTANT_FACTOR = 100.0


def tolerance(output, extra=0.0):
    return (TOL if output == 'p' else TOL_SUMMED) + extra


def accept(got, ref, terms, what, extra=0.0):
    """assert the rule for every output; -> {output: worst ratio}"""
    r = ratios(got, ref, terms)
    for k, v in r.items():
        assert v <= tolerance(k, extra), (what, k, v, tolerance(k, extra))
    return r


@functools.lru_cache(maxsize=None)
def _host_run(idx, mutant=None):
    """{('adam' | 'sgd', output): ratio} of the float32 restatement (or a mutant of it) on case idx;
    the reference takes the float32 bias factor of the UNMUTATED restatement, as the GPU test
    takes the kernel's"""
    c = case(idx)
    fac = float(fac_f32(c['t0'] + 1, c['h']['mom'], c['h']['b2']))
    out = {}
    if mutant != 'sgd_no_mom':
        got, _ = adam_f32(c['p'], c['g'], c['m'], c['s'], c['mult'], c['h'], c['t0'], c['gdiv'], c['gmul'], mutant)
        for k, v in ratios(got, *adam_expected(c, fac)).items():
            out['adam', k] = v
    if mutant not in ('eps_outside', 'fac_one', 't_off_by_one'):
        got = sgd_f32(c['p'], c['g'], c['d'], c['mult'], c['h'], c['gdiv'], c['gmul'], mutant)
        for k, v in ratios(got, *sgd_expected(c)).items():
            out['sgd', k] = v
    return out


def test_float32_yardsticks_are_what_is_recorded_here():
    worst = dict.fromkeys(YARD, 0.0)
    for idx in range(len(CASES)):
        for (_, k), v in _host_run(idx).items():
            worst[k] = max(worst[k], v)
    print("float32 restatement against float64, worst ratio per output: %s; TOL %.3e, TOL_SUMMED %.3e"
          % (", ".join("%s %.3e" % kv for kv in sorted(worst.items())), TOL, TOL_SUMMED))
    for k, v in worst.items():
        assert v <= YARD[k] <= 1.05 * v, (k, v, YARD[k])
    assert TOL_SUMMED < 6e-7 and TOL < 5e-5


def test_case_table_covers_what_it_claims():
    assert len(CASES) == len(set(CASES))
    cols = list(zip(*CASES))
    assert set(cols[0]) == set(N_SEGS) and set(cols[1]) == set(N_KINDS) and set(cols[2]) == set(T0S)
    assert set(cols[3]) == {0, 1} and set(cols[4]) == {0, 1, 2, 3} and set(cols[5]) == {0, 1}
    for ns in (1023, 1024):                               # the long tables: short and wrapping
        assert {c[1] for c in CASES if c[0] == ns} == {'seg4099', 'wrap'}
    for kind in ('1024', '1028', 'seg4099', 'wrap'):      # every scaling, both zero_g, at every length
        assert {c[4] for c in CASES if c[1] == kind} == {0, 1, 2, 3}, kind
        assert {c[5] for c in CASES if c[1] == kind} == {0, 1}, kind
    for idx in range(len(CASES)):
        c = case(idx)
        n_seg = CASES[idx][0]
        assert c['seg_off'][0] == 0 and c['seg_off'][-1] == c['n'] and c['mult'].shape == (c['n'],)
        assert (np.diff(c['seg_off'])[:-1] == 4).all() and c['seg_reg'][-1] == 2.5
        assert len(c['seg_reg']) == n_seg
        if c['gdiv'] == 0.0:
            assert not c['g'].any()
        elif c['n'] > 1000:
            # both regimes of Adam's root: the new s far below and far above eps
            ns = adam_expected(c, 1.0)[0]['s']
            assert (ns < 1e-2 * EPS).mean() > 0.2 and (ns > 1e2 * EPS).mean() > 0.2
            assert 0.03 < (c['g'] == 0).mean() < 0.08
        assert c['m'].all() and c['d'].all() and (c['s'] > 0).all()
    assert length('wrap', 1, HOST_CUS) // 4 > 2 * HOST_CUS * 256      # SGD's grid wraps


def test_restatement_is_the_oracle_segment_by_segment():
    """O.adam_step / O.sgd_step stay the definition: the restatement vectorises them over the
    segment table (the oracle has no gradient scale: it gets the scaled gradient)"""
    for idx in [i for i, c in enumerate(CASES) if c[1] in ('7', '1028', 'seg4099')]:
        c = case(idx)
        h, t = c['h'], c['t0'] + 1
        p, g, m, s, d = _f64(c['p'], c['g'], c['m'], c['s'], c['d'])
        got_a, _ = adam_expected(c, bias_factor(t, h['mom'], h['b2']))
        got_s, _ = sgd_expected(c)
        off = c['seg_off']
        for k, reg in enumerate(c['seg_reg']):
            sl = slice(off[k], off[k + 1])
            want = O.adam_step(p[sl], g[sl] * c['gs'], m[sl], s[sl], t, h['lr'], h['mom'], h['b2'], h['wd'], float(reg))
            for key, w in zip('pms', want):
                np.testing.assert_allclose(got_a[key][sl], w, rtol=1e-13, atol=0)
            want = O.sgd_step(p[sl], g[sl] * c['gs'], d[sl], h['lr'], h['mom'], h['wd'], float(reg))
            for key, w in zip('pd', want):
                np.testing.assert_allclose(got_s[key][sl], w, rtol=1e-13, atol=0)


def test_terms_are_the_summands():
    """the rule's denominators: each output is a signed sum of exactly the terms that are added up"""
    c = case(CASE_IDS.index([i for i in CASE_IDS if 'n1028' in i][0]))
    ref, terms = adam_expected(c, 0.7)
    for k in ref:
        assert (np.abs(ref[k]) <= terms[k] * (1 + 1e-12)).all(), k
    assert (terms['p'] >= 2 * np.abs(ref['p']) - 1e-300).all()
    ref, terms = sgd_expected(c)
    for k in ref:
        assert (np.abs(ref[k]) <= terms[k] * (1 + 1e-12)).all(), k


@pytest.mark.parametrize("t", [1, 2, 10, 1000])
def test_bias_factor_in_float32_is_inside_its_bound(t):
    h = HYPERS[0]
    want = bias_factor(t, h['mom'], h['b2'])
    got = float(fac_f32(t, h['mom'], h['b2']))
    e, b = abs(got - want) / want, fac_bound(t, h['mom'], h['b2'])
    print("t = %d: fac %.9g, float32 %.9g, relative error %.2e, bound %.2e" % (t, want, got, e, b))
    assert e <= b
    # and the bound notices a step counter one off
    assert abs(bias_factor(t + 1, h['mom'], h['b2']) - want) / want > 2 * b


MUTANTS = ['no_wd', 'mult_shift4', 'mult_clamp1', 'eps_outside', 'fac_one', 't_off_by_one', 'sgd_no_mom',
           'gs_ignored', 'gdiv_no_eps']


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_breaks_the_rule_a_hundredfold(mutant):
    """per kernel the mutant applies to: the worst ratio over CASES is at least 100 x TOL"""
    worst = {}
    for idx in range(len(CASES)):
        for (kern, k), v in _host_run(idx, mutant).items():
            v /= tolerance(k)
            if v > worst.get(kern, (0.0,))[0]:
                worst[kern] = (v, k, CASE_IDS[idx])
    print("%s: %s" % (mutant, ", ".join("%s %.3g x its tolerance (%s, %s)" % (kern, v, k, cid)
                                        for kern, (v, k, cid) in sorted(worst.items()))))
    assert worst
    for kern, (v, k, cid) in worst.items():
        assert v >= MUTANT_FACTOR, (mutant, kern, v, k, cid)


def test_t_off_by_one_shows_even_at_the_last_step_counter():
    """the weakest mutant where it is weakest: t0 = 999, where fac moves by 3e-4 a step"""
    worst = max(v / tolerance(k) for idx, c in enumerate(CASES) if c[2] == 999
                for (_, k), v in _host_run(idx, 't_off_by_one').items())
    print("t off by one at t0 = 999: %.3g x its tolerance" % worst)
    assert worst >= MUTANT_FACTOR


# ---- the multiplier rule ---------------------------------------------------------------------------
class _P(object):
    def __init__(self, apply_reg):
        self.apply_reg = apply_reg


@pytest.mark.parametrize("apply_reg,want", [(False, 0.0), (True, 1.0), (1, 1.0), (3.0, 3.0), (0.5, 1.0),
                                            (1.0, 1.0), (0, 0.0), (np.float32(3.0), 3.0)])
def test_reg_multiplier(apply_reg, want):
    """optimiser.py:148-155 of the reference: ``apply_reg`` itself only where it is > 1"""
    from elektronn2_amd.neuromancer.variables import reg_multiplier
    got = reg_multiplier(_P(apply_reg))
    assert type(got) is float and got == want
    # ... which is what the oracle's steps do with the same value
    p, g = np.array([1.5]), np.array([0.25])
    h = HYPERS[0]
    new_p, _ = O.sgd_step(p, g, 0.0, h['lr'], 0.0, h['wd'], apply_reg)
    assert abs(new_p[0] - sgd_ref(p, g, [0.0], [got], dict(h, mom=0.0))[0]["p"][0]) < 1e-15


def test_model_and_plan_use_the_one_helper():
    import inspect
    from elektronn2_amd.neuromancer import model, plan, variables
    assert model.reg_multiplier is variables.reg_multiplier is plan.reg_multiplier
    assert 'reg_multiplier' in inspect.getsource(model.Model.ensure_arena)
    assert 'reg_multiplier' in inspect.getsource(plan.Plan._plan_fused_update)
    for fn in (model.Model.ensure_arena, plan.Plan._plan_fused_update):
        assert 'apply_reg' not in inspect.getsource(fn)


# ---- the smallest net of tests/test_optimiser_gpu.py ------------------------------------------------
NET_HYPER = dict(lr=f32(0.05), mom=f32(0.9), wd=f32(0.5))
NET_B2 = f32(0.999)


def smallest_net(fractional=False, seed=71):
    """Conv (1,3,3) with batch norm in train mode -> (1,1,1) 'lin' Conv -> softmax -> NLL on a
    (1, 1, 3, 12, 12) input: multipliers 1 (w), 0 (b), 3 (gamma).  ``fractional``: the head's
    weight is registered with apply_reg = 0.5 before anything is planned."""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((1, 1, 3, 12, 12), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 5, (1, 3, 3), batch_normalisation='train', name='c0')
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin', name='head')
    probs = nm.Softmax(out)
    target = nm.Input_like(probs, override_f=1, name='target')
    loss = nm.AggregateLoss(nm.MultinoulliNLL(probs, target, target_is_sparse=True), name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=probs,
                          prediction_ext=[loss, probs])
    if fractional:
        model.nodes['head'].params['w'].apply_reg = 0.5
    model.set_opt_meta_params('SGD', NET_HYPER)
    model.set_opt_meta_params('Adam', dict(NET_HYPER, beta2=NET_B2))
    return model


def net_batch(seed=72):
    rng = np.random.RandomState(seed)
    return (rng.rand(1, 1, 3, 12, 12).astype(np.float32),
            rng.randint(0, 2, (1, 1, 3, 10, 10)).astype(np.float32))


@pytest.mark.parametrize("fractional", [False, True])
def test_smallest_net_carries_the_three_multipliers(fractional):
    from elektronn2_amd.neuromancer.variables import reg_multiplier
    m = smallest_net(fractional)
    params = m.loss_node.all_trainable_params
    mult = dict((k, reg_multiplier(p)) for k, p in params.items())
    print(mult)
    assert sorted(set(mult.values())) == [0.0, 1.0, 3.0]
    for k, v in mult.items():
        kind = k.rsplit('_', 1)[-1]
        assert v == dict(w=1.0, b=0.0, gamma=3.0)[kind], (k, v)
    assert (params['head_w'].apply_reg == 0.5) == fractional
