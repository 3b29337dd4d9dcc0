"""Adam / SGD updates on the GPU (csrc/arena_ops.hip: e2_adam_step_ex, e2_sgd_step_ex;
csrc/update_pack.hip: e2_adam_pack_step) against the float64 restatement of
tests/test_optimiser_host.py -- never the code under test -- on its case table: every output
(p, m, s / p, d, the step counter, the published bias factor, the arrival counter, the gradient
arena) under the rule |got - ref| <= TOL sum |terms| with the tolerances measured there; three
steps in a row with a changed lr; captured and replayed steps; the refusals; and a smallest net
whose SGD and Adam steps are checked tensor by tensor, teacher-forced on the model's own gradients,
with a weight registered with a fractional ``apply_reg``.

The bias factor 1 - b2^t cancels in float32 (3e-5 relative at t = 1): the element-wise reference
takes the factor the kernel publishes in hyper[5], and the factor itself is held to the float64
formula within ``fac_bound``."""
import numpy as np
import pytest
import torch

import test_optimiser_host as H
from test_optimiser_host import CASES, CASE_IDS

pytestmark = pytest.mark.gpu

# the project's bound for the float32-atomics noise of parameter gradients between two evaluations,
# as a fraction of the tensor's largest element (tests/test_bf16_gpu.py, measured <= 2.4e-7): where
# the model-level reference gets its gradients from model.gradients(), the step computes its own
GRAD_NOISE = 2e-6

WORST = {}


def note(kind, r):
    for k, v in r.items():
        WORST[kind, k] = max(WORST.get((kind, k), 0.0), v)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst ratio per output (tolerances: p %.3e, the others %.3e): %s"
          % (H.TOL, H.TOL_SUMMED, ", ".join("%s %s %.3e" % (a, b, v) for (a, b), v in sorted(WORST.items()))))


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def hyper_dev(h, t0, floats=8):
    return dev([h['lr'], h['mom'], h['b2'], h['wd'], t0, 0, 0, 0] + [0] * (floats - 8))


def check_counter_and_factor(hyp, h, t0, what):
    """t = t0 + 1, the arrival counter back at integer 0, lr .. wd untouched; -> the published fac,
    checked against the float64 formula"""
    hv = host(hyp)
    assert hv[4] == t0 + 1, (what, hv[4])
    assert int(hyp.view(torch.int32)[7]) == 0, what
    assert np.array_equal(hv[:4], np.array([h['lr'], h['mom'], h['b2'], h['wd']], np.float32)), what
    fac, want = float(hv[5]), H.bias_factor(t0 + 1, h['mom'], h['b2'])
    e = abs(fac - want) / want
    assert e <= H.fac_bound(t0 + 1, h['mom'], h['b2']), (what, fac, want, e)
    note('fac', dict(fac=e / H.fac_bound(t0 + 1, h['mom'], h['b2'])))
    return fac


def upload(c, keys):
    so = torch.tensor(c['seg_off'], device="cuda")
    sr = dev(c['seg_reg'])
    gdiv = dev([c['gdiv']]) if c['gdiv'] is not None else None
    return [dev(c[k]) for k in keys], so, sr, gdiv


def check_gradient_arena(G, c, what):
    if c['zero_g']:
        assert not G.any(), what
    else:
        assert same_bits(G, dev(c['g'])), what


# ---- A. the two sweeps over the case table -----------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_adam_step_against_the_restatement(ctx, idx):
    c = H.case(idx, cus())
    (P, G, M, S), so, sr, gdiv = upload(c, 'pgms')
    hyp = hyper_dev(c['h'], c['t0'])
    ctx.adam_step(P, G, M, S, so, sr, hyp, gdiv=gdiv, gmul=c['gmul'], zero_g=c['zero_g'])
    torch.cuda.synchronize()
    fac = check_counter_and_factor(hyp, c['h'], c['t0'], CASE_IDS[idx])
    ref, terms = H.adam_expected(c, fac)
    r = H.ratios(dict(p=host(P), m=host(M), s=host(S)), ref, terms)
    print(CASE_IDS[idx], "n = %d, fac %.9g:" % (c['n'], fac), ", ".join("%s %.2e" % kv for kv in r.items()))
    note('adam', r)
    H.accept(dict(p=host(P), m=host(M), s=host(S)), ref, terms, CASE_IDS[idx])
    check_gradient_arena(G, c, CASE_IDS[idx])
    assert torch.equal(so, torch.tensor(c['seg_off'], device="cuda")) and same_bits(sr, dev(c['seg_reg']))


@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_sgd_step_against_the_restatement(ctx, idx):
    c = H.case(idx, cus())
    (P, G, D), so, sr, gdiv = upload(c, 'pgd')
    hyp = hyper_dev(c['h'], c['t0'])
    before = hyp.clone()
    ctx.sgd_step(P, G, D, so, sr, hyp, gdiv=gdiv, gmul=c['gmul'], zero_g=c['zero_g'])
    torch.cuda.synchronize()
    assert same_bits(hyp, before)                                  # SGD keeps no counter
    ref, terms = H.sgd_expected(c)
    r = H.ratios(dict(p=host(P), d=host(D)), ref, terms)
    print(CASE_IDS[idx], "n = %d:" % c['n'], ", ".join("%s %.2e" % kv for kv in r.items()))
    note('sgd', r)
    H.accept(dict(p=host(P), d=host(D)), ref, terms, CASE_IDS[idx])
    check_gradient_arena(G, c, CASE_IDS[idx])


def check_tail_repeats_the_vector_body(launch, st, keys):
    """an arena of 4 * 256 + 3 elements, ONE segment with the multiplier 2.5, whose last three
    elements repeat p, g and the state of elements 0..2: after one step the three elements of the
    scalar tail carry the same BITS as elements 0..2 of the float4 body in every output (p and each
    state array ``keys`` of ``st``) -- with gmul 1 and 0.5, zero_g off and on, t0 = 0 and 3.
    ``launch``: the context's step method."""
    n = 4 * 256 + 3
    vals = dict((k, np.array(st[k][:n])) for k in ['p', 'g'] + list(keys))
    for v in vals.values():
        v[-3:] = v[:3]
    so, sr = torch.tensor([0, n], device="cuda"), dev([2.5])
    for gmul in (1.0, 0.5):
        for zero_g in (False, True):
            for t0 in (0, 3):
                what = (gmul, zero_g, t0)
                P, G = dev(vals['p']), dev(vals['g'])
                S = [dev(vals[k]) for k in keys]
                launch(P, G, *S, so, sr, hyper_dev(H.HYPERS[0], t0), gmul=gmul, zero_g=zero_g)
                torch.cuda.synchronize()
                assert not same_bits(P[:3], dev(vals['p'][:3])), what          # the step ran
                for out in [P] + S:
                    assert same_bits(out[-3:], out[:3]), what
                assert (not G.any()) if zero_g else same_bits(G, dev(vals['g'])), what


@pytest.mark.parametrize("kernel", ["adam", "sgd"])
def test_the_scalar_tail_runs_the_rule_of_the_vector_body(ctx, kernel):
    st = H.draw_state(np.random.RandomState(35), 4 * 256 + 3)
    check_tail_repeats_the_vector_body(getattr(ctx, kernel + '_step'), st, dict(adam='ms', sgd='d')[kernel])


# ---- B. steps in a row, eager and replayed -----------------------------------------------------------
def _chain_case(seed, t0):
    n = H.length('wrap', 3, cus())
    off, reg = H.segment_table(3, n)
    st = H.draw_state(np.random.RandomState(seed), n)
    return n, off, reg, H.per_element(off, reg), st, dict(H.HYPERS[0]), t0


def _fresh_gradient(n, seed):
    return H.draw_state(np.random.RandomState(seed), n)['g']


def test_three_steps_in_a_row_with_a_new_lr_before_the_third(ctx):
    """t advances with every launch and the lr of the moment is used; each step is checked from the
    device's own state before it"""
    n, off, reg, mult, st, h, t0 = _chain_case(31, 9)
    so, sr = torch.tensor(off, device="cuda"), dev(reg)
    P, M, S, D, Ps = dev(st['p']), dev(st['m']), dev(st['s']), dev(st['d']), dev(st['p'])
    hyp = hyper_dev(h, t0)
    for step in range(3):
        if step == 2:
            h['lr'] = H.f32(0.02)
            hyp[0] = h['lr']
        g = _fresh_gradient(n, 40 + step)
        G, Gs = dev(g), dev(g)
        prev = dict(p=host(P), m=host(M), s=host(S), ps=host(Ps), d=host(D))
        ctx.adam_step(P, G, M, S, so, sr, hyp, zero_g=bool(step & 1))
        ctx.sgd_step(Ps, Gs, D, so, sr, hyp, zero_g=bool(step & 1))
        torch.cuda.synchronize()
        fac = check_counter_and_factor(hyp, h, t0 + step, step)
        ref, terms = H.adam_ref(prev['p'], g, prev['m'], prev['s'], mult, h, fac)
        note('adam', H.accept(dict(p=host(P), m=host(M), s=host(S)), ref, terms, ('adam', step)))
        ref, terms = H.sgd_ref(prev['ps'], g, prev['d'], mult, h)
        note('sgd', H.accept(dict(p=host(Ps), d=host(D)), ref, terms, ('sgd', step)))
        assert bool(G.any()) != bool(step & 1) and bool(Gs.any()) != bool(step & 1)
    assert float(hyp[4]) == t0 + 3


@pytest.mark.parametrize("kernel", ["adam", "sgd"])
def test_a_captured_step_replayed_three_times(ctx, kernel):
    """one launch captured with the context's graph calls (as test_graph_capture_replay) and replayed:
    every replay is one more step -- t read from and published to the device -- from the state the
    replay before it left"""
    n, off, reg, mult, st, h, t0 = _chain_case(32, 1)
    so, sr = torch.tensor(off, device="cuda"), dev(reg)
    P, G, M, S, D = (dev(st[k]) for k in 'pgmsd')
    hyp = hyper_dev(h, t0)
    side = torch.cuda.Stream()
    old = ctx.stream
    torch.cuda.synchronize()
    ctx.set_stream(side)
    try:
        ctx.graph_begin()
        if kernel == 'adam':
            ctx.adam_step(P, G, M, S, so, sr, hyp)
        else:
            ctx.sgd_step(P, G, D, so, sr, hyp)
        graph = ctx.graph_end()
        assert same_bits(P, dev(st['p'])) and float(hyp[4]) == t0            # captured, not run
        for replay in range(3):
            prev = dict(p=host(P), m=host(M), s=host(S), d=host(D))
            torch.cuda.synchronize()
            ctx.graph_launch(graph)
            ctx.synchronize()
            if kernel == 'adam':
                fac = check_counter_and_factor(hyp, h, t0 + replay, replay)
                ref, terms = H.adam_ref(prev['p'], st['g'], prev['m'], prev['s'], mult, h, fac)
                note('adam', H.accept(dict(p=host(P), m=host(M), s=host(S)), ref, terms, replay))
            else:
                ref, terms = H.sgd_ref(prev['p'], st['g'], prev['d'], mult, h)
                note('sgd', H.accept(dict(p=host(P), d=host(D)), ref, terms, replay))
                assert float(hyp[4]) == t0
            assert same_bits(G, dev(st['g']))
        ctx.graph_destroy(graph)
    finally:
        ctx.set_stream(old)


# ---- C. the update that also writes the packed images -----------------------------------------------
def test_adam_pack_step_against_the_restatement(ctx):
    """p, m, s and t of e2_adam_pack_step (the images: test_adam_step_that_writes_the_packed_images):
    two conv tensors off the 32-channel tiles with a bias between them, multipliers 3, 0 and 1"""
    tensors = [("w1", (37, 21, 2, 2, 3), 3.0), ("b1", (37,), 0.0), ("w2", (40, 30, 1, 5, 5), 1.0)]
    offs, off = {}, 0
    for name, sh, _ in tensors:
        offs[name] = off
        off += (int(np.prod(sh)) + 3) // 4 * 4
    n = off
    used = np.zeros(n, bool)
    mult = np.zeros(n)
    for name, sh, reg in tensors:
        used[offs[name]:offs[name] + int(np.prod(sh))] = True
        mult[offs[name]:offs[name] + int(np.prod(sh))] = reg
    assert not used.all()                                          # (the bias is padded to 40)
    st = H.draw_state(np.random.RandomState(33), n)
    h, t0, gdiv = H.HYPERS[0], 9, 1234.0
    P, G, M, S = (dev(st[k]) for k in 'pgms')
    hyp = hyper_dev(h, t0, 24)
    # (images as in test_adam_step_that_writes_the_packed_images: w1 has the data-gradient image
    # only, w2 the forward image only)
    jobs = []
    for name, sh, reg in tensors:
        if len(sh) == 5:
            img = torch.zeros(ctx.conv_ws_bytes(sh[0], sh[1], sh[2:]) // 4 + 64, device="cuda")
            jobs.append((offs[name], None, img, sh, reg) if name == "w1" else (offs[name], img, None, sh, reg))
    upd = ctx.make_upd_jobs(jobs, [(offs["b1"], 37, 0.0)])
    ctx.adam_pack_step(P, G, M, S, upd, hyp, gdiv=dev([gdiv]), gmul=1.0, zero_g=True)
    torch.cuda.synchronize()
    fac = check_counter_and_factor(hyp, h, t0, 'pack')
    assert not hyp.view(torch.int32)[8:].any()                     # the sub-counters too
    ref, terms = H.adam_ref(st['p'], st['g'], st['m'], st['s'], mult, h, fac, H.grad_scale(gdiv, 1.0))
    got = dict(p=host(P), m=host(M), s=host(S))
    pick = lambda d: dict((k, v[used]) for k, v in d.items())
    r = H.accept(pick(got), pick(ref), pick(terms), 'pack')
    print("adam_pack_step:", r)
    note('adam_pack', r)
    for k in 'pms':                                                # the padding belongs to nobody
        assert np.array_equal(got[k][~used].view(np.int32), st[k][~used].view(np.int32)), k
    assert not G[torch.tensor(used, device="cuda")].any()
    for _, wf, wd_, _, _ in jobs:
        assert (wd_ if wf is None else wf).any()


# ---- D. refusals, before any launch ---------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(ctx):
    from elektronn2_amd import backend
    n = 4 * 1025 + 8
    vals = np.random.RandomState(34).randn(5, n + 4).astype(np.float32)
    store = [dev(v) for v in vals]
    P, G, M, S, D = (t[:n] for t in store)
    hyp = hyper_dev(H.HYPERS[0], 5, 24)
    hyp0 = hyp.clone()
    off, reg = H.segment_table(1025, n)
    so, sr = torch.tensor(off, device="cuda"), dev(reg)
    with pytest.raises(backend.E2Error, match="1025 parameter tensors"):
        ctx.adam_step(P, G, M, S, so, sr, hyp)
    with pytest.raises(backend.E2Error, match="1025 parameter tensors"):
        ctx.sgd_step(P, G, D, so, sr, hyp)
    # an arena view 4 bytes off its 16-byte boundary, in each position
    off, reg = H.segment_table(3, n)
    so, sr = torch.tensor(off, device="cuda"), dev(reg)
    assert P.data_ptr() % 16 == 0
    for bad in range(4):
        a = [t[1:n + 1] if i == bad else t[:n] for i, t in enumerate(store[:4])]
        assert a[bad].data_ptr() % 16 == 4
        with pytest.raises(backend.E2Error, match="16-byte aligned"):
            ctx.adam_step(a[0], a[1], a[2], a[3], so, sr, hyp)
    for bad in range(3):
        a = [t[1:n + 1] if i == bad else t[:n] for i, t in enumerate((store[0], store[1], store[4]))]
        with pytest.raises(backend.E2Error, match="16-byte aligned"):
            ctx.sgd_step(a[0], a[1], a[2], so, sr, hyp)
    # 97 conv tensors for the pack step
    img = torch.zeros(ctx.conv_ws_bytes(4, 4, (1, 1, 1)) // 4 + 64, device="cuda")
    upd = ctx.make_upd_jobs([(16 * k, img, None, (4, 4, 1, 1, 1), 1.0) for k in range(97)], [])
    with pytest.raises(backend.E2Error, match="97 conv tensors"):
        ctx.adam_pack_step(P, G, M, S, upd, hyp)
    torch.cuda.synchronize()
    for t, v in zip(store, vals):
        assert same_bits(t, dev(v))
    assert same_bits(hyp, hyp0) and not img.any()


# ---- E. a smallest net, teacher-forced on its own gradients -------------------------------------------
def _flat_state(model, params, flat):
    out = {}
    for name, p in params.items():
        o, cnt, sh = model._slots[id(p)]
        out[name] = np.zeros(sh, np.float32) if flat is None else np.asarray(flat[o:o + cnt]).reshape(sh)
    return out


def _noise_slack(out, g, h, delta):
    """what a gradient that is off by ``delta`` (absolute) moves the state outputs by"""
    if out == 'm':
        return (1.0 - h['mom']) * delta
    if out == 's':
        return (1.0 - h['b2']) * (2.0 * np.abs(g) * delta + delta * delta)
    if out == 'd':
        return delta
    return 0.0


@pytest.mark.parametrize("gradients", ["of_the_step", "evaluated_before"])
@pytest.mark.parametrize("adam_pack", [False, True], ids=["two_launches", "adam_pack"])
@pytest.mark.parametrize("fractional", [False, True], ids=["as_built", "apply_reg_0.5"])
def test_smallest_net_steps_tensor_by_tensor(fractional, adam_pack, gradients):
    """one SGD step, one Adam step and a second Adam step (lr 0.05, wd 0.5): every trainable tensor
    and the optimiser state against the restatement applied tensor by tensor at the parameters
    before the step, with the multipliers of variables.reg_multiplier -- 1 (w), 0 (b), 3 (gamma), and 1
    for the weight registered with apply_reg = 0.5 (its own value before the helper: p then misses
    by 6e-3 of its terms).

    ``of_the_step``: plan option zero_in_update off, so the gradient arena still holds what the
    update consumed; the reference takes exactly that and the op rule holds with no addend.

    ``evaluated_before``: the plan as shipped (the update clears the arena); the gradients come
    from model.gradients() before the step.  Two evaluations differ by the float32 atomics of the
    weight / bias sums, which the project bounds by 2e-6 OF THE TENSOR'S LARGEST ELEMENT
    (tests/test_bf16_gpu.py, measured <= 2.4e-7; here 1.2 .. 2.2e-7).  p is held to the op rule with
    TOL + 2e-6 (worst seen 1.2e-7).  m, s and d are linear / quadratic in one element's gradient
    alone, so noise of that size is 2e-6 of an element's terms only where the element is the
    largest: measured 0.5 .. 6.8e-6 of the terms on c0_w from run to run, all of it the gradient's
    own difference.  They get the noise in its own units instead: TOL_SUMMED of the terms plus what
    delta = 2e-6 max|g| moves them by."""
    from elektronn2_amd.neuromancer import plan_options
    from elektronn2_amd.neuromancer.variables import reg_multiplier
    h = dict(H.NET_HYPER, b2=H.NET_B2)
    exact = gradients == "of_the_step"
    with plan_options(adam_pack=adam_pack, zero_in_update=not exact):
        m = H.smallest_net(fractional)
        x, t = H.net_batch()
        params = m.loss_node.all_trainable_params
        names = list(params)
        mults = dict((k, reg_multiplier(p)) for k, p in params.items())
        assert mults['head_w'] == 1.0 and sorted(set(mults.values())) == [0.0, 1.0, 3.0]
        for step, name in enumerate(('SGD', 'Adam', 'Adam')):
            opt = m.optimisers[name]
            before = dict((k, p.get_value()) for k, p in params.items())
            if not exact:
                grads = dict(zip(names, m.gradients(x, t)))
            sd = opt.state_dict()
            t_before = opt.t if name == 'Adam' else None
            m.trainingstep(x, t, optimiser=name)
            assert opt.step.func._upd_zeroes_g() == (not exact)
            if exact:
                grads = dict((k, host(m.device_grad(p))) for k, p in params.items())
            else:
                assert not m.G.any()
            after = dict((k, p.get_value()) for k, p in params.items())
            sd2 = opt.state_dict()
            if name == 'Adam':
                assert opt.t == t_before + 1 == max(step, 1) and float(sd2['t']) == opt.t
                fac = float(opt._hyper[5])
                want = H.bias_factor(opt.t, h['mom'], h['b2'])
                assert abs(fac - want) / want <= H.fac_bound(opt.t, h['mom'], h['b2'])
                assert int(opt._hyper.view(torch.int32)[7]) == 0
                old = dict(m=_flat_state(m, params, sd.get('m')), s=_flat_state(m, params, sd.get('s')))
                new = dict(m=_flat_state(m, params, sd2['m']), s=_flat_state(m, params, sd2['s']))
            else:
                old = dict(d=_flat_state(m, params, sd.get('last_dir')))
                new = dict(d=_flat_state(m, params, sd2['last_dir']))
            worst, excess = {}, {}
            for k in names:
                mult = np.full(before[k].shape, mults[k])
                g = np.asarray(grads[k], np.float64).reshape(before[k].shape)
                assert np.abs(g).max() > 0 and not np.array_equal(after[k], before[k]), k
                if name == 'Adam':
                    ref, terms = H.adam_ref(before[k], g, old['m'][k], old['s'][k], mult, h, fac)
                else:
                    ref, terms = H.sgd_ref(before[k], g, old['d'][k], mult, h)
                got = dict((o, new[o][k]) for o in new)
                got['p'] = after[k]
                for o, v in H.ratios(got, ref, terms).items():
                    worst[o] = max(worst.get(o, (0.0, '')), (v, k))
                for o in terms:
                    delta = 0.0 if exact else GRAD_NOISE * np.abs(g).max()
                    extra = GRAD_NOISE if (o.startswith('p') and not exact) else 0.0
                    allowed = H.tolerance(o, extra) * terms[o] + _noise_slack(o, g, h, delta)
                    diff = np.abs(np.asarray(got[o.split('_')[0]], np.float64) - ref[o.split('_')[0]])
                    assert (diff[allowed == 0] == 0).all(), (name, step, o, k)
                    e = float((diff[allowed > 0] / allowed[allowed > 0]).max())
                    excess[o] = max(excess.get(o, (0.0, '')), (e, k))
            print("%s step %d (adam_pack %s, _upd %s, gradients %s): worst ratio to the terms %s; of what is allowed %s"
                  % (name, step, adam_pack, getattr(opt.step.func, '_upd', None) is not None, gradients, worst, excess))
            note('net_%s_%s' % (name.lower(), gradients), dict((o, v) for o, (v, _) in worst.items()))
            for o, (e, k) in excess.items():
                assert e <= 1.0, (name, step, o, k, e, worst[o])
