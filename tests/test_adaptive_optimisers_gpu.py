"""AdaGrad / AdaDelta updates on the GPU (csrc/arena_ops.hip: e2_adagrad_step_ex,
e2_adadelta_step_ex) against the float64 restatements of tests/test_adaptive_optimisers_host.py --
never the code under test -- on its case table, under its rule and tolerances: every output
(p, h / p, s, d), the step counter and the arrival counter, the gradient arena, the elements
without any gradient, NaN guards around every arena; three steps in a row with a changed lr; a
captured step replayed; the refusals; the smallest net of tests/test_optimiser_host.py stepped
twice with each optimiser and checked tensor by tensor; several steps per graph launch; a
checkpoint in mid-run; bf16 mode."""
import numpy as np
import pytest
import torch

import test_optimiser_host as H
import test_adaptive_optimisers_host as A
from test_optimiser_host import CASES, CASE_IDS
from test_optimiser_gpu import GRAD_NOISE, dev, host, same_bits, cus, hyper_dev, upload, check_gradient_arena, _flat_state, \
    check_tail_repeats_the_vector_body

pytestmark = pytest.mark.gpu

GUARD = 64                                   # floats of NaN on either side of an arena
WORST = {}


def note(kind, r):
    for k, v in r.items():
        WORST[kind, k] = max(WORST.get((kind, k), 0.0), v)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst ratio per output (tolerances: %s): %s"
          % (", ".join("%s %s %.3e" % (a, b, v) for (a, b), v in sorted(A.TOLS.items())),
             ", ".join("%s %s %.3e" % (a, b, v) for (a, b), v in sorted(WORST.items()))))


def guarded(values):
    """-> (store, view): the values on a 16-byte boundary between two runs of NaN"""
    v = np.asarray(values, np.float32)
    store = torch.full((v.size + 2 * GUARD,), float('nan'), device="cuda")
    view = store[GUARD:GUARD + v.size]
    view.copy_(dev(v))
    assert view.data_ptr() % 16 == 0
    return store, view


def guards_intact(store, n):
    nan = torch.full((GUARD,), float('nan'), device="cuda")
    return same_bits(store[:GUARD], nan) and same_bits(store[GUARD + n:], nan)


def check_counter(hyp, h, t0, what):
    """t = t0 + 1, the arrival counter back at integer 0, everything else as it was"""
    hv = host(hyp)
    assert hv[4] == t0 + 1, (what, hv[4])
    assert int(hyp.view(torch.int32)[7]) == 0, what
    assert np.array_equal(hv[:4], np.array([h['lr'], h['mom'], h['b2'], h['wd']], np.float32)), what
    assert not hv[5:7].any(), what


# ---- A. the two sweeps over the case table -----------------------------------------------------------
def test_the_case_table_holds_what_the_kernels_can_get_wrong():
    cols = list(zip(*CASES))
    assert {'4', '7', '1028', 'wrap'} <= set(cols[1]) and {1, 1024} <= set(cols[0])
    assert {0, 999} <= set(cols[2]) and set(cols[4]) == set(range(len(H.GSCALES))) and set(cols[5]) == {0, 1}
    assert H.length('wrap', 1, cus()) // 4 > 2 * cus() * 256           # beyond one sweep of either grid


@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_adagrad_step_against_the_restatement(ctx, idx):
    c = A.case(idx, cus())
    _, so, sr, gdiv = upload(c, '')
    (Ps, P), (Gs, G), (Hs, Hh) = (guarded(c[k]) for k in ('p', 'g', 'hs'))
    hyp = hyper_dev(c['h'], c['t0'])
    ctx.adagrad_step(P, G, Hh, so, sr, hyp, gdiv=gdiv, gmul=c['gmul'], zero_g=c['zero_g'])
    torch.cuda.synchronize()
    check_counter(hyp, c['h'], c['t0'], CASE_IDS[idx])
    ref, terms = A.adagrad_expected(c)
    got = dict(p=host(P), h=host(Hh))
    r = H.ratios(got, ref, terms)
    print(CASE_IDS[idx], "n = %d:" % c['n'], ", ".join("%s %.2e" % kv for kv in r.items()))
    note('adagrad', r)
    A.accept('adagrad', got, ref, terms, CASE_IDS[idx])
    check_gradient_arena(G, c, CASE_IDS[idx])
    dead = ref['h'] == 0                                            # no gradient since the start
    assert dead[1] and not dead[2]
    for k, a in (('p', got['p']), ('hs', got['h'])):
        assert np.array_equal(a[dead].view(np.int32), c[k][dead].view(np.int32)), k
    for store in (Ps, Gs, Hs):
        assert guards_intact(store, c['n'])
    assert torch.equal(so, torch.tensor(c['seg_off'], device="cuda")) and same_bits(sr, dev(c['seg_reg']))


@pytest.mark.parametrize("idx", range(len(CASES)), ids=CASE_IDS)
def test_adadelta_step_against_the_restatement(ctx, idx):
    c = A.case(idx, cus())
    _, so, sr, gdiv = upload(c, '')
    (Ps, P), (Gs, G), (Ss, S), (Ds, D) = (guarded(c[k]) for k in 'pgsd')
    hyp = hyper_dev(c['h'], c['t0'])
    before = hyp.clone()
    ctx.adadelta_step(P, G, S, D, so, sr, hyp, gdiv=gdiv, gmul=c['gmul'], zero_g=c['zero_g'])
    torch.cuda.synchronize()
    assert same_bits(hyp, before)                                  # AdaDelta keeps no counter
    ref, terms = A.adadelta_expected(c)
    got = dict(p=host(P), s=host(S), d=host(D))
    r = H.ratios(got, ref, terms)
    print(CASE_IDS[idx], "n = %d:" % c['n'], ", ".join("%s %.2e" % kv for kv in r.items()))
    note('adadelta', r)
    A.accept('adadelta', got, ref, terms, CASE_IDS[idx])
    check_gradient_arena(G, c, CASE_IDS[idx])
    for store in (Ps, Gs, Ss, Ds):
        assert guards_intact(store, c['n'])


@pytest.mark.parametrize("kernel", ["adagrad", "adadelta"])
def test_the_scalar_tail_runs_the_rule_of_the_vector_body(ctx, kernel):
    """tests/test_optimiser_gpu.py check_tail_repeats_the_vector_body; element 1 has no gradient on
    h = 0 (AdaGrad leaves it as it is), element 2 none on h > 0"""
    st = A.draw_state(np.random.RandomState(55), 4 * 256 + 3, 1.0)
    check_tail_repeats_the_vector_body(getattr(ctx, kernel + '_step'), st,
                                       dict(adagrad=['hs'], adadelta=['s', 'd'])[kernel])


# ---- B. steps in a row, eager and replayed -----------------------------------------------------------
def _chain_case(seed):
    n = H.length('wrap', 3, cus())
    off, reg = A.segment_table(3, n)
    st = A.draw_state(np.random.RandomState(seed), n, 1.0)
    return n, off, reg, H.per_element(off, reg), st, dict(H.HYPERS[0])


def test_three_steps_in_a_row_with_a_new_lr_before_the_third(ctx):
    """from t = 0: the first step doubles, the others do not; t advances with every launch and the
    lr of the moment is used; each step is checked from the device's own state before it"""
    n, off, reg, mult, st, h = _chain_case(51)
    so, sr = torch.tensor(off, device="cuda"), dev(reg)
    P, Hh, Pd, S, D = dev(st['p']), dev(st['hs']), dev(st['p']), dev(st['s']), dev(st['d'])
    hyp = hyper_dev(h, 0)
    for step in range(3):
        if step == 2:
            h['lr'] = H.f32(0.02)
            hyp[0] = h['lr']
        g = A.draw_gradient(np.random.RandomState(60 + step), n, 1.0)
        G, Gd = dev(g), dev(g)
        prev = dict(p=host(P), h=host(Hh), pd=host(Pd), s=host(S), d=host(D))
        ctx.adagrad_step(P, G, Hh, so, sr, hyp, zero_g=bool(step & 1))
        ctx.adadelta_step(Pd, Gd, S, D, so, sr, hyp, zero_g=bool(step & 1))
        torch.cuda.synchronize()
        check_counter(hyp, h, step, step)
        ref, terms = A.adagrad_ref(prev['p'], g, prev['h'], mult, h, step)
        note('adagrad', A.accept('adagrad', dict(p=host(P), h=host(Hh)), ref, terms, step))
        ref, terms = A.adadelta_ref(prev['pd'], g, prev['s'], prev['d'], mult, h)
        note('adadelta', A.accept('adadelta', dict(p=host(Pd), s=host(S), d=host(D)), ref, terms, step))
        assert bool(G.any()) != bool(step & 1) and bool(Gd.any()) != bool(step & 1)
    assert float(hyp[4]) == 3


@pytest.mark.parametrize("kernel", ["adagrad", "adadelta"])
def test_a_captured_step_replayed_three_times(ctx, kernel):
    """one launch captured from t = 0 and replayed: every replay is one more step from the state the
    replay before it left -- the counter is read from and published to the device, so the doubling
    happens at the first replay and never again"""
    n, off, reg, mult, st, h = _chain_case(52)
    so, sr = torch.tensor(off, device="cuda"), dev(reg)
    P, G, Hh, S, D = (dev(st[k]) for k in ('p', 'g', 'hs', 's', 'd'))
    hyp = hyper_dev(h, 0)
    side = torch.cuda.Stream()
    old = ctx.stream
    torch.cuda.synchronize()
    ctx.set_stream(side)
    try:
        ctx.graph_begin()
        if kernel == 'adagrad':
            ctx.adagrad_step(P, G, Hh, so, sr, hyp)
        else:
            ctx.adadelta_step(P, G, S, D, so, sr, hyp)
        graph = ctx.graph_end()
        assert same_bits(P, dev(st['p'])) and float(hyp[4]) == 0                # captured, not run
        for replay in range(3):
            prev = dict(p=host(P), h=host(Hh), s=host(S), d=host(D))
            torch.cuda.synchronize()
            ctx.graph_launch(graph)
            ctx.synchronize()
            if kernel == 'adagrad':
                check_counter(hyp, h, replay, replay)
                ref, terms = A.adagrad_ref(prev['p'], st['g'], prev['h'], mult, h, replay)
                note('adagrad', A.accept('adagrad', dict(p=host(P), h=host(Hh)), ref, terms, replay))
            else:
                ref, terms = A.adadelta_ref(prev['p'], st['g'], prev['s'], prev['d'], mult, h)
                note('adadelta', A.accept('adadelta', dict(p=host(P), s=host(S), d=host(D)), ref, terms, replay))
                assert float(hyp[4]) == 0
            assert same_bits(G, dev(st['g']))
        ctx.graph_destroy(graph)
    finally:
        ctx.set_stream(old)


# ---- C. refusals, before any launch ---------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(ctx):
    from elektronn2_amd import backend
    n = 4 * 1025 + 8
    vals = np.random.RandomState(54).rand(4, n + 4).astype(np.float32)
    store = [dev(v) for v in vals]
    P, G, S, D = (t[:n] for t in store)
    hyp = hyper_dev(H.HYPERS[0], 0)
    hyp0 = hyp.clone()
    off, reg = A.segment_table(1025, n)
    so, sr = torch.tensor(off, device="cuda"), dev(reg)
    with pytest.raises(backend.E2Error, match="1025 parameter tensors"):
        ctx.adagrad_step(P, G, S, so, sr, hyp)
    with pytest.raises(backend.E2Error, match="1025 parameter tensors"):
        ctx.adadelta_step(P, G, S, D, so, sr, hyp)
    off, reg = A.segment_table(3, n)
    so, sr = torch.tensor(off, device="cuda"), dev(reg)
    with pytest.raises(backend.E2Error, match="null argument"):     # no segment at all
        ctx.adagrad_step(P, G, S, so, sr[:0], hyp)
    with pytest.raises(backend.E2Error, match="null argument"):
        ctx.adadelta_step(P, G, S, D, so, sr[:0], hyp)
    with pytest.raises(backend.E2Error, match="null argument"):
        ctx.adagrad_step(P, G, S, so, sr, None)
    with pytest.raises(backend.E2Error, match="null argument"):
        ctx.adadelta_step(P, G, S, D, so, sr, None)
    # an arena view 4 bytes off its 16-byte boundary, in each position
    assert P.data_ptr() % 16 == 0
    for bad in range(3):
        a = [t[1:n + 1] if i == bad else t[:n] for i, t in enumerate(store[:3])]
        assert a[bad].data_ptr() % 16 == 4
        with pytest.raises(backend.E2Error, match="16-byte aligned"):
            ctx.adagrad_step(a[0], a[1], a[2], so, sr, hyp)
    for bad in range(4):
        a = [t[1:n + 1] if i == bad else t[:n] for i, t in enumerate(store)]
        with pytest.raises(backend.E2Error, match="16-byte aligned"):
            ctx.adadelta_step(a[0], a[1], a[2], a[3], so, sr, hyp)
    torch.cuda.synchronize()
    for t, v in zip(store, vals):
        assert same_bits(t, dev(v))
    assert same_bits(hyp, hyp0)


# ---- D. the smallest net, teacher-forced on its own gradients ------------------------------------------
def _noise_slack(name, out, before, g, old, mult, h, t0, delta):
    """what a gradient that is off by up to ``delta`` (absolute) can move an output by.
    AdaGrad: h' = h + c g^2 moves by c (2 |g| delta + delta^2); p' = p - lr (g + w) / sqrt(h + c g^2)
    with w = wd r p has the derivative -lr (h - c g w) / (h + c g^2)^(3/2) in g, bounded over
    [g - delta, g + delta] by its largest numerator over its smallest denominator (no bound where that
    is 0: a gradient that noise can carry through 0 on h = 0).  AdaDelta: dir = g K with
    K = sqrt(d + eps) / sqrt(s + eps) of the old state, so p' moves by lr K delta, s' by
    (1 - mom) (2 |g| delta + delta^2) and d' by K^2 times that."""
    if delta == 0.0:
        return 0.0
    g = np.abs(g)
    sq = 2.0 * g * delta + delta * delta
    if name == 'AdaGrad':
        c = 2.0 if t0 == 0 else 1.0
        if out == 'h':
            return c * sq
        w = np.abs(h['wd'] * (mult != 0) * before)
        den = (old['h'] + c * np.maximum(g - delta, 0.0) ** 2) ** 1.5
        num = delta * h['lr'] * (old['h'] + c * (g + delta) * w)
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.inf)
    K = np.sqrt(old['d'] + A.EPS) / np.sqrt(old['s'] + A.EPS)
    return dict(p=h['lr'] * K * delta, s=(1.0 - h['mom']) * sq, d=(1.0 - h['mom']) * K * K * sq)[out]


@pytest.mark.parametrize("gradients", ["of_the_step", "evaluated_before"])
@pytest.mark.parametrize("fractional", [False, True], ids=["as_built", "apply_reg_0.5"])
@pytest.mark.parametrize("name", ["AdaGrad", "AdaDelta"])
def test_smallest_net_steps_tensor_by_tensor(name, fractional, gradients):
    """two steps of one optimiser (lr 0.05, mom 0.9, wd 0.5): every trainable tensor and the
    optimiser state against the restatement applied tensor by tensor at the parameters before the
    step, with the multipliers of variables.reg_multiplier -- 1 (w), 0 (b), 3 (gamma), which AdaGrad
    takes as 1, 0, 1.  The method of tests/test_optimiser_gpu.py:

    ``of_the_step``: plan option zero_in_update off, so the gradient arena still holds what the
    update consumed; the reference takes exactly that and the op rule holds with no addend.

    ``evaluated_before``: the plan as shipped (the update clears the arena, which is checked); the
    gradients come from model.gradients() before the step and differ from the step's own by the
    float32 atomics of the weight / bias sums, bounded by 2e-6 of the tensor's largest element
    (tests/test_bf16_gpu.py): each output gets its tolerance of the terms plus what
    delta = 2e-6 max|g| can move it by (_noise_slack).

    The SECOND step is the one that shows a missing update launch, packed weight images that were
    not marked stale, or a gradient arena that was not cleared: its loss must be the loss at the
    parameters the first step left (a fresh evaluation by the loss plan), not the first loss again,
    and its tensors are checked like the first step's.  Batch norm's running statistics move with
    every step."""
    from elektronn2_amd.neuromancer import plan_options
    from elektronn2_amd.neuromancer.variables import reg_multiplier
    h = dict(H.NET_HYPER)
    exact = gradients == "of_the_step"
    key = 'adagrad' if name == 'AdaGrad' else 'adadelta'
    with plan_options(zero_in_update=not exact):
        m = H.smallest_net(fractional)
        m.set_opt_meta_params(name, H.NET_HYPER)
        x, t = H.net_batch()
        params = m.loss_node.all_trainable_params
        names = list(params)
        mults = dict((k, reg_multiplier(p)) for k, p in params.items())
        assert mults['head_w'] == 1.0 and sorted(set(mults.values())) == [0.0, 1.0, 3.0]
        opt = m.optimisers[name]
        losses = []
        for step in range(2):
            before = dict((k, p.get_value()) for k, p in params.items())
            stats = (m.nodes['c0'].mean.get_value(), m.nodes['c0'].std.get_value())
            loss_here = float(m.loss(x, t))
            if not exact:
                grads = dict(zip(names, m.gradients(x, t)))
            sd = opt.state_dict()
            assert (sd == {}) == (step == 0)
            loss, _, _ = m.trainingstep(x, t, optimiser=name)
            losses.append(float(loss))
            assert abs(losses[-1] - loss_here) <= 1e-5 * abs(loss_here), (step, losses, loss_here)
            assert opt.step.func._upd_zeroes_g() == (not exact)
            if exact:
                grads = dict((k, host(m.device_grad(p))) for k, p in params.items())
            else:
                assert not m.G.any()
            after = dict((k, p.get_value()) for k, p in params.items())
            sd2 = opt.state_dict()
            assert not np.array_equal(m.nodes['c0'].mean.get_value(), stats[0])
            assert not np.array_equal(m.nodes['c0'].std.get_value(), stats[1])
            if name == 'AdaGrad':
                assert opt.t == step + 1 == float(sd2['t']) and int(opt._hyper.view(torch.int32)[7]) == 0
                old = dict(h=_flat_state(m, params, sd.get('h')))
                new = dict(h=_flat_state(m, params, sd2['h']))
            else:
                old = dict(s=_flat_state(m, params, sd.get('s')), d=_flat_state(m, params, sd.get('d')))
                new = dict(s=_flat_state(m, params, sd2['s']), d=_flat_state(m, params, sd2['d']))
            worst, excess = {}, {}
            for k in names:
                mult = np.full(before[k].shape, mults[k])
                g = np.asarray(grads[k], np.float64).reshape(before[k].shape)
                assert np.abs(g).max() > 0 and not np.array_equal(after[k], before[k]), k
                o64 = dict((o, np.asarray(v[k], np.float64)) for o, v in old.items())
                if name == 'AdaGrad':
                    ref, terms = A.adagrad_ref(before[k], g, o64['h'], mult, h, step)
                else:
                    ref, terms = A.adadelta_ref(before[k], g, o64['s'], o64['d'], mult, h)
                got = dict((o, new[o][k]) for o in new)
                got['p'] = after[k]
                for o, v in H.ratios(got, ref, terms).items():
                    worst[o] = max(worst.get(o, (0.0, '')), (v, k))
                delta = 0.0 if exact else GRAD_NOISE * np.abs(g).max()
                for o in terms:
                    allowed = A.tolerance(key, o) * terms[o] + _noise_slack(name, o, np.asarray(before[k], np.float64),
                                                                            g, o64, mult, h, step, delta)
                    diff = np.abs(np.asarray(got[o], np.float64) - ref[o])
                    assert (diff[allowed == 0] == 0).all(), (name, step, o, k)
                    e = float((diff[allowed > 0] / allowed[allowed > 0]).max())
                    excess[o] = max(excess.get(o, (0.0, '')), (e, k))
            print("%s step %d (gradients %s): loss %.6f, worst ratio to the terms %s; of what is allowed %s"
                  % (name, step, gradients, losses[-1], worst, excess))
            note('net_%s_%s' % (key, gradients), dict((o, v) for o, (v, _) in worst.items()))
            for o, (e, k) in excess.items():
                assert e <= 1.0, (name, step, o, k, e, worst[o])
        # the loss moves by far more than two evaluations of one loss differ by
        assert abs(losses[1] - losses[0]) > 1e-3 * abs(losses[0]), losses


# ---- E. several steps per launch, a checkpoint in mid-run, bf16 mode -----------------------------------
def _lite(seed, name, sp=(7, 47, 47)):
    from oracle import e2_oracle as O
    from elektronn2_amd import nets, neuromancer as nm
    nm.model_manager.reset()
    m = nets.neuro3d_lite((None, 1) + sp, params=O.init_net(O.NEURO3D_LITE, 1, seed=seed))
    m.set_opt_meta_params(name, dict(lr=dict(AdaGrad=5e-4, AdaDelta=1e-3)[name], mom=0.9, wd=0.5e-4))
    return m


def _batches(n, sp=(7, 47, 47), seed=8):
    from oracle import e2_oracle as O
    rng = np.random.RandomState(seed)
    osp = O.net_out_shape(O.NEURO3D_LITE, sp)
    return ([rng.rand(1, 1, *sp).astype(np.float32) for _ in range(n)],
            [rng.randint(0, 2, (1, 1) + osp).astype(np.float32) for _ in range(n)])


def _values(m):
    return [p.get_value() for p in m.loss_node.all_trainable_params.values()]


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def test_several_adadelta_steps_in_one_graph_launch():
    """trainingstep + trainingsteps(3) + trainingsteps(3) over a ring of four batches (the first
    launch still contains the single step's capture, the second is one graph of three steps) against
    seven single steps: the same losses step by step (1e-5) and the same parameters (1e-4), the
    bounds of tests/test_model_gpu.py::test_several_steps_in_one_graph_launch"""
    xs, ts = _batches(4)
    a = _lite(3, 'AdaDelta')
    la = [float(a.trainingstep(xs[i % 4], ts[i % 4], optimiser='AdaDelta')[0]) for i in range(7)]
    b = _lite(3, 'AdaDelta')
    start = _values(b)
    lb = [float(b.trainingstep(xs[0], ts[0], optimiser='AdaDelta')[0])]
    plan = b.optimisers['AdaDelta'].step.func
    ring = torch.zeros(4, plan.input_arena.numel(), device=plan.ctx.device)
    for j in range(4):
        for node, src in zip(plan.inputs[:2], (xs[j], ts[j])):
            o, n = plan.input_slices[node]
            ring[j, o:o + n] = torch.tensor(src.ravel(), device=ring.device)
    plan.set_input_ring(ring)
    plan._step_state[0] += 1                     # the ring's next slot is the one of step 1
    l3, _ = b.trainingsteps(3, optimiser='AdaDelta', ring=ring)
    assert len(l3) == 3 and plan._multi, "no multi-step graph was captured"
    l3b, t3 = b.trainingsteps(3, optimiser='AdaDelta', ring=ring)
    assert len(l3b) == 3 and 3 in plan._multi and t3 > 0
    assert plan.ring_position() == 7 and b.iterations == 7
    lb += [float(v) for v in l3] + [float(v) for v in l3b]
    print("single steps %s, 1 + 3 + 3 %s" % (la, lb))
    for i, (u, v) in enumerate(zip(la, lb)):
        assert abs(u - v) < 1e-5 * abs(u), (i, la, lb)
    for u, v, w in zip(_values(a), _values(b), start):
        assert _rel(v, u) < 1e-4
        assert not np.array_equal(v, w)
    assert len(set(la)) == 7


def test_adagrad_resumes_from_a_checkpoint_without_doubling_again(tmp_path):
    """two steps, save, modelload into a fresh model, the third step -- against the third step of
    the uninterrupted run: loss 1e-5, parameters 1e-4; t goes on at 2 (a counter that restarted at 0
    would add the third gradient's square twice: h is compared as well)"""
    from elektronn2_amd.neuromancer.model import modelload
    xs, ts = _batches(3)
    a = _lite(1, 'AdaGrad')
    for i in range(2):
        a.trainingstep(xs[i], ts[i], optimiser='AdaGrad')
    f = str(tmp_path / "state.mdl")
    a.save(f)
    saved = a.optimisers['AdaGrad'].state_dict()
    assert float(saved['t']) == 2.0 and saved['h'].max() > 0
    want = float(a.trainingstep(xs[2], ts[2], optimiser='AdaGrad')[0])
    b = _lite(9, 'AdaGrad')                      # other weights, nothing on the device yet
    modelload(f, b)
    assert b.optimisers['AdaGrad'].t == 2.0 and b.iterations == 2
    assert np.array_equal(b.optimisers['AdaGrad'].state_dict()['h'], saved['h'])
    got = float(b.trainingstep(xs[2], ts[2], optimiser='AdaGrad')[0])
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    assert b.optimisers['AdaGrad'].t == 3.0 == a.optimisers['AdaGrad'].t
    for u, v in zip(_values(a), _values(b)):
        assert _rel(v, u) < 1e-4
    ha, hb = a.optimisers['AdaGrad'].state_dict()['h'], b.optimisers['AdaGrad'].state_dict()['h']
    assert _rel(hb, ha) < 1e-4
    # ... which a second doubling would miss by far
    assert _rel(saved['h'] + 2 * (ha - saved['h']), ha) > 1e-2


@pytest.fixture()
def process_bf16():
    import elektronn2_amd
    elektronn2_amd.set_mfma_dtype('bf16')
    yield
    elektronn2_amd.set_mfma_dtype('f32')


def test_two_adagrad_steps_in_bf16_mode(process_bf16):
    """bf16 mode keeps bf16 images of the weights that are rewritten after every update: two AdaGrad
    steps with the operands made ahead against two with the operands converted inside the kernels,
    which cannot go stale -- the method and bounds of tests/test_bf16_gpu.py::
    test_no_operand_goes_stale_across_optimiser_steps (first loss the same bits' worth, 1e-6;
    trajectory 2e-3), and a third loss that has seen the second update"""
    import test_bf16_gpu as B
    from elektronn2_amd import neuromancer as nm
    sp = (9, 71, 71)
    xs, ts = _batches(1, sp, seed=5)
    res = []
    for ahead in (False, True):
        with nm.plan_options(bf16_ahead=ahead, bf16_ahead_min=0.0):
            m = _lite(3, 'AdaGrad', sp)
            m.optimisers['AdaGrad'].step.compile()       # (plans snapshot the options when constructed)
        with B._pinned():
            losses = [float(m.trainingstep(xs[0], ts[0], optimiser='AdaGrad')[0]) for _ in range(3)]
        plan = m.optimisers['AdaGrad'].step.func
        res.append((losses, plan.model.P.detach().cpu().numpy().copy(), sorted(set(k for (_, k) in plan.bf16a))))
    (l0, p0, k0), (l1, p1, k1) = res
    print("bf16 mode, AdaGrad: converting %s, made ahead %s" % (l0, l1))
    assert k0 == [] and {'fwd', 'dgrad', 'wgrad'} <= set(k1), (k0, k1)
    assert np.isfinite(l1).all() and len(set(l1)) == 3
    assert abs(l1[0] - l0[0]) <= 1e-6 * abs(l0[0])
    np.testing.assert_allclose(l1, l0, rtol=2e-3)
    assert np.abs(p1 - p0).max() <= 2e-3 * np.abs(p0).max()
