"""Two nodes that share a parameter object, on the GPU: every route on which a launch adds to --
or overwrites -- the weight and bias gradient, against the float64 reference of
tests/shared_param_cases.py (one leaf per shared parameter: autograd sums the contributions, Adam
updates it once).  Bound: 1e-4 of the reference's largest magnitude (tests/test_model_gpu.py:17).
tests/test_shared_params_host.py shows on the reference alone that each single contribution is more
than 10x that bound away from the sum, so a dropped, overwritten or doubled one cannot pass.

Nets (shared_param_cases.NETS; node 'b' takes its parameters from node 'a'):
S1 two generic convs of different signatures, S2 of identical signatures, S3 two UpConvs, S4 the
fused first layer and a generic conv, S5 the tail's 1x1x1 conv and an earlier pointwise conv, S6 two
softmax heads of a multi-task net, S7 two Perceptrons, S8 two batch-normalised convs sharing gamma
and b, S9 a valid and a 'same' conv sharing w.  Every case asserts the route it names."""
import contextlib
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import shared_param_cases as S
from shared_param_cases import ADAM, NETS, N_STEPS, TOL

pytestmark = pytest.mark.gpu


def rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


class Figures(object):
    """every figure is printed before any is asserted"""

    def __init__(self, case, tol=TOL):
        self.case, self.tol, self.rows = case, tol, []

    def add(self, what, got, ref, tol=None):
        self.rows.append((what, rel(got, ref), self.tol if tol is None else tol))

    def check(self):
        for what, v, tol in self.rows:
            print("%s: %s %.3g (bound %.0e)" % (self.case, what, v, tol))
        bad = [(w, v) for w, v, tol in self.rows if not v < tol]
        assert not bad, "%s: %s" % (self.case, bad)


def train_plan(m, opt='Adam'):
    return m.optimisers[opt].step.func


# ---- the route every case names ----------------------------------------------------------------------
def assert_routes(name, m, plan, **opt):
    from elektronn2_amd.neuromancer import neural
    a, b = m.nodes['a'], m.nodes['b']
    for k in NETS[name][2]:
        assert getattr(b, k) is getattr(a, k) and plan.shared(getattr(a, k))
    assert all(n in plan.nodes for n in (a, b))
    if name in ('S1', 'S2', 'S8', 'S9'):
        assert type(a) is neural.Conv and type(b) is neural.Conv
        assert a._route(plan) == 'gemm' and b._route(plan) == 'gemm'
    if name == 'S1':
        assert m.nodes['stem']._route(plan) == 'first'
        assert b._p3 == (1, 1, 1) and a._p3 == (1, 2, 2)
        if plan.training:
            assert a._sig_wgrad(plan) != b._sig_wgrad(plan)
        assert a._sig_fwd(plan) != b._sig_fwd(plan)
    elif name == 'S2':
        if plan.training:
            assert a._sig_wgrad(plan) == b._sig_wgrad(plan) and a._sig_dgrad(plan) == b._sig_dgrad(plan)
        assert a._sig_fwd(plan) == b._sig_fwd(plan)
    elif name == 'S3':
        assert type(a) is neural.UpConv and type(b) is neural.UpConv
        packed = opt.get('upconv_packed', True)
        for n in (a, b):
            assert ((n, 'wp_f') in plan.scratch) == packed
            if plan.training:
                assert ((n, 'wp_d') in plan.scratch) == packed
        if packed:
            assert plan.scratch[a, 'wp_f'].data_ptr() != plan.scratch[b, 'wp_f'].data_ptr()
    elif name == 'S4':
        assert a._route(plan) == 'first' and b._route(plan) == 'gemm'
        assert b.parent.shape['f'] == 1 and not b.parent.is_source
    elif name == 'S5':
        tail = plan.training and opt.get('fuse_tail', True)
        assert a._route(plan) == 'gemm'
        assert b._route(plan) == ('tail' if tail else 'gemm')
        assert m.nodes['head']._route(plan) == 'head'
        assert a._k3 == (1, 1, 1) and b._k3 == (1, 1, 1)
    elif name == 'S6':
        fused = opt.get('fuse_multihead', True)
        heads = m.loss_node._fused_heads(plan) if plan.training else None
        if plan.training:
            assert (heads is not None) == fused
            if fused:
                assert any(h is a for h in heads) and any(h is b for h in heads)
            assert a._route(plan) == b._route(plan) == ('head' if fused else 'gemm')
    elif name == 'S7':
        assert type(a) is neural.Perceptron and type(b) is neural.Perceptron
    elif name == 'S8':
        assert a._bn() and b._bn() and a.gamma is b.gamma and a.w is not b.w
    elif name == 'S9':
        assert a._valid_mode() and not b._valid_mode()
        assert (b, 'xf') in plan.scratch and (a, 'xf') not in plan.scratch


# ---- the comparison ----------------------------------------------------------------------------------
def compare_forward_and_gradients(fig, m, r, which, tol=None):
    x, t = S.batch(r)
    end = which == 'end'
    fig.add("loss (%s)" % which, float(m.loss(x, t)), r['loss_end' if end else 'loss0'], tol)
    fig.add("predict (%s)" % which, m.predict(x), r['pred_end' if end else 'pred0'], tol)
    got = m.gradients(x, t)
    ref = r['grads_end' if end else 'grads0']
    assert len(got) == len(ref) == len(m.trainable_params)
    names = list(m.loss_node.all_trainable_params.keys())
    for k, g, g0 in zip(names, got, ref):
        fig.add("d/d%s (%s)" % (k, which), g, g0, tol)


def compare_params(fig, m, ref_params, what):
    names = list(m.loss_node.all_trainable_params.keys())
    for k, p, p0 in zip(names, m.trainable_params, ref_params):
        fig.add("%s %s" % (k, what), p.get_value(), p0)


def run_protocol(name, case, **opt):
    """loss, predict, gradients; four Adam steps (one eager, then replays unless graph=False);
    predict and gradients again with the updated weights -- both users' images refreshed"""
    from elektronn2_amd.neuromancer import plan_options
    r = S.reference(name)
    fig = Figures("%s %s" % (name, case))
    with plan_options(**opt):
        m = S.build(name)
        compare_forward_and_gradients(fig, m, r, 'start')
        for s in range(N_STEPS):
            loss = m.trainingstep(*S.batch(r), optimiser='Adam')[0]
            fig.add("loss of step %d" % s, float(loss), r['losses'][s])
        compare_params(fig, m, r['params'][-1], "after %d steps" % N_STEPS)
        compare_forward_and_gradients(fig, m, r, 'end')
        plan = train_plan(m)
        assert plan.use_graph == opt.get('graph', True)
        for p in (plan, m._grad_func.func, m.prediction_node._output_func.func):
            assert_routes(name, m, p, **opt)
    fig.check()
    return m


@pytest.mark.parametrize("name", sorted(NETS))
def test_default_options(name):
    run_protocol(name, "default")


@pytest.mark.parametrize("name", ['S1', 'S3', 'S5'])
def test_eager_only(name):
    run_protocol(name, "graph=False", graph=False)


@pytest.mark.parametrize("name", ['S1', 'S4', 'S5'])
def test_adam_launch_writes_the_weight_images(name):
    """adam_pack: the update job holds one image pair per parameter; a shared weight has one pair
    per user, so the plan keeps the repack launch (every image current) -- an unshared net keeps
    the fused update"""
    m = run_protocol(name, "adam_pack", adam_pack=True)
    plan = train_plan(m)
    images = [(mode, wp.data_ptr()) for (w, wp, mode) in plan.pack_jobs if w is m.nodes['a'].w]
    assert len(images) == len(set(images)) >= 2
    modes = [mode for mode, _ in images]
    several = len(set(modes)) < len(modes)           # (S4: the fused first layer reads no image)
    assert several == (name != 'S4')
    assert (plan._upd is None) == several and plan._pack_dev is not None
    if plan._upd is None:
        return           # (the head of every step repacks every image: the default path)
    # the update launch wrote the images: each equals a fresh pack of its parameter -- an image
    # that the update job does not hold lags behind
    torch.cuda.synchronize()
    old = plan.ctx.stream
    plan.ctx.set_stream(plan.stream)
    try:
        with torch.cuda.stream(plan.stream):       # (one stream: the copies, then the repack)
            held = [wp.clone() for (_, wp, _) in plan.pack_jobs]
            plan.ctx.conv3d_pack_multi(*plan._pack_dev)
    finally:
        plan.ctx.set_stream(old)
    torch.cuda.synchronize()
    owner = {id(plan.scratch[k]): k[0].name for k in plan.scratch
             if isinstance(k, tuple) and len(k) == 2 and k[1] in ('wp_f', 'wp_d')}
    stale = [(owner.get(id(wp)), mode) for (w, wp, mode), h in zip(plan.pack_jobs, held)
             if not torch.equal(wp, h)]
    assert not stale, "images that did not hold the current weights: %s" % (stale,)


def test_adam_pack_stays_fused_without_sharing():
    from elektronn2_amd import nets, neuromancer as nm
    from elektronn2_amd.neuromancer import plan_options
    from oracle import e2_oracle as O
    with plan_options(adam_pack=True):
        nm.model_manager.reset()
        sp = (7, 47, 47)
        m = nets.neuro3d_lite((None, 1) + sp, params=O.init_net(O.NEURO3D_LITE, 1, seed=1))
        m.set_opt_meta_params('Adam', ADAM)
        rng = np.random.RandomState(0)
        x = rng.rand(1, 1, *sp).astype(np.float32)
        t = rng.randint(0, 2, (1, 1) + O.net_out_shape(O.NEURO3D_LITE, sp)).astype(np.float32)
        m.trainingstep(x, t, optimiser='Adam')
        plan = train_plan(m)
        assert plan._upd is not None and not plan._shared_ids


def test_upconv_repacks_inside_its_calls():
    run_protocol('S3', "upconv_packed=False", upconv_packed=False)


def test_upconv_repacks_inside_its_calls_eager():
    run_protocol('S3', "upconv_packed=False graph=False", upconv_packed=False, graph=False)


def test_weight_gradients_on_the_side_stream():
    m = run_protocol('S1', "side_stream", side_stream=True)
    assert train_plan(m).use_side


def test_tail_off_head_and_pointwise_gemm():
    run_protocol('S5', "fuse_tail=False", fuse_tail=False)


def test_heads_as_ordinary_launches():
    run_protocol('S6', "fuse_multihead=False", fuse_multihead=False)


# ---- the tuner runs --------------------------------------------------------------------------------------
@contextlib.contextmanager
def fresh_tuner(monkeypatch, keep=8):
    """an empty in-process table and a scratch cache file: every signature is tuned at first sight
    (over the first ``keep`` candidates of each list -- the path through tuned_call is the same).
    The table, the rankings and the environment are restored; the user's cache is never written."""
    from elektronn2_amd import autotune
    assert autotune.enabled()
    table = autotune._load()
    saved, ranks, dirty = dict(table), dict(autotune.last_ranking), autotune._dirty
    env = os.environ.get("E2HIP_TUNE_CACHE")
    scratch = tempfile.mkdtemp(prefix="e2_tune_")
    os.environ["E2HIP_TUNE_CACHE"] = os.path.join(scratch, "tune_cache.json")
    table.clear()
    autotune.last_ranking.clear()
    for fn in ('wgrad_candidates', 'igemm_candidates'):
        orig = getattr(autotune, fn)
        monkeypatch.setattr(autotune, fn, (lambda o: lambda *a, **k: o(*a, **k)[:keep])(orig))
    try:
        yield autotune
    finally:
        monkeypatch.undo()
        table.clear()
        table.update(saved)
        autotune.last_ranking.clear()
        autotune.last_ranking.update(ranks)
        autotune._dirty = dirty
        if env is None:
            os.environ.pop("E2HIP_TUNE_CACHE", None)
        else:
            os.environ["E2HIP_TUNE_CACHE"] = env
        shutil.rmtree(scratch, ignore_errors=True)


def wgrad_keys(m, plan):
    """the tuning keys of the weight-gradient launches of the two users (the fused first layer
    has none: its backward is one untuned launch)"""
    from elektronn2_amd import tiling
    from elektronn2_amd.neuromancer import neural
    keys = []
    for n in (m.nodes['a'], m.nodes['b']):
        if type(n) is neural.UpConv:
            sig = n._tune_sigs(plan)['wgrad'][0]
        elif n._route(plan) == 'gemm':
            sig = n._sig_wgrad(plan)
        else:
            continue
        keys.append(tiling.key('wgrad', sig, False))
    return keys


@pytest.mark.parametrize("name", ['S1', 'S3', 'S4'])
def test_gradients_of_the_call_that_tunes(name, monkeypatch):
    """the first gradients() of a process that has tuned nothing: every launch is tuned at first
    sight, and the timing runs of one user must not wipe what the other added to the shared slot"""
    r = S.reference(name)
    fig = Figures("%s tuned gradients" % name)
    with fresh_tuner(monkeypatch) as autotune:
        m = S.build(name)
        got = m.gradients(*S.batch(r))
        plan = m._grad_func.func
        keys = wgrad_keys(m, plan)
        assert len(keys) == (1 if name == 'S4' else 2) and len(set(keys)) == len(keys)
        for k in keys:
            assert k in autotune.last_ranking and len(autotune.last_ranking[k]) > 1, k
        assert_routes(name, m, plan)
    for k, g, g0 in zip(m.loss_node.all_trainable_params.keys(), got, r['grads0']):
        fig.add("d/d%s" % k, g, g0)
    fig.check()


@pytest.mark.parametrize("name", ['S1', 'S3', 'S4'])
def test_training_step_that_tunes(name, monkeypatch):
    """the same for the training plan: loss and parameters of that very first step, then replays"""
    r = S.reference(name)
    fig = Figures("%s tuned step" % name)
    with fresh_tuner(monkeypatch) as autotune:
        m = S.build(name)
        loss = m.trainingstep(*S.batch(r), optimiser='Adam')[0]
        plan = train_plan(m)
        for k in wgrad_keys(m, plan):
            assert k in autotune.last_ranking and len(autotune.last_ranking[k]) > 1, k
        fig.add("loss of the tuning step", float(loss), r['losses'][0])
        compare_params(fig, m, r['params'][0], "after the tuning step")
        for s in range(1, N_STEPS):
            loss = m.trainingstep(*S.batch(r), optimiser='Adam')[0]
            fig.add("loss of step %d" % s, float(loss), r['losses'][s])
        compare_params(fig, m, r['params'][-1], "after %d steps" % N_STEPS)
        assert_routes(name, m, plan)
    fig.check()


# ---- several steps per launch ------------------------------------------------------------------------
def test_three_steps_in_one_launch():
    r = S.reference('S1')
    fig = Figures("S1 trainingsteps")
    m = S.build('S1')
    loss = m.trainingstep(*S.batch(r), optimiser='Adam')[0]
    fig.add("loss of step 0", float(loss), r['losses'][0])
    plan = train_plan(m)
    ring = torch.zeros(2, plan.input_arena.numel(), device=plan.ctx.device)
    for j in range(2):
        for node, src in zip(plan.inputs, S.batch(r)):
            o, n = plan.input_slices[node]
            assert n == src.size
            ring[j, o:o + n] = torch.tensor(src.ravel(), device=ring.device)
    losses, _ = m.trainingsteps(3, optimiser='Adam', ring=ring)
    for s, l in enumerate(losses):
        fig.add("loss of step %d" % (s + 1), float(l), r['losses'][s + 1])
    compare_params(fig, m, r['params'][3], "after 1 + 3 steps")
    assert_routes('S1', m, plan)
    fig.check()


# ---- the other optimisers ----------------------------------------------------------------------------
HYPER = dict(lr=1e-3, mom=0.9, wd=0.5e-4)


def reference_steps(name, optimiser, k):
    """k steps of ``optimiser`` on the reference, with the float64 restatements of
    tests/test_optimiser_host.py and tests/test_adaptive_optimisers_host.py"""
    import test_adaptive_optimisers_host as A
    import test_optimiser_host as H
    from elektronn2_amd.neuromancer.variables import reg_multiplier
    r = S.reference(name)
    m = S.build(name)
    ref = S.SRef(m)
    state = [dict(d=0.0, h=0.0, s=0.0) for _ in m.trainable_params]
    losses = []
    for step in range(k):
        losses.append(ref.loss_and_grads(*S.batch(r))[0])
        for par, st, g in zip(m.trainable_params, state, ref.grads()):
            p = ref.p(par).detach().numpy()
            mult = np.full(p.shape, reg_multiplier(par))
            zero = np.zeros(p.shape)
            if optimiser == 'SGD':
                new, _ = H.sgd_ref(p, g, st['d'] + zero, mult, HYPER)
            elif optimiser == 'AdaGrad':
                new, _ = A.adagrad_ref(p, g, st['h'] + zero, mult, HYPER, step)
            else:
                new, _ = A.adadelta_ref(p, g, st['s'] + zero, st['d'] + zero, mult, HYPER)
            st.update({q: v for q, v in new.items() if q != 'p'})
            with torch.no_grad():
                ref.p(par).copy_(torch.tensor(new['p']))
    return losses, [ref.p(p).detach().numpy() for p in m.trainable_params]


@pytest.mark.parametrize("name,optimiser", [('S1', 'SGD'), ('S3', 'SGD'), ('S1', 'AdaGrad'),
                                            ('S1', 'AdaDelta')])
def test_other_optimisers_update_a_shared_parameter_once(name, optimiser):
    k = 3
    ref_losses, ref_params = reference_steps(name, optimiser, k)
    r = S.reference(name)
    fig = Figures("%s %s" % (name, optimiser))
    m = S.build(name)
    m.set_opt_meta_params(optimiser, HYPER)
    for s in range(k):
        loss = m.trainingstep(*S.batch(r), optimiser=optimiser)[0]
        fig.add("loss of step %d" % s, float(loss), ref_losses[s])
    compare_params(fig, m, ref_params, "after %d steps" % k)
    assert_routes(name, m, train_plan(m, optimiser))
    fig.check()


# ---- bf16 operands -------------------------------------------------------------------------------------
from test_bf16_gpu import process_bf16          # noqa: E402,F401  (the fixture of that file, unchanged)

BF16_LOSS, BF16_GRAD = S.BF16_LOSS, S.BF16_GRAD


def test_bf16_mode(process_bf16):
    """S1 with bf16 operands against the reference of the f32 net, with the bounds of
    test_training_step_bf16_close_to_f32_oracle.  (Each contribution to S1's shared gradients
    exceeds 10x the gradient bound: test_shared_params_host.py.  No seed of S5 gives that, so S5
    has no bf16 variant.)"""
    r = S.reference('S1')
    fig = Figures("S1 bf16", BF16_GRAD)
    m = S.build('S1')
    x, t = S.batch(r)
    loss = float(m.loss(x, t))
    fig.add("loss", loss, r['loss0'], BF16_LOSS)
    assert abs(loss - r['loss0']) > 1e-7 * abs(r['loss0'])         # not the f32 path
    got = m.gradients(x, t)
    for k, g, g0 in zip(m.loss_node.all_trainable_params.keys(), got, r['grads0']):
        fig.add("d/d%s" % k, g, g0)
    for s in range(N_STEPS):
        loss = m.trainingstep(x, t, optimiser='Adam')[0]
        fig.add("loss of step %d" % s, float(loss), r['losses'][s], BF16_LOSS)
    got = m.gradients(x, t)
    for k, g, g0 in zip(m.loss_node.all_trainable_params.keys(), got, r['grads_end']):
        fig.add("d/d%s (end)" % k, g, g0)
    assert_routes('S1', m, train_plan(m))
    fig.check()
