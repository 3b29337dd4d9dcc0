"""Activations shared between nodes (fan-out), on the GPU: every launch that overwrites -- or adds
to -- the output gradient of a node with several consumers, and every fused route that has to
stand down there, against the float64 reference of tests/wiring_cases.py (``WRef``; autograd sums
the consumers' contributions).  Bound: 1e-4 of the reference's largest magnitude
(tests/test_model_gpu.py:17); one route against another 1e-5 (losses) / 1e-4 (parameters)
(tests/test_conv_modes_gpu.py).  tests/test_wiring_host.py shows on the reference alone that
dropping or doubling the gradient along any single consumer edge moves some parameter gradient by
more than 10x that bound, so a wrong `first` flag, a missing `accumulate` or a fusion that fails to
stand down cannot pass.  Everything runs under ``debug_poison``: a gradient buffer read before its
first writer shows as NaN.

Every net exists in two orders (wiring_cases: ``flip``), so that each writer kind -- valid and
'same' Conv data gradient, split-K data gradient, UpConv, max / average Pool, LRN, Perceptron,
Crop, Pad, a copied Concat slice, Add -- is once the first writer (overwrites) and once a later
one (adds).  The fused head and the fused multi-head launches are the only gradient writers of
their trunk wherever they run (see ``test_fused_heads_are_the_only_writers_of_their_trunk``).
Every case asserts the route it names and prints its route record."""
import contextlib
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import wiring_cases as W
from wiring_cases import CASES, CASE_IDS, N_STEPS
from test_shared_params_gpu import Figures as _Figures, train_plan

pytestmark = pytest.mark.gpu


class Figures(_Figures):
    """``show`` prints every figure (once); ``check`` shows them, then asserts.  A test calls ``show``
    before its route assertions, so that a failing route hides no figure."""
    shown = False

    def show(self):
        if not self.shown:
            for what, v, tol in self.rows:
                print("%s: %s %.3g (bound %.0e)" % (self.case, what, v, tol))
        self.shown = True

    def check(self):
        self.show()
        bad = [(w, v) for w, v, tol in self.rows if not v < tol]
        assert not bad, "%s: %s" % (self.case, bad)


# ---- the route every case names ----------------------------------------------------------------------
def route_record(name, flip, m, plan):
    """[(fan-out node, consumer, kind, 'first' | 'later')] of a TRAINING plan, printed: the graph's
    writer kinds (wiring_cases.writers over plan._bwd_nodes()) refined by what the plan tells --
    the route of a Conv, split-K parts left by a first writer, a Concat slice copied or aliased"""
    ws = W.writers(m, plan._bwd_nodes())
    rec = []
    fused = getattr(m.loss_node, '_fused_heads', lambda p: None)(plan) or []
    for node, lst in ws.items():
        fan = m.nodes[node]
        mh = [w for w in lst if any(h is m.nodes[w[0]] for h in fused)]
        if mh:      # the heads of the fused multi-head launches: ONE writer, where the first of them stands
            at = lst.index(mh[0])
            lst = [w for w in lst if w not in mh]
            lst.insert(at, ("+".join(w[0] for w in mh), 0, 'multihead'))
        for i, (cname, slot, kind) in enumerate(lst):
            c = m.nodes.get(cname)
            if type(c).__name__ == 'Conv':
                route = c._route(plan)
                if route != 'gemm':
                    kind = route
                elif i == 0 and plan.scratch.get((fan, 'grad_nparts'), 1) > 1:
                    kind += '_splitk'             # partial sums in the parent's slabs
                elif i > 0 and plan.scratch.get((c, 'dgrad_atomics')):
                    kind += '_splitk'             # onto a zero fill of the scratch tensor
            elif kind == 'concat':
                kind += '_alias' if 'grad' in plan.scratch[c, 'alias'].get(fan, '') else '_copy'
            rec.append((node, "%s[%d]" % (cname, slot), kind, 'first' if i == 0 else 'later'))
    for r in rec:
        print("%s%s route record: d/d%s <- %s: %s, %s" % ((name, '-flip' if flip else '') + r))
    return rec


def assert_routes(name, flip, m, plan, **opt):
    from elektronn2_amd.neuromancer import neural
    n = m.nodes
    route = lambda k: n[k]._route(plan)
    train = plan.training
    tail_on = train and opt.get('fuse_tail', True)
    if train:
        ws = W.writers(m, plan._bwd_nodes())
        assert dict((k, v[0][0]) for k, v in ws.items()) == W.FIRST[name, flip]
        # fuse_actbwd: the consumer's data gradient never carries the activation backward of a node
        # whose gradient has another writer
        for fan in ws:
            assert (n[fan], 'dy_done') not in plan.scratch, fan
            assert (n[fan], 'dy_by_tail') not in plan.scratch, fan
    head_in_plan = 'head' in n and any(q is n['head'] for q in plan.nodes)
    if head_in_plan and 'probs' in n and any(q is n['probs'] for q in plan.nodes) \
            and type(n['head']) is neural.Conv:
        assert route('head') == ('gemm' if name == 'head_kid' else 'head')
    if name == 'residual':
        assert route('a') == 'first' and [route(k) for k in 'bcd'] == ['gemm'] * 3
        # (the fused first layer wants dense output rows: the 'same' conv pads by launch)
        assert plan.scratch.get((n['b'], 'xf_launch')) is True and (n['b'], 'xf') in plan.scratch
        assert (n['a'], 'frame') not in plan.scratch
    elif name == 'head_kid':
        # two children: not the form of a fused head; the logits exist, the NLL writes their gradient
        assert len(n['head'].children) == 2 and n['head']._head_form(plan) is None
        assert [route(k) for k in 'auv'] == ['gemm'] * 3
        if any(q is n['head'] for q in plan.nodes):
            assert plan.out[n['head']] is not None
        if train:
            assert (n['nll'], 'head_ws') not in plan.scratch and n['head'] in plan.grad
            if plan.updates_params():
                assert any(q is n['aux'] for q in plan.outputs)
    elif name == 'unet_cat':
        assert route('c0') == 'first' and [route(k) for k in ('c1', 'low', 'post')] == ['gemm'] * 3
        # the Concat hands the UpConv its output slice and both parents their gradient slices; the
        # Crop's parent c1 is the fan-out node: its gradient is written FROM the concat's slice
        alias = plan.scratch[n['merge'], 'alias']
        want = {} if not opt.get('concat_alias', True) else \
            {'UpConv': 'out+grad', 'Crop': 'grad'} if train else {'UpConv': 'out'}
        assert dict((type(k).__name__, v) for k, v in alias.items()) == want
        assert ((n['merge'], 'frame') in plan.scratch) == opt.get('pad_inplace', True)
    elif name == 'unet_add':
        assert route('c0') == 'first' and [route(k) for k in ('c1', 'low', 'post')] == ['gemm'] * 3
        inplace = opt.get('pad_inplace', True)
        # the Add writes into the framed image the 'same' conv reads
        assert ((n['merge'], 'frame') in plan.scratch) == inplace
        assert (plan.scratch.get((n['post'], 'xf_launch')) is True) == (not inplace)
        if train:          # (slabs for split-K partial sums, unless the fused activation backward is on)
            assert ((n['c1'], 'grad_parts') in plan.scratch) == (not opt.get('fuse_actbwd'))
    elif name == 'tail_shaped':
        assert [route(k) for k in ('b', 't1', 'side')] == ['gemm'] * 3
        assert (n['t1'], 'tail_ws') not in plan.scratch
    elif name == 'tail_kid':
        assert len(n['t1'].children) == 2
        assert route('t1') == 'gemm' and route('b') == 'gemm'
        assert (n['b'], 'dy_by_tail') not in plan.scratch
        if train and opt.get('fuse_actbwd'):       # (b has ONE writer: the fusion may engage there)
            assert plan.scratch.get((n['b'], 'dy_done')) is True
    elif name == 'tail_plain':
        assert route('t1') == ('tail' if tail_on else 'gemm') and route('b') == 'gemm'
        if train and plan._calls:
            assert bool(plan.scratch.get((n['b'], 'dy_by_tail'))) == (tail_on and opt.get('tail_gm', True))
    elif name.startswith('fan_'):
        assert route('c0') == 'first' and route('a') == 'gemm' and route('post') == 'gemm'
        if 'w_same' in n:        # the parent's pooling / activation pass writes the framed image
            assert (n['a'], 'frame') in plan.scratch and (n['w_same'], 'xf_launch') not in plan.scratch
        if 'w_upconv' in n:
            assert type(n['w_upconv']) is neural.UpConv and (n['w_upconv'], 'wp_f') in plan.scratch
    elif name == 'cat_copy':
        assert [route(k) for k in 'abcd'] == ['gemm'] * 4
        assert plan.scratch[n['cat'], 'alias'] == {}             # a Conv parent is always copied
    elif name == 'twice':
        assert route('a') == 'gemm' and route('c') == 'gemm'
        # the Crop feeds only the Concat, but twice: its gradient is no slice of the concat's
        assert plan.scratch[n['cat'], 'alias'] == {}
    elif name == 'dense':
        assert route('a') == 'gemm'
        assert all(type(n[k]) is neural.Perceptron for k in ('p1', 'p2', 'head'))
    elif name == 'two_valid':
        assert [route(k) for k in 'auv'] == ['gemm'] * 3
        if train:
            assert ((n['a'], 'grad_parts') in plan.scratch) == (not opt.get('fuse_actbwd'))
    elif name == 'pred_trunk':
        assert [route(k) for k in 'auv'] == ['gemm'] * 3         # (u: its child is the Add, no tail)
        if train:
            assert (m.nodes['nll'], 'head_ws') in plan.scratch
            if plan.updates_params():
                assert any(q is n['aux'] for q in plan.outputs) and route('aux') == 'gemm'
    elif name == 'mh_fused':
        if train:
            heads = m.loss_node._fused_heads(plan)
            fused = opt.get('fuse_multihead', True)
            assert (heads is not None) == fused
            assert route('head0') == route('head1') == ('head' if fused else 'gemm')
            if plan.updates_params():
                assert any(q is n['side'] for q in plan.nodes) and route('side') == 'gemm'
    elif name == 'mh_third':
        if train:              # the third head stands on another trunk: none of them is fused
            assert m.loss_node._fused_heads(plan) is None
            assert [route(k) for k in ('head0', 'head1', 'head2', 'side')] == ['gemm'] * 4


# ---- the comparison ----------------------------------------------------------------------------------
def compare_forward_and_gradients(fig, m, r, which, tol=None):
    x, t = W.batch(r)
    end = which == 'end'
    fig.add("loss (%s)" % which, float(m.loss(x, t)), r['loss_end' if end else 'loss0'], tol)
    fig.add("predict (%s)" % which, m.predict(x), r['pred_end' if end else 'pred0'], tol)
    got = m.gradients(x, t)
    ref = r['grads_end' if end else 'grads0']
    assert len(got) == len(ref) == len(m.trainable_params)
    for k, g, g0 in zip(m.loss_node.all_trainable_params.keys(), got, ref):
        fig.add("d/d%s (%s)" % (k, which), g, g0, tol)


def compare_params(fig, m, ref_params, what):
    for k, p, p0 in zip(m.loss_node.all_trainable_params.keys(), m.trainable_params, ref_params):
        fig.add("%s %s" % (k, what), p.get_value(), p0)


def run_protocol(name, flip, case, **opt):
    """loss, predict, gradients; four Adam steps (one eager, then replays unless graph=False); loss,
    predict and gradients again with the updated weights"""
    from elektronn2_amd.neuromancer import plan_options
    r = W.reference(name, flip)
    fig = Figures("%s%s %s" % (name, '-flip' if flip else '', case))
    with plan_options(debug_poison=True, **opt):
        m = W.build(name, flip)
        compare_forward_and_gradients(fig, m, r, 'start')
        for s in range(N_STEPS):
            loss = m.trainingstep(*W.batch(r), optimiser='Adam')[0]
            fig.add("loss of step %d" % s, float(loss), r['losses'][s])
        compare_params(fig, m, r['params'][-1], "after %d steps" % N_STEPS)
        compare_forward_and_gradients(fig, m, r, 'end')
        plan = train_plan(m)
        fig.show()                               # every figure, before any assertion
        rec = route_record(name, flip, m, plan)
        assert plan.opt['debug_poison'] and plan.use_graph == opt.get('graph', True)
        for p in (plan, m._grad_func.func, m.prediction_node._output_func.func):
            assert_routes(name, flip, m, p, **opt)
    fig.check()
    return m, rec


@pytest.mark.parametrize("name,flip", CASES, ids=CASE_IDS)
def test_default_options(name, flip):
    run_protocol(name, flip, "default")


# ---- option sweeps -------------------------------------------------------------------------------------
SWEEP_NETS = ('residual', 'unet_add', 'tail_shaped')
# ... and where an option changes no plan of those three, the nets whose plans it does change
SWEEP_MORE = {'concat_alias': ('cat_copy', 'unet_cat'), 'pad_inplace': ('unet_cat',),
              'fuse_tail': ('tail_plain',), 'tail_gm': ('tail_plain',)}
SWEEPS = [dict(graph=False), dict(fuse_actbwd=1), dict(tail_gm=False), dict(fuse_tail=False),
          dict(concat_alias=False), dict(pad_inplace=False), dict(side_stream=True)]


def _oid(o):
    return ",".join("%s=%s" % kv for kv in sorted(o.items()))


@pytest.mark.parametrize("opt", SWEEPS, ids=_oid)
@pytest.mark.parametrize("name", SWEEP_NETS)
def test_option_sweep(name, opt):
    flip = bool(SWEEPS.index(opt) % 2)          # (both orders meet the options)
    m, _ = run_protocol(name, flip, _oid(opt), **opt)
    plan = train_plan(m)
    if 'side_stream' in opt:
        assert plan.use_side
    if 'fuse_actbwd' in opt:
        assert plan.fuse_actbwd == 1
        # (split-K slabs and the fused activation backward exclude each other: Conv._parts_ok)
        assert not any(isinstance(k, tuple) and len(k) == 2 and k[1] == 'grad_parts' for k in plan.scratch)


@pytest.mark.parametrize("name,opt", [(nme, o) for o in SWEEPS for k in o for nme in SWEEP_MORE.get(k, ())] +
                                     [('tail_kid', dict(fuse_actbwd=1)), ('head_kid', dict(fuse_actbwd=1)),
                                      ('two_valid', dict(fuse_actbwd=1)), ('mh_fused', dict(fuse_multihead=False))],
                         ids=lambda v: _oid(v) if isinstance(v, dict) else v)
def test_controls_of_the_fused_routes(name, opt):
    """the nets whose plans an option of the sweep changes (SWEEP_MORE): the Concat nets with
    concat_alias off -- unet_cat then copies both parents, forward and backward -- the tail with
    each of its switches off; fuse_actbwd where the parent has ONE writer (it
    engages: tail_kid) and where it has two (it declines: assert_routes); the two heads of mh_fused
    as ordinary launches -- the trunk's gradient then has two 'gemm' writers"""
    flip = name in ('two_valid', 'unet_cat')
    m, rec = run_protocol(name, flip, _oid(opt), **opt)
    if name == 'mh_fused':
        assert [(r[2], r[3]) for r in rec] == [('conv_valid', 'first'), ('conv_valid', 'later')]


# ---- the heads ---------------------------------------------------------------------------------------
def test_fused_heads_are_the_only_writers_of_their_trunk():
    """head_bwd and multihead_bwd take ``accumulate_dx = not first``.  A second writer of their
    trunk's gradient would have to reach the loss past the head: under a single NLL there is no
    such path, and a further NLL term on another trunk takes every head of the aggregate off the
    fused route (AggregateLoss._fused_heads; mh_third).  What can be built is a trunk with a
    second consumer OFF the loss path -- the trunk as the prediction output, a Conv on it as an
    extra output of the step: the fused launch is then the first and only writer, and the
    trunk's gradient (poisoned beforehand) must come out whole."""
    for name in ('pred_trunk', 'mh_fused'):
        m, rec = run_protocol(name, False, "heads")
        plan = train_plan(m)
        trunk = m.nodes['trunk' if name == 'pred_trunk' else 'a']
        kids = [c for c in trunk.children.values() if any(q is c for q in plan.nodes)]
        assert len(kids) == (2 if name == 'pred_trunk' else 3)
        assert id(trunk) in plan._grad_written and torch.isfinite(plan.grad[trunk]).all()
        if name == 'pred_trunk':      # (one writer on the loss path: no entry of route_record)
            assert m.nodes['head']._route(plan) == 'head'
            print("pred_trunk route record: d/dtrunk <- head[0]: head, first (the only writer)")
        if name == 'mh_fused':
            assert [(r[1], r[2], r[3]) for r in rec] == [('head1+head0[0]', 'multihead', 'first')]


def test_logits_with_two_gradient_writers_are_refused():
    """one (1,1,1) 'lin' conv read by two Softmax nodes, each under a sparse NLL of its own in one
    AggregateLoss: two writers of the logits' gradient.  The loss launches overwrite it
    (e2_nll_multi_bwd has no accumulating form), so the form is refused -- "logits consumed by
    several nodes" -- when the backward pass is issued, never a silent result.  The forward runs."""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(6)
    inp = nm.Input((1, 1, 4, 12, 12), 'b,f,z,x,y', name='raw')
    a = nm.Conv(nm.Conv(inp, 4, (1, 3, 3), name='c0'), 6, (1, 3, 3), name='a')
    logits = nm.Conv(a, 2, (1, 1, 1), activation_func='lin', name='head')
    sms = [nm.Softmax(logits, name='probs%d' % k) for k in range(2)]
    target = nm.Input_like(sms[0], override_f=2, name='target')
    parts = nm.split(target, 'f', n_out=2)
    nlls = [nm.MultinoulliNLL(s, t, target_is_sparse=True, name='nll%d' % k)
            for k, (s, t) in enumerate(zip(sms, parts))]
    loss = nm.AggregateLoss(nlls, mixing_weights=[1.5, 0.5], name='loss')
    m = nm.model_manager.getmodel()
    m.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=sms[0])
    m.set_opt_meta_params('Adam', W.ADAM)
    m._classes = (2, 2)
    x, t = W.batch_for(m, 8)
    ref_loss = float(W.WRef(m).forward(x, t)[0].detach())
    assert abs(float(m.loss(x, t)) - ref_loss) < W.TOL * abs(ref_loss)
    with pytest.raises(NotImplementedError, match="consumed by several"):
        m.gradients(x, t)
    with pytest.raises(NotImplementedError, match="consumed by several"):
        m.trainingstep(x, t, optimiser='Adam')
    assert len(logits.children) == 2 and logits._route(m._grad_func.func) == 'gemm'


def test_a_split_part_that_needs_a_gradient_is_refused():
    """fan-out through ``split`` of a tensor with trainable parameters upstream: refused when the
    training plan is built, never a silent result"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(5)
    inp = nm.Input((1, 1, 4, 12, 12), 'b,f,z,x,y', name='raw')
    a = nm.Conv(nm.Conv(inp, 4, (1, 3, 3), name='c0'), 6, (1, 3, 3), name='a')
    lo, hi = nm.split(a, 'f', n_out=2)
    m = W._finish(nm, inp, W._head(nm, nm.Add(lo, hi, name='merge')))
    x, t = W.batch_for(m, 7)
    assert m.predict(x).shape == (1, 2, 4, 8, 8)                     # (forward only: views)
    with pytest.raises(NotImplementedError, match="needs a gradient"):
        m.gradients(x, t)
    with pytest.raises(NotImplementedError, match="needs a gradient"):
        m.trainingstep(x, t, optimiser='Adam')


# ---- split-K partial sums of a first writer, then a second writer onto slab 0 -------------------------
def _splits_k(c):
    from elektronn2_amd import tiling
    t = tiling.parse('igemm', c)
    if t is None:
        return False
    return {'16x16x4': lambda v: v[3] > 1, '4x4x1': lambda v: v[4] > 1}.get(t.family, lambda v: False)(t.v)


@contextlib.contextmanager
def split_k_tuner(monkeypatch, keep=8):
    """``fresh_tuner`` of tests/test_shared_params_gpu.py -- an empty in-process table and a scratch
    cache file, everything restored -- with the conv GEMM candidates narrowed to those that split K"""
    from elektronn2_amd import autotune
    assert autotune.enabled()
    table = autotune._load()
    saved, ranks, dirty = dict(table), dict(autotune.last_ranking), autotune._dirty
    env = os.environ.get("E2HIP_TUNE_CACHE")
    scratch = tempfile.mkdtemp(prefix="e2_tune_")
    os.environ["E2HIP_TUNE_CACHE"] = os.path.join(scratch, "tune_cache.json")
    table.clear()
    autotune.last_ranking.clear()
    orig = autotune.igemm_candidates
    monkeypatch.setattr(autotune, 'igemm_candidates',
                        lambda *a, **k: [c for c in orig(*a, **k) if _splits_k(c)][:keep])
    worig = autotune.wgrad_candidates
    monkeypatch.setattr(autotune, 'wgrad_candidates', lambda *a, **k: worig(*a, **k)[:keep])
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


@pytest.mark.parametrize("flip", [False, True], ids=["v_first", "u_first"])
def test_split_k_first_writer_then_a_second_writer(flip, monkeypatch):
    """Conv a -> two valid (3,3,3) Convs.  The first writer's data gradient leaves its split-K
    partial sums in a's slabs; the second goes to a scratch tensor and is added onto slab 0; a's
    activation backward adds the slabs up."""
    from elektronn2_amd.neuromancer import plan_options
    r = W.reference('two_valid', flip)
    fig = Figures("two_valid%s split-K" % ('-flip' if flip else ''))
    with split_k_tuner(monkeypatch), plan_options(debug_poison=True):
        m = W.build('two_valid', flip)
        got = m.gradients(*W.batch(r))
        for k, g, g0 in zip(m.loss_node.all_trainable_params.keys(), got, r['grads0']):
            fig.add("d/d%s" % k, g, g0)
        for s in range(2):                       # the eager step, then the captured one
            loss = m.trainingstep(*W.batch(r), optimiser='Adam')[0]
            fig.add("loss of step %d" % s, float(loss), r['losses'][s])
        compare_params(fig, m, r['params'][1], "after 2 steps")
        a = m.nodes['a']
        for plan in (m._grad_func.func, train_plan(m)):
            assert_routes('two_valid', flip, m, plan)
            nparts = plan.scratch.get((a, 'grad_nparts'), 1)
            print("two_valid%s: the first writer left %d parts" % ('-flip' if flip else '', nparts))
            assert nparts > 1
            assert plan.grad[a].data_ptr() == plan.scratch[a, 'grad_parts'][0].data_ptr()
            assert ('tmp', tuple(plan.grad[a].shape)) in plan.scratch           # the second writer's
        rec = route_record('two_valid', flip, m, train_plan(m))
        # (every tiling on offer splits K: the later writer fills the scratch tensor and adds)
        assert [(q[2], q[3]) for q in rec] == [('conv_valid_splitk', 'first'), ('conv_valid_splitk', 'later')]
    fig.check()


# ---- later writers share one scratch tensor ------------------------------------------------------------
@pytest.mark.parametrize("name,flip", [('cat_copy', True), ('residual', True)],
                         ids=['cat_copy-flip', 'residual-flip'])
def test_two_later_writers_one_of_which_splits_k(name, flip):
    """Two later writers of one gradient run their data gradients into the SAME scratch tensor
    (Plan.tmp_like, keyed by shape), one after the other.  With every conv GEMM pinned to
    "1,1,4,2" the 'same' conv b of cat_copy (3 filters: one K chunk) does not split K and
    overwrites the scratch tensor; the valid conv d behind it (6 filters: two chunks) splits K and
    adds onto a zero fill of its own -- which the captured step must not move to the head of the
    step, in front of b's launch.  (residual: b and d both split.)  Eager step, capture, replays."""
    from elektronn2_amd import autotune
    autotune.force('igemm', "1,1,4,2")
    try:
        m, rec = run_protocol(name, flip, "igemm 1,1,4,2")
    finally:
        autotune.force('igemm', None)
    plan = train_plan(m)
    later = [q for q in rec if q[0] == 'a' and q[3] == 'later' and q[2].startswith('conv_')]
    # cat_copy: b (3 filters, one K chunk of 4) overwrites the scratch tensor, d (6 filters, two
    # chunks) fills it and adds; residual: b (5 filters) and d (6, three depth taps) both split
    assert [(q[1], q[2]) for q in later] == ([('b[0]', 'conv_same'), ('d[0]', 'conv_valid_splitk')]
                                             if name == 'cat_copy' else
                                             [('b[0]', 'conv_same_splitk'), ('d[0]', 'conv_valid_splitk')])
    for p in (plan, m._grad_func.func):
        assert p.scratch[m.nodes['d'], 'dgrad_atomics'] is True
        assert p.scratch[m.nodes['b'], 'dgrad_atomics'] is (name == 'residual')
    assert len(later) == 2 and ('tmp', tuple(plan.grad[m.nodes['a']].shape)) in plan.scratch
    # no zero fill of the shared scratch tensor is batched at the head of a segment
    tmp = plan.scratch['tmp', tuple(plan.grad[m.nodes['a']].shape)].data_ptr()
    assert all(tmp not in ptrs for ptrs in plan._zero_batched.values())


# ---- several steps per launch ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['residual', 'unet_add'])
def test_three_steps_in_one_launch(name):
    """Model.trainingsteps(k=3) against three single steps (1e-5 losses, 1e-4 parameters: one route
    against another) and both against the reference"""
    from elektronn2_amd.neuromancer import plan_options
    r = W.reference(name)
    fig = Figures("%s trainingsteps" % name)
    with plan_options(debug_poison=True):
        single = W.build(name)
        ones = [float(single.trainingstep(*W.batch(r), optimiser='Adam')[0]) for _ in range(4)]
        ones_p = [p.get_value() for p in single.trainable_params]
        m = W.build(name)
        loss = m.trainingstep(*W.batch(r), optimiser='Adam')[0]
        fig.add("loss of step 0", float(loss), r['losses'][0])
        plan = train_plan(m)
        ring = torch.zeros(2, plan.input_arena.numel(), device=plan.ctx.device)
        for j in range(2):
            for node, src in zip(plan.inputs, W.batch(r)):
                o, cnt = plan.input_slices[node]
                assert cnt == src.size
                ring[j, o:o + cnt] = torch.tensor(src.ravel(), device=ring.device)
        losses, _ = m.trainingsteps(3, optimiser='Adam', ring=ring)
        assert len(plan._multi) == 1
        for s, l in enumerate(losses):
            fig.add("loss of step %d" % (s + 1), float(l), r['losses'][s + 1])
            fig.add("loss of step %d against the single step" % (s + 1), float(l), ones[s + 1], 1e-5)
        compare_params(fig, m, r['params'][3], "after 1 + 3 steps")
        for k, p, p0 in zip(m.loss_node.all_trainable_params.keys(), m.trainable_params, ones_p):
            fig.add("%s against four single steps" % k, p.get_value(), p0, 1e-4)
        assert_routes(name, False, m, plan)
    fig.check()


# ---- bf16 operands -------------------------------------------------------------------------------------
from test_bf16_gpu import process_bf16, _pinned          # noqa: E402,F401  (of that file, unchanged)


def _bf16_evaluation(name, ahead, calls=3):
    """test_bf16_gpu._one_evaluation for a net of wiring_cases: ``calls`` gradient evaluations (eager,
    captured, replay) with every conv launch pinned to the kernels with bf16 operands in memory"""
    from elektronn2_amd.neuromancer import plan_options
    r = W.reference(name)
    x, t = W.batch(r)
    with plan_options(bf16_ahead=ahead, bf16_ahead_min=0.0, debug_poison=True):
        m = W.build(name)
        with _pinned():
            for _ in range(calls):
                g = m.gradients(x, t)
            loss = float(m.loss(x, t))
    plan = m._grad_func.func
    torch.cuda.synchronize()
    outs = {n.name: plan.out[n].detach().cpu().numpy().copy() for n in plan.nodes if plan.out.get(n) is not None}
    douts = {n.name: plan.grad[n].detach().cpu().numpy().copy() for n in plan.nodes
             if plan.grad.get(n) is not None and type(n).__name__ == 'Conv' and n._route(plan) != 'head'}
    names = list(m.loss_node.all_trainable_params.keys())
    return dict(outs=outs, douts=douts, g=dict(zip(names, g)), loss=loss, plan=plan, model=m,
                kinds=sorted(set(k for (_, k) in plan.bf16a)))


@pytest.mark.parametrize("name", ['residual', 'two_valid'])
def test_bf16_operands_made_ahead_with_a_second_consumer(process_bf16, name):
    """the producer of a tensor writes the bf16 input image of ONE consumer, the other converts for
    itself (bf16_ahead.prepare): every node output and every Conv output gradient is bit-identical
    to the step in which every launch converts, every parameter gradient within 2e-6 (the bounds of
    test_operands_made_ahead_give_the_converting_steps_tensors)"""
    A = _bf16_evaluation(name, False)
    B = _bf16_evaluation(name, True)
    assert A['kinds'] == [] and 'fwd' in B['kinds'], (A['kinds'], B['kinds'])
    plan, n = B['plan'], B['model'].nodes
    a = n['a']
    fan = W.writers(B['model'], plan._bwd_nodes())['a']
    assert len(fan) >= 2 and 'a' in A['douts']
    if name == 'two_valid':
        assert {'fwd', 'dgrad', 'wgrad', 'dy', 'next'} <= set(B['kinds']), B['kinds']
        nx = plan.bf16a[a, 'next']['consumer']
        assert nx is n['u']                                  # (the first in the plan's order)
        assert plan.bf16a[n['u'], 'fwd']['producer'] is a
        assert plan.bf16a[n['v'], 'fwd']['producer'] is None   # the second consumer converts by itself
        assert sum(1 for (q, k) in plan.bf16a if k == 'next' and q is a) == 1
    else:
        # `a` is the fused first layer: it writes the image of ONE consumer, the valid conv d; the
        # 'same' conv b reads a framed image of its own (no entry), the conv behind the Add has no
        # producer
        assert a._route(plan) == 'first' and plan.bf16a[a, 'next']['consumer'] is n['d']
        assert plan.bf16a[n['d'], 'fwd']['producer'] is a
        assert plan.bf16a[n['c'], 'fwd']['producer'] is None
        assert (n['b'], 'fwd') not in plan.bf16a
        assert sum(1 for (q, k) in plan.bf16a if k == 'next' and q is a) == 1
    for what in ("outs", "douts"):
        assert set(A[what]) == set(B[what])
        for k in A[what]:
            u, v = A[what][k], B[what][k]
            assert np.isfinite(v).all(), (what, k)
            assert np.array_equal(u.view(np.int32), v.view(np.int32)), \
                "%s of %s: %d words differ" % (what, k, int((u.view(np.int32) != v.view(np.int32)).sum()))
    for k, ga in A['g'].items():
        d = np.abs(B['g'][k] - ga).max() / max(np.abs(ga).max(), 1e-30)
        print("%s bf16: d/d%s ahead against converting %.3g (bound 2e-06)" % (name, k, d))
        assert np.isfinite(B['g'][k]).all() and d <= 2e-6, k


@pytest.mark.parametrize("name", ['residual', 'two_valid'])
def test_bf16_mode_against_the_reference(process_bf16, name):
    """SANITY CHECK ONLY: the bf16 step against the float64 reference of the f32 net at the bf16
    bounds of the suite (loss 1e-2, gradients 1e-1 of their largest entry).  A dropped contribution
    below that bound -- the edge a -> b of `residual` moves the gradients by 2.4e-1, but a partly
    wrong sum need not -- cannot be seen here; the bit-identity test above and the f32 tests carry
    the wiring."""
    r = W.reference(name)
    fig = Figures("%s bf16" % name, W.BF16_GRAD)
    B = _bf16_evaluation(name, True, calls=2)
    fig.add("loss", B['loss'], r['loss0'], W.BF16_LOSS)
    assert abs(B['loss'] - r['loss0']) > 1e-7 * abs(r['loss0'])         # not the f32 path
    for (k, g), g0 in zip(B['g'].items(), r['grads0']):
        fig.add("d/d%s" % k, g, g0)
    fig.check()
