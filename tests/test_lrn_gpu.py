"""LRN node on the GPU (csrc/lrn.hip: e2_lrn_fwd / e2_lrn_bwd; neural.py:2043-2181 of the reference).

The reference of every number is the float64 restatement of tests/test_lrn_host.py (``lrn_ref``,
autograd for the backward; ``LrnRef`` for whole graphs; pinned there against a literal NumPy loop
and the hand-derived backward) -- never the code under test.  Bounds are the project's own, as in
tests/test_pool_modes_gpu.py: ops 2e-5 of the reference's largest magnitude; loss, prediction and
every gradient of a step 1e-4; parameters after Adam steps 5e-4.  The op inputs are x = 2 randn,
g = randn with alpha = 0.7, k = 1.5, beta = 0.75 (tests/test_lrn_host.py shows that a window one
short moves the reference by more than 100 times the op bound there)."""
import numpy as np
import pytest
import torch

from test_dropout_gpu import VIEWS
from test_lrn_host import (ADAM, ALPHA, BETA, K, NET_CASES, NET_IDS, NEW_PARAMS, OP_CONFIGS, OP_IDS,
                           OP_SHAPES, LrnRef, batch_for, lrn_nodes, lrn_ref, net_chain, op_case,
                           sharpen, _finish)

pytestmark = pytest.mark.gpu
TOL = 2e-5
TOL_STEP = 1e-4
TOL_PARAM = 5e-4


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device='cuda')


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def scalars(alpha=ALPHA, k=K, beta=BETA):
    return dev([alpha]), dev([k]), dev([beta])


def f3(mode, f):
    return tuple(f) if mode == 'spatial' else (f, 1, 1)


# ---- A. the ops through the C ABI ------------------------------------------------------------------
def _filled(make, shape, value, data=None):
    """(storage, view, copy of the storage, mask of the storage outside the view)"""
    store, view = make(shape)
    store.fill_(0); view.fill_(1)
    outside = store == 0
    store.fill_(value)
    if data is not None:
        view.copy_(dev(data))
    return store, view, store.clone(), outside


@pytest.mark.parametrize("mixed", [False, True], ids=["same_views", "mixed_views"])
@pytest.mark.parametrize("view", range(len(VIEWS)), ids=[v[0] for v in VIEWS])
@pytest.mark.parametrize("mode,f", OP_CONFIGS, ids=OP_IDS)
def test_fwd_and_bwd_through_the_c_abi(ctx, mode, f, view, mixed):
    """x, dout (and q, as the backward reads it) in one kind of view, out / q / tmp / dx in the
    same kind or -- ``mixed`` -- the next one, so that the alignments of source and destination
    rows differ"""
    rd = VIEWS[view][1]
    wr = VIEWS[(view + 1) % len(VIEWS)][1] if mixed else rd
    al, k, be = scalars()
    win = f3(mode, f)
    for shape in OP_SHAPES:
        x, g, ref_out, ref_q, ref_dx = op_case(shape, mode, f)
        what = (mode, f, shape)
        xs, xv, xb, _ = _filled(rd, shape, -77.0, x)
        # ---- forward, q kept
        os_, ov, ob, o_out = _filled(wr, shape, -55.0)
        qs, qv, qb, q_out = _filled(wr, shape, -33.0)
        ctx.lrn_fwd(xv, mode, win, al, k, be, ov, q=qv)
        got, got_q = ov.cpu().numpy(), qv.cpu().numpy()
        e_o, e_q = rel(got, ref_out), rel(got_q, ref_q)
        print(what, "out %.2e q %.2e" % (e_o, e_q))
        assert e_o < TOL and e_q < TOL, (what, e_o, e_q)
        assert torch.equal(xs, xb), what                                     # x is only read
        assert torch.equal(os_[o_out], ob[o_out]) and torch.equal(qs[q_out], qb[q_out]), what
        # ---- again into fresh storage, and without q: the same bits
        _, ov2, _, _ = _filled(wr, shape, 3.0)
        _, qv2, _, _ = _filled(wr, shape, 4.0)
        ctx.lrn_fwd(xv, mode, win, al, k, be, ov2, q=qv2)
        assert np.array_equal(bits(ov2.cpu().numpy()), bits(got)), what
        assert np.array_equal(bits(qv2.cpu().numpy()), bits(got_q)), what
        _, ov3, _, _ = _filled(wr, shape, 5.0)
        ctx.lrn_fwd(xv, mode, win, al, k, be, ov3)
        assert np.array_equal(bits(ov3.cpu().numpy()), bits(got)), what
        # ---- backward: dout and q in source views, tmp and dx in destination views
        gs, gv, gb, _ = _filled(rd, shape, -77.0, g)
        q2s, q2v, q2b, _ = _filled(rd, shape, -11.0, got_q)
        ts, tv, tb, t_out = _filled(wr, shape, -22.0)
        ds, dv, db, d_out = _filled(wr, shape, -55.0)
        ctx.lrn_bwd(gv, xv, q2v, mode, win, al, be, tv, dv)
        gdx = dv.cpu().numpy()
        e_d = rel(gdx, ref_dx)
        print(what, "dx %.2e" % e_d)
        assert e_d < TOL, (what, e_d)
        for s, b in ((xs, xb), (gs, gb), (q2s, q2b)):
            assert torch.equal(s, b), what
        assert torch.equal(ts[t_out], tb[t_out]) and torch.equal(ds[d_out], db[d_out]), what
        _, tv2, _, _ = _filled(wr, shape, 6.0)
        _, dv2, _, _ = _filled(wr, shape, 7.0)
        ctx.lrn_bwd(gv, xv, q2v, mode, win, al, be, tv2, dv2)
        assert np.array_equal(bits(dv2.cpu().numpy()), bits(gdx)), what
        # ---- accumulate: dx = base + gradient
        base = np.random.RandomState(3).randn(*shape).astype(np.float32)
        dv.copy_(dev(base))
        db = ds.clone()
        ctx.lrn_bwd(gv, xv, q2v, mode, win, al, be, tv, dv, accumulate=True)
        e_a = rel(dv.cpu().numpy(), base.astype(np.float64) + ref_dx)
        assert e_a < TOL, (what, e_a)
        assert torch.equal(ds[d_out], db[d_out]), what
        assert np.array_equal(bits(dv.cpu().numpy()), bits(base + gdx)), what  # a plain read-add-write


def test_the_kernels_read_alpha_k_beta_when_they_run(ctx):
    shape, mode, f = OP_SHAPES[0], 'spatial', (1, 3, 3)
    x, g, _, _, _ = op_case(shape, mode, f)
    al, k, be = scalars()
    xv, gv = dev(x), dev(g)
    out, q, tmp, dx = (torch.empty(shape, device='cuda') for _ in range(4))
    for vals in ((ALPHA, K, BETA), (1e-4, 1.0, 0.75), (2.0, 0.5, 1.25)):
        for t, v in zip((al, k, be), vals):
            t.fill_(v)                                   # the same device words, new contents
        ctx.lrn_fwd(xv, mode, f, al, k, be, out, q=q)
        ctx.lrn_bwd(gv, xv, q, mode, f, al, be, tmp, dx)
        from test_lrn_host import lrn_ref_fwd_bwd
        ro, rq, rd = lrn_ref_fwd_bwd(x, g, f, mode, *[float(np.float32(v)) for v in vals])
        assert rel(out.cpu().numpy(), ro) < TOL and rel(q.cpu().numpy(), rq) < TOL, vals
        assert rel(dx.cpu().numpy(), rd) < TOL, vals


def test_rejected_arguments_name_the_entry_point(ctx):
    from elektronn2_amd import backend
    al, k, be = scalars()
    sh = (1, 2, 4, 6, 8)
    x, g, q, tmp, out, dx = (torch.zeros(sh, device='cuda') for _ in range(6))
    ctx.lrn_fwd(x, 'spatial', (1, 3, 3), al, k, be, out, q=q)
    ctx.lrn_bwd(g, x, q, 'spatial', (1, 3, 3), al, be, tmp, dx)
    fwd = lambda mode, win, o=out, qq=q: ctx.lrn_fwd(x, mode, win, al, k, be, o, q=qq)
    bwd = lambda mode, win, d=dx, t=tmp, qq=q: ctx.lrn_bwd(g, x, qq, mode, win, al, be, t, d)
    for other in ((1, 2, 4, 6, 7), (1, 2, 4, 5, 8), (1, 2, 3, 6, 8), (1, 3, 4, 6, 8), (2, 2, 4, 6, 8)):
        o = torch.zeros(other, device='cuda')
        with pytest.raises(backend.E2Error, match="e2_lrn_fwd"):             # sizes do not match
            fwd('spatial', (1, 3, 3), o=o)
        with pytest.raises(backend.E2Error, match="e2_lrn_fwd"):
            fwd('spatial', (1, 3, 3), qq=o)
        with pytest.raises(backend.E2Error, match="e2_lrn_bwd"):
            bwd('spatial', (1, 3, 3), d=o)
        with pytest.raises(backend.E2Error, match="e2_lrn_bwd"):
            bwd('spatial', (1, 3, 3), t=o)
        with pytest.raises(backend.E2Error, match="e2_lrn_bwd"):
            bwd('spatial', (1, 3, 3), qq=o)
    for name, call in (("e2_lrn_fwd", fwd), ("e2_lrn_bwd", bwd)):
        for win in ((1, 2, 3), (2, 3, 3), (1, 3, 4), (1, 0, 3), (1, 3, -1)):
            with pytest.raises(backend.E2Error, match=name):                 # an even or < 1 extent
                call('spatial', win)
        for win in ((2, 1, 1), (0, 1, 1), (3, 3, 1), (3, 1, 3)):
            with pytest.raises(backend.E2Error, match=name):                 # channel: odd fz, fy = fx = 1
                call('channel', win)
        for bad in (2, -1, 7):
            with pytest.raises(backend.E2Error, match=name):                 # a mode outside the enum
                call(bad, (1, 3, 3))
    with pytest.raises(backend.E2Error, match="e2_lrn_fwd"):                 # out aliasing x
        fwd('spatial', (1, 3, 3), o=x)
    with pytest.raises(backend.E2Error, match="e2_lrn_bwd"):                 # dx aliasing dout
        bwd('spatial', (1, 3, 3), d=g)
    with pytest.raises(backend.E2Error, match="e2_lrn_bwd"):                 # tmp aliasing dx
        bwd('channel', (3, 1, 1), t=dx)


# ---- B. small nets ---------------------------------------------------------------------------------
def check_loss_and_grads(m, x, t, what=""):
    """loss, every parameter gradient and the gradient with respect to every LRN's parent"""
    ref = LrnRef(m)
    lref, pref = ref.loss_and_grads(x, t)
    loss = float(m.loss(x, t))
    e_l = abs(loss - lref) / abs(lref)
    got = m.gradients(x, t)
    names = list(m.loss_node.all_trainable_params.keys())
    want = ref.grads()
    assert len(got) == len(want) == len(names)
    errs = dict((nme, rel(g, w)) for nme, g, w in zip(names, got, want))
    plan = m._grad_func.func
    for node, w in ref.lrn_parent_grads().items():
        g = plan.user_view(node.parent, plan.grad[node.parent]).cpu().numpy()
        if any(type(c).__name__ == 'Pool' and c.mode == 'max' for c in node.parent.children.values()):
            # a max Pool beside the LRN decides: among the exact zeros a relu parent puts into one
            # window the kernel hands the gradient to every tied maximum, autograd to the first
            # (tests/test_pool_modes_gpu.py).  Compared where the parent's relu lets a gradient
            # through, which is all of the gradient that goes on; the LRN's share is there in full.
            live = ref.val[node.parent].detach().numpy() != 0
            g, w = g * live, w * live
        assert np.abs(w).max() > 0, node.name
        errs["d(%s)" % node.parent.name] = rel(g, w)
    print("%s: loss %.7f ref %.7f (%.1e); gradients worst %s"
          % (what, loss, lref, e_l, sorted(errs.items(), key=lambda kv: -kv[1])[:3]))
    assert e_l < TOL_STEP, (loss, lref)
    for nme, w in zip(names, want):
        assert np.abs(w).max() > 0, nme
    for nme, e in errs.items():
        assert e < TOL_STEP, (nme, e)
    return ref


@pytest.mark.parametrize("name,make,ncls,batch,data_seed", NET_CASES, ids=NET_IDS)
def test_whole_steps_against_float64(name, make, ncls, batch, data_seed):
    """loss, prediction, every parameter gradient and every LRN parent's gradient (eager, captured,
    replayed), then loss and parameters over 3 Adam steps (eager, captured, replayed step graph)"""
    m = make(batch=batch)
    x, t = batch_for(m, data_seed, ncls)
    assert lrn_nodes(m)
    ref = None
    for call in range(3):
        ref = check_loss_and_grads(m, x, t, "%s call %d" % (name, call))
        e = rel(m.predict(x), ref.predict(x))
        print("%s call %d: prediction %.2e" % (name, call, e))
        assert e < TOL_STEP
    for step in range(3):
        lref, _ = ref.loss_and_grads(x, t)
        ref.adam(**ADAM)
        loss = float(m.trainingstep(x, t, optimiser='Adam')[0])
        assert abs(loss - lref) / abs(lref) < TOL_STEP, (step, loss, lref)
        worst = ('', 0.0)
        for nme, p in m.loss_node.all_trainable_params.items():
            e = rel(p.get_value(), ref.p(p).detach().numpy())
            worst = max(worst, (nme, e), key=lambda kv: kv[1])
            assert e < TOL_PARAM, (step, nme, e)
        print("%s step %d: loss %.7f ref %.7f, parameters worst %s" % (name, step, loss, lref, worst))
    assert m.optimisers['Adam'].step.func.use_graph
    # the nodes' own outputs, as ops on what their parents produced on the device
    for node in lrn_nodes(m):
        src, got = node.parent(x), node(x)
        want = lrn_ref(torch.tensor(src.astype(np.float64)), node.filter_shape, node.mode,
                       *[float(node.params[k].get_value()) for k in ('alpha', 'k', 'beta')]).numpy()
        assert rel(got, want) < TOL, node.name


def test_set_value_reaches_a_captured_step_without_a_new_capture():
    """net (a) under a sharpened head (tests/test_lrn_host.py: the loss then moves by more than
    100 times the bound when the parameters change): three steps (eager, captured, replayed), new
    alpha / k / beta on both nodes, and the next REPLAYED step has the float64 loss of the new
    values; the graphs are the ones captured before"""
    m = net_chain()
    sharpen(m)
    x, t = batch_for(m, 62)
    ref = LrnRef(m)
    for step in range(3):
        lref, _ = ref.loss_and_grads(x, t)
        ref.adam(**ADAM)
        loss = float(m.trainingstep(x, t, optimiser='Adam')[0])
        assert abs(loss - lref) / abs(lref) < TOL_STEP, (step, loss, lref)
    plan = m.optimisers['Adam'].step.func
    assert plan.use_graph and plan._graphs
    graphs = list(plan._graphs)
    stale, _ = ref.loss_and_grads(x, t)
    for node, (al, k, be) in zip(lrn_nodes(m), NEW_PARAMS):
        node.alpha.set_value(al); node.k.set_value(k); node.beta.set_value(be)
        ref.set_params(node)
    lref, _ = ref.loss_and_grads(x, t)
    assert abs(stale - lref) / abs(lref) > 100 * TOL_STEP, (stale, lref)
    loss = float(m.trainingstep(x, t, optimiser='Adam')[0])
    print("after set_value: loss %.7f ref %.7f (with the old values %.7f)" % (loss, lref, stale))
    assert abs(loss - lref) / abs(lref) < TOL_STEP, (loss, lref, stale)
    assert list(plan._graphs) == graphs                                      # no new capture
    assert [float(n.alpha.get_value()) for n in lrn_nodes(m)] == [float(np.float32(p[0])) for p in NEW_PARAMS]


# ---- C. plan behaviour -----------------------------------------------------------------------------
def _steps(m, x, t, n=3):
    losses = [float(m.trainingstep(x, t, optimiser='Adam')[0]) for _ in range(n)]
    return losses, [p.get_value() for p in m.loss_node.all_trainable_params.values()]


def test_graph_replay_equals_eager():
    """net (a).  Bit for bit where the arithmetic of a step does not depend on the order in which
    work-groups arrive -- the prediction and both LRN outputs of a REPLAYED evaluation against an
    eager one (the LRN launches themselves are order-free: test A compares their bits run to run).
    The loss is a sum over work-groups and the parameters after Adam steps pass through the conv
    kernels' bias and weight gradients, all added up with float atomics: they differ in the last
    bit now and then whatever the route (measured here: the loss of one evaluation 0.69194990
    against 0.69194996, one ulp; of four training steps the losses 1 to 3 equal in every bit, loss
    4 one ulp apart), so those are compared at the bound the other route tests use (losses 1e-5,
    parameters 1e-4)."""
    from elektronn2_amd.neuromancer import plan_options
    res, fwd = {}, {}
    for graph in (True, False):
        with plan_options(graph=graph):
            m = net_chain()
            x, t = batch_for(m, 62)
            for _ in range(3):                               # eager, captured, replayed
                fwd[graph] = [np.float32(m.loss(x, t)), m.predict(x)] + [n(x) for n in lrn_nodes(m)]
            assert m.loss_node._output_func.func.use_graph == graph
            res[graph] = _steps(m, x, t, 4)
            assert m.optimisers['Adam'].step.func.use_graph == graph
    assert abs(fwd[True][0] - fwd[False][0]) < 1e-5 * abs(fwd[False][0])
    for u, v in zip(fwd[True][1:], fwd[False][1:]):
        assert np.array_equal(bits(u), bits(v))
    print("losses", res[True][0], res[False][0])
    for u, v in zip(res[True][0], res[False][0]):
        assert abs(u - v) < 1e-5 * abs(v), (res[True][0], res[False][0])
    for u, v in zip(res[True][1], res[False][1]):
        assert rel(u, v) < 1e-4


def test_several_steps_in_one_graph_equal_single_steps():
    m0 = net_chain()
    x, t = batch_for(m0, 62)

    def fresh():
        mm = net_chain()
        for _ in range(2):
            mm.trainingstep(x, t, optimiser='Adam')
        return mm
    a = fresh()
    single = [float(a.trainingstep(x, t, optimiser='Adam')[0]) for _ in range(3)]
    b = fresh()
    pl = b.optimisers['Adam'].step.func
    ring = torch.empty((3, pl.input_arena.numel()), device='cuda')
    ring[:] = pl.input_arena
    losses, tsec = b.trainingsteps(3, optimiser='Adam', ring=ring)
    assert len(losses) == 3
    for u, v in zip(single, losses):
        assert abs(u - float(v)) / abs(u) < 1e-5, (single, list(losses))
    for pa, pb in zip(a.loss_node.all_trainable_params.values(), b.loss_node.all_trainable_params.values()):
        assert rel(pb.get_value(), pa.get_value()) < 1e-4


def test_checkpoint_after_two_steps_resumes_to_the_same_third_step(tmp_path):
    from elektronn2_amd import neuromancer as nm
    a = net_chain()
    a.nodes['lrn_c'].k.set_value(1.25)
    x, t = batch_for(a, 62)
    for _ in range(2):
        a.trainingstep(x, t, optimiser='Adam')
    f = str(tmp_path / "lrn.mdl")
    a.save(f)
    pred = a.predict(x)
    third = float(a.trainingstep(x, t, optimiser='Adam')[0])
    b = nm.modelload(f, name='reloaded')
    b.set_opt_meta_params('Adam', ADAM)
    describe = lambda mm: [(n.mode, n.filter_shape, [float(n.params[k].get_value()) for k in ('alpha', 'k', 'beta')])
                           for n in lrn_nodes(mm)]
    assert describe(b) == describe(a)
    assert describe(b)[1][2][1] == 1.25 and isinstance(describe(b)[0][1], tuple)
    assert np.array_equal(bits(b.predict(x)), bits(pred))
    got = float(b.trainingstep(x, t, optimiser='Adam')[0])
    print("third step %.9g, resumed %.9g" % (third, got))
    assert np.array_equal(bits([got]), bits([third])), (got, third)


# one eager Adam step of net (a) WITHOUT its two LRN nodes, batch 2: the entry points in the order
# of issue, recorded with the tree as it was before the LRN node existed; the node must not change
# it.  (A conv launch whose tuned tiling splits K hands partial sums to the `_parts` form of the
# pass behind it; which layers do depends on the tuner's timings, so the suffix is dropped.)
LAUNCHES_WITHOUT_LRN = [
    'e2_ctx_set_stream', 'e2_conv3d_pack_multi_ex', 'e2_conv1_pool_act_fwd', 'e2_conv3d_fwd_packed',
    'e2_pool_bias_act_fwd', 'e2_conv3d_fwd_packed', 'e2_pool_bias_act_fwd', 'e2_fill', 'e2_head_fwd',
    'e2_head_bwd', 'e2_pool_bias_act_bwd', 'e2_conv3d_wgrad_pad', 'e2_conv3d_dgrad_packed',
    'e2_pool_bias_act_bwd', 'e2_conv3d_wgrad_pad', 'e2_conv3d_dgrad_packed', 'e2_conv1_pool_act_bwd',
    'e2_adam_step_ex', 'e2_ctx_set_stream']


def _entry_points_of_one_eager_step(m, x, t, monkeypatch):
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
        assert m.optimisers['Adam'].step.func.use_graph is False
    skip = ('e2_event', 'e2_stream', 'e2_last_launch', 'e2_set_', 'e2_conv_last_zero_fill')
    return [c[:-len('_parts')] if c.endswith('_parts') else c for c in calls if not c.startswith(skip)]


def test_routes_with_and_without_the_nodes(monkeypatch):
    """without LRN nodes net (a) issues the launches it issued before the node existed; with them
    every Conv next to an LRN runs the launches that materialise its output and read its output
    gradient, and the LRN launches are one forward and one backward call per node"""
    plain = net_chain(lrn=False)
    x, t = batch_for(plain, 62)
    got = _entry_points_of_one_eager_step(plain, x, t, monkeypatch)
    print("launches without LRN:", got)
    assert not any('lrn' in c for c in got)
    assert got == LAUNCHES_WITHOUT_LRN
    m = net_chain()
    with_lrn = _entry_points_of_one_eager_step(m, x, t, monkeypatch)
    print("launches with LRN:", with_lrn)
    assert with_lrn.count('e2_lrn_fwd') == 2 and with_lrn.count('e2_lrn_bwd') == 2
    rest = [c for c in with_lrn if 'lrn' not in c]
    plan = m.optimisers['Adam'].step.func
    convs = dict((n.name, n) for n in plan.nodes if type(n).__name__ == 'Conv')
    for name in ('c0', 'c1', 'c2'):
        n = convs[name]
        assert plan.out[n] is not None and n in plan.grad, name
        assert n._tail(plan) is None and n._fused_head(plan) is None, name
        assert not n._actbwd_into_parent(plan), name
        assert (n, 'next') not in plan.bf16a, name
    for node in lrn_nodes(m):
        assert plan.out[node].is_contiguous() and (node, 'q') in plan.scratch and (node, 'tmp') in plan.scratch
        # the parent's gradient slabs (if it has any) are written as ONE plain gradient
        assert plan.scratch.get((node.parent, 'grad_nparts'), 1) == 1
    assert convs['head']._fused_head(plan) is not None
    # a prediction plan keeps no q and hands the kernel none
    m.prediction_node(x)
    pplan = m.prediction_node._output_func.func
    assert not pplan.training
    for node in lrn_nodes(m):
        assert (node, 'q') not in pplan.scratch and (node, 'tmp') not in pplan.scratch
    assert len(rest) >= len(got)


@pytest.fixture()
def process_bf16():
    import elektronn2_amd
    elektronn2_amd.set_mfma_dtype('bf16')
    yield
    elektronn2_amd.set_mfma_dtype('f32')


def test_bf16_mode_leaves_the_lrn_launches_in_f32(process_bf16):
    """local to the layer, at the op bound (the bound of the bf16 test of the activation pair,
    which also compares layer by layer on the tensors the pass produced): each LRN's output is the
    float64 restatement of the output its parent produced on the device -- bf16 rounding upstream
    does not enter; the steps run and stay finite"""
    m = net_chain()
    x, t = batch_for(m, 62)
    for node in lrn_nodes(m):
        src, got = node.parent(x), node(x)
        want = lrn_ref(torch.tensor(src.astype(np.float64)), node.filter_shape, node.mode,
                       float(np.float32(ALPHA)), K, BETA).numpy()
        e = rel(got, want)
        print("bf16 mode, %s (%s): %.2e" % (node.name, node.mode, e))
        assert e < TOL, (node.name, e)
    losses = [float(m.trainingstep(x, t, optimiser='Adam')[0]) for _ in range(3)]
    assert np.isfinite(losses).all()
    plan = m.optimisers['Adam'].step.func
    for node in lrn_nodes(m):
        g = plan.grad[node.parent]
        assert torch.isfinite(g).all()
    # the backward of one node on the tensors of that step, against float64 at the op bound
    torch.cuda.synchronize()
    for node in lrn_nodes(m):
        xin = plan.out[node.parent].detach().cpu().numpy().astype(np.float64)
        gout = plan.grad[node].detach().cpu().numpy().astype(np.float64)
        xt = torch.tensor(xin, requires_grad=True)
        lrn_ref(xt, node.filter_shape, node.mode, float(np.float32(ALPHA)), K, BETA).backward(torch.tensor(gout))
        if len(node.parent.children) == 1:                # (the LRN is the gradient's only writer)
            e = rel(plan.grad[node.parent].detach().cpu().numpy(), xt.grad.numpy())
            print("bf16 mode, d(%s): %.2e" % (node.parent.name, e))
            assert e < TOL, (node.name, e)


def test_predict_dense_through_a_channel_mode_net_equals_one_pass():
    """the channel mode is pointwise in space: tiles and stride offsets go through it unchanged"""
    from elektronn2_amd import neuromancer as nm
    # (net (a) with its spatial node taken out: a spatial LRN is refused, tests/test_lrn_host.py)
    nm.model_manager.reset()
    np.random.seed(74)
    inp = nm.Input((None, 1, 6, 22, 22), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 6, (1, 3, 3), name='c0')
    out = nm.Conv(out, 8, (1, 3, 3), (1, 2, 2), name='c1')
    out = nm.LRN(out, 3, mode='channel', name='lrn_c', alpha=ALPHA, k=K, beta=BETA)
    out = nm.Conv(out, 8, (3, 3, 3), name='c2')
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin', name='head')
    m = _finish(nm, inp, out)
    fov = tuple(int(v) for v in m.prediction_node.shape.fov)
    strides = tuple(int(v) for v in m.prediction_node.shape.strides)
    assert strides == (1, 2, 2)
    rng = np.random.RandomState(6)
    raw = rng.rand(1, 9, 31, 29).astype(np.float32)
    got = m.predict_dense(raw)
    off = tuple(int(v) for v in m.prediction_node.shape.offsets)
    assert got.shape == (2,) + tuple(s - 2 * o for s, o in zip(raw.shape[1:], off))
    ref = LrnRef(m)
    for (z, a, b) in [(0, 0, 0), (5, 19, 17), (3, 7, 11), (4, 1, 16), (2, 13, 4)]:
        patch = raw[None, :, z:z + fov[0], a:a + fov[1], b:b + fov[2]]
        want = ref.predict(patch)
        assert want.shape == (1, 2, 1, 1, 1)
        assert np.abs(got[:, z, a, b] - want[0, :, 0, 0, 0]).max() < 1e-4, (z, a, b)
    # ... and the one-pass prediction of a whole patch: output voxel (i, j, k) is the dense voxel
    # (i, 2 j, 2 k) from the patch's origin
    for (z, a, b) in [(0, 0, 0), (2, 5, 4)]:
        one = m.predict(raw[None, :, z:z + 6, a:a + 22, b:b + 22])
        assert one.shape == (1, 2, 4, 7, 7)
        assert np.abs(got[:, z:z + 4, a:a + 14:2, b:b + 14:2] - one[0]).max() < 1e-4, (z, a, b)
