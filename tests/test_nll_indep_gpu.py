"""MultinoulliNLL over several independent softmaxes on the GPU: the one-launch kernels
e2_softmax_nll_grouped_fwd / _bwd (csrc/softmax_nll.hip) through the C ABI, and nets whose last
layer is ``Softmax(n_indep=E)`` under ``MultinoulliNLL(target_is_sparse=True)``.

The reference of every comparison is the float64 loop restatement of the contract in
tests/test_nll_indep_host.py (pinned there to oracle.e2_oracle.nll_loss_and_grad for E = 1), on
the float32 inputs the kernels saw.  Bounds are the project's own for the same quantities:
tests/test_ops_gpu.py::test_softmax_nll for the ops (probabilities 1e-6, loss 1e-5, dlogits 1e-5
of the largest magnitude, count within 0.5); tests/test_model_gpu.py for whole steps (loss,
prediction and gradients 1e-4, parameters after Adam steps 5e-4; graph against eager, a ring
against single steps: losses 1e-5, parameters 1e-4); tests/test_checkpoint.py for a resumed run;
tests/test_bf16_gpu.py for a small net's bf16 loss (1e-2)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_activations_gpu import Ref, ADAM
from test_nll_indep_host import grouped_nll, grouped_errors, EPS
from test_unet_config5_gpu import small_unet

pytestmark = pytest.mark.gpu
TOL = 1e-4          # tests/test_model_gpu.py:17
TOL_ADAM = 5e-4     # tests/test_model_gpu.py:22

# (n, E*k, d, h, w), E, k: S = 399 and 1310 -- several work-groups with a ragged last one, a w that
# is neither a multiple of 4 nor of 64
SHAPES = [((2, 6, 3, 7, 19), 3, 2), ((1, 6, 2, 5, 131), 2, 3)]
SHAPE_IDS = ["E3k2_S399", "E2k3_S1310"]


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


def inputs(shape, E, k, seed):
    """logits randn * 3; class ids with planted runs of -1 in two groups"""
    rng = np.random.RandomState(seed)
    n, f, d, h, w = shape
    lg = (rng.randn(*shape) * 3).astype(np.float32)
    tg = rng.randint(0, k, (n, E, d, h, w)).astype(np.float32)
    tg[0, 0, 0, 0, :3] = -1
    tg[n - 1, E - 1, d - 1, 1:3, 5:17] = -1
    return lg, tg


_REF = {}


def reference(shape, E, k, seed=15):
    """(lg, tg, restatement) -- computed once per case, shared, never written to"""
    key = (shape, E, k, seed)
    if key not in _REF:
        lg, tg = inputs(shape, E, k, seed)
        for a in (lg, tg):
            a.setflags(write=False)
        _REF[key] = (lg, tg, grouped_nll(lg, tg, E))
    return _REF[key]


def run_grouped(ctx, lg, tg, E, alias=False):
    """forward + backward on fresh contiguous buffers -> (probs, stats, dlogits, loss)"""
    lgd, tgd = dev(lg), dev(tg)
    probs = torch.full(lg.shape, float("nan"), device="cuda")
    stats = torch.zeros(2, device="cuda")
    ctx.softmax_nll_grouped_fwd(lgd, tgd, probs, E, stats)
    p_out = probs.clone()
    dl = probs if alias else torch.full(lg.shape, float("nan"), device="cuda")
    loss = torch.full((1,), float("nan"), device="cuda")
    ctx.softmax_nll_grouped_bwd(probs, tgd, E, stats, dl, loss)
    torch.cuda.synchronize()
    return p_out, stats, dl, loss


def check_against(p, stats, dl, loss, want):
    loss_ref, dl_ref, p_ref, n_lab, loss_sum = want
    print("probs %.2e, dlogits %.2e, loss %.8f ref %.8f, count %s ref %d"
          % (relerr(p, p_ref), relerr(dl, dl_ref), float(loss), loss_ref, float(stats[1]), n_lab))
    assert relerr(p, p_ref) < 1e-6
    assert abs(float(loss) - loss_ref) / loss_ref < 1e-5
    assert abs(float(stats[0]) - loss_sum) / loss_sum < 1e-5
    assert relerr(dl, dl_ref) < 1e-5
    assert abs(float(stats[1]) - n_lab) < 0.5


# ---- 1. the kernels through the C ABI ------------------------------------------------------------
@pytest.mark.parametrize("shape,E,k", SHAPES, ids=SHAPE_IDS)
def test_ops_against_the_float64_restatement(ctx, shape, E, k):
    lg, tg, want = reference(shape, E, k)
    check_against(*run_grouped(ctx, lg, tg, E), want)


@pytest.mark.parametrize("shape,E,k", SHAPES, ids=SHAPE_IDS)
def test_strided_views_and_untouched_surroundings(ctx, shape, E, k):
    """logits / dlogits: channels 2:8 of 10-channel buffers; the target: a channel, row and column
    window of a wider buffer; probabilities into a window of a padded buffer.  Everything outside
    the output views is NaN before and after."""
    lg, tg, want = reference(shape, E, k)
    n, f, d, h, w = shape
    nan = float("nan")
    lbuf = torch.full((n, 10, d, h, w), nan, device="cuda")
    lbuf[:, 2:8] = dev(lg)
    tbuf = torch.full((n, E + 2, d, h + 1, w + 5), nan, device="cuda")
    tv = tbuf[:, 1:1 + E, :, 1:, 2:2 + w]
    tv.copy_(dev(tg))
    pbuf = torch.full((n, f, d, h + 2, w + 3), nan, device="cuda")
    pv = pbuf[:, :, :, 1:1 + h, 3:]
    dbuf = torch.full((n, 10, d, h, w), nan, device="cuda")
    stats = torch.zeros(2, device="cuda")
    loss = torch.zeros(1, device="cuda")
    lcopy, tcopy = lbuf.clone(), tbuf.clone()
    ctx.softmax_nll_grouped_fwd(lbuf[:, 2:8], tv, pv, E, stats)
    ctx.softmax_nll_grouped_bwd(pv, tv, E, stats, dbuf[:, 2:8], loss)
    torch.cuda.synchronize()
    check_against(pv, stats, dbuf[:, 2:8], loss, want)
    # inputs unchanged (bit patterns: NaN included), output surroundings still NaN
    assert np.array_equal(bits(lbuf), bits(lcopy)) and np.array_equal(bits(tbuf), bits(tcopy))
    outside = torch.ones_like(pbuf, dtype=torch.bool)
    outside[:, :, :, 1:1 + h, 3:] = False
    assert bool(torch.isnan(pbuf[outside]).all()) and not bool(torch.isnan(pv).any())
    assert bool(torch.isnan(dbuf[:, :2]).all()) and bool(torch.isnan(dbuf[:, 8:]).all())
    assert not bool(torch.isnan(dbuf[:, 2:8]).any())
    # the same bits as the dense call
    p0, _, dl0, _ = run_grouped(ctx, lg, tg, E)
    assert np.array_equal(bits(pv), bits(p0)) and np.array_equal(bits(dbuf[:, 2:8]), bits(dl0))


@pytest.mark.parametrize("shape,E,k", SHAPES, ids=SHAPE_IDS)
def test_corners(ctx, shape, E, k):
    lg, tg0, _ = reference(shape, E, k)
    # one whole group unlabelled: exact zeros there, the rest over the remaining count
    tg = tg0.copy()
    tg[:, 1] = -1
    want = grouped_nll(lg, tg, E)
    p, stats, dl, loss = run_grouped(ctx, lg, tg, E)
    check_against(p, stats, dl, loss, want)
    assert want[3] == int((tg >= 0).sum()) < int((tg0 >= 0).sum())
    assert not host(dl)[:, k:2 * k].any()
    # ids >= k and non-integers are ignored
    tg = tg0.copy()
    tg[0, 0, 0, 1, :4] = k
    tg[0, E - 1, 0, 2, :4] = 0.5
    tg[0, 0, 0, 3, :2] = k + 40
    tg[0, 0, 0, 4, :2] = 1e-3
    want = grouped_nll(lg, tg, E)
    assert want[3] == int((tg0 >= 0).sum()) - 12
    p, stats, dl, loss = run_grouped(ctx, lg, tg, E)
    check_against(p, stats, dl, loss, want)
    assert not host(dl)[0, :k, 0, 1, :4].any() and not host(dl)[0, (E - 1) * k:, 0, 2, :4].any()
    # everything unlabelled: loss 0, every dlogit 0 and finite
    p, stats, dl, loss = run_grouped(ctx, lg, np.full_like(tg0, -1), E)
    assert float(loss) == 0.0 and float(stats[0]) == 0.0 and float(stats[1]) == 0.0
    assert bool(torch.isfinite(dl).all()) and not host(dl).any()
    assert relerr(p, grouped_nll(lg, tg0, E)[2]) < 1e-6


@pytest.mark.parametrize("shape,E,k", SHAPES, ids=SHAPE_IDS)
def test_dlogits_may_alias_probs_and_a_null_target_gives_probabilities_only(ctx, shape, E, k):
    lg, tg, want = reference(shape, E, k)
    p0, s0, dl0, loss0 = run_grouped(ctx, lg, tg, E)
    p1, s1, dl1, loss1 = run_grouped(ctx, lg, tg, E, alias=True)
    assert np.array_equal(bits(p0), bits(p1)) and np.array_equal(bits(dl0), bits(dl1))
    assert close(loss1, loss0, 1e-6)
    # target None: the same probabilities, stats untouched (or absent)
    probs = torch.full(lg.shape, float("nan"), device="cuda")
    stats = dev([3.5, 7.25])
    ctx.softmax_nll_grouped_fwd(dev(lg), None, probs, E, stats)
    torch.cuda.synchronize()
    assert np.array_equal(bits(probs), bits(p0))
    assert host(stats).tolist() == [3.5, 7.25]
    probs2 = torch.full(lg.shape, float("nan"), device="cuda")
    ctx.softmax_nll_grouped_fwd(dev(lg), None, probs2, E, None)
    torch.cuda.synchronize()
    assert np.array_equal(bits(probs2), bits(p0))


@pytest.mark.parametrize("shape,E,k", SHAPES, ids=SHAPE_IDS)
def test_agreement_with_the_per_slice_kernels(ctx, shape, E, k):
    """E launches of e2_softmax_nll_fwd into ONE stats buffer, then E launches of
    e2_softmax_nll_bwd that read it -- the kernels every n_indep = 1 net runs.  Loss and count are
    sums of atomics (to the tolerances of the op test); the grouped kernels compile the same
    per-thread body (softmax_nll_{fwd,bwd}_body.hpp) with the same flags and the count is an exact
    integer in float32, so probabilities and dlogits must be bit-equal."""
    lg, tg, want = reference(shape, E, k)
    lgd, tgd = dev(lg), dev(tg)
    probs = torch.full(lg.shape, float("nan"), device="cuda")
    dl = torch.full(lg.shape, float("nan"), device="cuda")
    stats = torch.zeros(2, device="cuda")
    loss = torch.zeros(1, device="cuda")
    for g in range(E):
        sl = slice(g * k, (g + 1) * k)
        ctx.softmax_nll_fwd(lgd[:, sl], tgd[:, g:g + 1], probs[:, sl], stats)
    for g in range(E):
        sl = slice(g * k, (g + 1) * k)
        ctx.softmax_nll_bwd(probs[:, sl], tgd[:, g:g + 1], stats, dl[:, sl], loss)
    torch.cuda.synchronize()
    p1, s1, dl1, loss1 = run_grouped(ctx, lg, tg, E)
    print("loss %.8f per-slice %.8f; count %s / %s" % (float(loss1), float(loss), float(s1[1]), float(stats[1])))
    assert close(loss1, loss, 1e-5) and close(s1[0], stats[0], 1e-5)
    assert abs(float(s1[1]) - float(stats[1])) < 0.5
    assert np.array_equal(bits(p1), bits(probs))
    assert np.array_equal(bits(dl1), bits(dl))


def test_sum_mode_leaves_the_gradient_unnormalised_and_reports_the_count(ctx):
    shape, E, k = SHAPES[0]
    lg, tg, want = reference(shape, E, k)
    n_lab = want[3]
    p0, s0, dl0, loss0 = run_grouped(ctx, lg, tg, E)
    count = torch.full((1,), float("nan"), device="cuda")
    ctx.set_loss_grad_mode(True, count)
    try:
        p1, s1, dl1, loss1 = run_grouped(ctx, lg, tg, E)
    finally:
        ctx.set_loss_grad_mode(False, None)
    assert float(count) == float(n_lab)
    assert relerr(dl1, host(dl0).astype(np.float64) * (np.float64(np.float32(n_lab)) + EPS)) < 1e-5
    assert relerr(dl1, want[1] * (n_lab + EPS)) < 1e-5
    assert close(loss1, loss0, 1e-6)                       # (loss values are unaffected)
    # the mode is restored: normalised again, the count slot is left alone
    count.fill_(-3.0)
    p2, s2, dl2, loss2 = run_grouped(ctx, lg, tg, E)
    assert np.array_equal(bits(dl2), bits(dl0)) and float(count) == -3.0


def test_bad_arguments_are_errors_that_launch_nothing(ctx):
    from elektronn2_amd import backend
    shape, E, k = SHAPES[0]
    lg, tg, _ = reference(shape, E, k)
    n, f, d, h, w = shape
    lgd, tgd = dev(lg), dev(tg)
    out = torch.full(shape, 7.0, device="cuda")
    stats = torch.zeros(2, device="cuda")
    loss = torch.full((1,), 7.0, device="cuda")
    good_p = torch.rand(shape, device="cuda")
    bad_fwd = [(lgd, tgd, out, 4),                              # 6 % 4 != 0
               (lgd, tgd[:, :2], out, 3),                       # target.c != n_indep
               (lgd, tgd, out, 2),                              # (6 % 2 == 0, but target.c = 3)
               (lgd, tgd, out, 0), (lgd, tgd, out, -1),         # n_indep < 1
               (lgd, tgd[:, :, :, :, :w - 1], out, 3),          # spatial extents
               (lgd, tgd[:1], out, 3),                          # batch extent
               (lgd, tgd, out[:, :, :d - 1], 3),
               (lgd[:, :4], tgd, out, 2)]                       # probs / logits features
    for a in bad_fwd:
        with pytest.raises(backend.E2Error):
            ctx.softmax_nll_grouped_fwd(a[0], a[1], a[2], a[3], stats)
    bad_bwd = [(good_p, tgd, 4, out), (good_p, tgd[:, :2], 3, out), (good_p, tgd, 2, out),
               (good_p, tgd, 0, out), (good_p, tgd[:, :, :, :h - 1], 3, out), (good_p, tgd[:1], 3, out),
               (good_p, tgd, 3, out[:, :4])]
    for a in bad_bwd:
        with pytest.raises(backend.E2Error):
            ctx.softmax_nll_grouped_bwd(a[0], a[1], a[2], stats, a[3], loss)
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0 and float(loss) == 7.0
    assert not host(stats).any()


# ---- 2. nets ---------------------------------------------------------------------------------------
class RefG(Ref):
    """tests/test_activations_gpu.py's float64 restatement of a graph up to the logits; the loss and
    its gradient with respect to the logits come from tests/test_nll_indep_host.py's loop."""

    def logits(self, x):
        m = self.model
        self.min_pre, self.n_kinked = np.inf, 0
        val = {}
        sm = m.prediction_node
        for node in m.nodes.values():
            kind = type(node).__name__
            par = node.parent
            if node is m.input_node:
                val[node] = torch.tensor(np.asarray(x, np.float64))
            elif kind in ('Conv', 'UpConv'):
                h, w, b = val[par], self.p(node.w), self.p(node.b)
                if kind == 'UpConv':
                    y = F.conv_transpose3d(h, w.permute(1, 0, 2, 3, 4), stride=tuple(node.pool_shape))
                else:
                    y = F.conv3d(h, w.flip(2, 3, 4))
                    if any(q != 1 for q in node.pool_shape):
                        y = F.max_pool3d(y, tuple(node.pool_shape))
                assert not node.batch_normalisation
                val[node] = self.act(node, y + b.view(1, -1, 1, 1, 1))
            elif kind == 'Pool':
                val[node] = F.max_pool3d(val[par], tuple(node.pool_shape))
            elif kind == 'Crop':
                val[node] = val[par][node._slicer()]
            elif kind == 'Concat':
                val[node] = torch.cat([val[q] for q in par], dim=1)
            elif node is sm:
                return val[par]
        raise AssertionError("no Softmax node")

    def loss_and_grads(self, x, t):
        for v in self.P.values():
            v.grad = None
        lg = self.logits(x)
        assert self.min_pre >= 1e-6, "ill-posed case: a kinked unit at %.1e" % self.min_pre
        loss, dl, probs, n_lab, _ = grouped_nll(lg.detach().numpy(), t, self.model.prediction_node.n_indep)
        lg.backward(torch.tensor(dl))
        self.n_lab = n_lab
        return loss, probs


def _finish(nm, inp, probs):
    target = nm.Input_like(probs, override_f=probs.n_indep, name='target')
    nll = nm.MultinoulliNLL(probs, target, target_is_sparse=True, name='nll')
    loss = nm.AggregateLoss(nll, name='loss')
    errors = nm.Errors(probs, target, target_is_sparse=True)
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss,
                          prediction_node=probs, prediction_ext=[loss, errors, probs])
    model.set_opt_meta_params('Adam', ADAM)
    return model


def net_convs(batch=1, seed=71):
    """a pooled first layer, a (3,3,3) conv, a 6-feature 'lin' head: three 2-class softmaxes.
    (x, y = 26: a (1,3,3) conv in front of a (1,2,2) pool needs an even extent behind the conv;
    the output is (7, 10, 10), 700 positions per item and group -- three work-groups, the last
    one ragged)"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(seed)
    inp = nm.Input((batch, 1, 9, 26, 26), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 8, (1, 3, 3), (1, 2, 2))
    out = nm.Conv(out, 8, (3, 3, 3))
    out = nm.Conv(out, 6, (1, 1, 1), activation_func='lin', name='head')
    return _finish(nm, inp, nm.Softmax(out, n_indep=3))


def net_unet(batch=1, seed=72):
    """the small U-Net of tests/test_unet_config5_gpu.py with n_out = 6, n_indep = 3"""
    np.random.seed(seed)
    nm, inp, probs = small_unet((6, 22, 22), n_out=6, batch=batch, n_indep=3)
    return _finish(nm, inp, probs)


def batch_for(m, seed):
    rng = np.random.RandomState(seed)
    x = rng.rand(*m.input_node.shape.shape).astype(np.float32)
    t = rng.randint(0, m.prediction_node.n_class, m.target_node.shape.shape).astype(np.float32)
    t.flat[::17] = -1                      # unlabelled voxels
    t[0, 1, 0] = -1                        # and a plane of one group
    return x, t


def rel(a, b):
    return relerr(np.asarray(a), b)


# name, constructor, batch, seed of the batch (chosen on the reference alone: RefG's assertion)
NETS = [("convs_b1", net_convs, 1, 81), ("convs_b2", net_convs, 2, 81), ("unet", net_unet, 1, 131)]


@pytest.mark.parametrize("name,make,batch,data_seed", NETS, ids=[n[0] for n in NETS])
def test_loss_gradients_errors_and_adam_steps_against_float64(name, make, batch, data_seed):
    """loss, prediction, Errors, EVERY parameter gradient -- eager, captured and replayed calls --
    and three Adam steps (eager, captured, replayed) against the float64 step"""
    m = make(batch)
    assert m.prediction_node.n_indep == 3 and m.loss_node.parent[0].n_indep == 3
    x, t = batch_for(m, data_seed)
    ref = RefG(m)
    for call in range(3):                                   # eager, capture, replay
        lref, pref = ref.loss_and_grads(x, t)
        loss = float(m.loss(x, t))
        print("%s call %d: loss %.7f ref %.7f (kinked closest %.1e, %d labelled)"
              % (name, call, loss, lref, ref.min_pre, ref.n_lab))
        assert close(loss, lref, TOL), (call, loss, lref)
        assert rel(m.predict(x), pref) < TOL
        l2, err, pr = m.predict_ext(x, t)
        assert close(l2, lref, TOL) and rel(pr, pref) < TOL
        assert abs(float(err) - grouped_errors(pr, t, 3)) < 1e-6
        margin = np.sort(pref.reshape(batch, 3, 2, -1), axis=2)
        if (margin[:, :, 1] - margin[:, :, 0]).min() > 1e-3:        # (no argmax near a tie)
            assert abs(float(err) - grouped_errors(pref, t, 3)) < 1e-6
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
        lref, _ = ref.loss_and_grads(x, t)
        ref.adam(**ADAM)
        loss = float(m.trainingstep(x, t, optimiser='Adam')[0])
        assert close(loss, lref, TOL), (step, loss, lref)
        worst = ('', 0.0)
        for nme, p in m.loss_node.all_trainable_params.items():
            e = rel(p.get_value(), ref.p(p).detach().numpy())
            worst = max(worst, (nme, e), key=lambda kv: kv[1])
            assert e < TOL_ADAM, (step, nme, e)
        print("%s step %d: loss %.7f ref %.7f, parameters worst %s" % (name, step, loss, lref, worst))
    plan = m.optimisers['Adam'].step.func
    assert plan._graphs, "the step was not captured"
    stats = plan.scratch[m.prediction_node, 'stats']
    assert abs(float(stats[1]) - ref.n_lab) < 0.5
    # the loss took the grouped pair, in one launch each: no fused head, no per-group loop
    assert m.prediction_node._head(plan) is None


# ---- 3. the model protocol -------------------------------------------------------------------------
def _batches(m, n, seed=90):
    return [batch_for(m, seed + i) for i in range(n)]


def _params(m):
    return [p.get_value() for p in m.loss_node.all_trainable_params.values()]


def test_graph_replay_equals_eager_for_three_steps():
    runs = []
    for use_graph in (True, False):
        m = net_convs()
        bs = _batches(m, 3)
        opt = m.optimisers['Adam']
        opt.step.compile()
        opt.step.func.use_graph = use_graph
        losses = [float(m.trainingstep(x, t, optimiser='Adam')[0]) for x, t in bs]
        assert bool(opt.step.func._graphs) == use_graph
        runs.append((losses, _params(m)))
    (lg, pg), (le, pe) = runs
    for a, b in zip(lg, le):
        assert close(a, b, 1e-5), (lg, le)
    for a, b in zip(pg, pe):
        assert rel(a, b) < 1e-4


def test_trainingsteps_from_a_ring_returns_the_losses_of_single_steps():
    a = net_convs()
    bs = _batches(a, 3)
    single = [float(a.trainingstep(*bs[i % 3], optimiser='Adam')[0]) for i in range(5)]
    c = net_convs()
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
    a = net_convs()
    x, t = batch_for(a, 81)
    for _ in range(2):
        a.trainingstep(x, t, optimiser='Adam')
    f = str(tmp_path / "indep.mdl")
    a.save(f)
    saved = _params(a)
    third = float(a.trainingstep(x, t, optimiser='Adam')[0])
    end_p = _params(a)
    b = net_convs(seed=99)                                   # other weights, nothing on the device
    modelload(f, b)
    for v, p in zip(saved, _params(b)):
        assert np.array_equal(v, p)                          # bit-equal
    got = float(b.trainingstep(x, t, optimiser='Adam')[0])
    assert close(got, third, 2e-6), (third, got)             # tests/test_checkpoint.py:171-185
    for v, p in zip(end_p, _params(b)):
        assert np.abs(v - p).max() <= 1e-5 * np.abs(v).max()
    c = modelload(f)                                         # the graph rebuilt from the file alone
    assert c.prediction_node.n_indep == 3 and c.loss_node.parent[0].n_indep == 3
    b2 = net_convs(seed=98)
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
    m = net_convs()
    x, t = batch_for(m, 81)
    lref, _ = RefG(m).loss_and_grads(x, t)
    loss = float(m.trainingstep(x, t, optimiser='Adam')[0])
    print("bf16 loss %.7f, float64 of the f32 net %.7f" % (loss, lref))
    assert np.isfinite(loss) and abs(loss - lref) < 1e-2 * abs(lref)


def test_sampler_feeds_an_affinity_step():
    """getbatch(affinities='affinity') -> (images, aff (b, E, z, x, y)): the sparse target of this
    loss as it is; the labelled count is the number of affinities >= 0"""
    from elektronn2_amd.data import PatchSampler
    nhood = np.array([[-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.int32)
    m = net_unet()                         # (stride 1, an odd field of view: centred targets)
    sp = tuple(m.input_node.shape.spatial_shape)
    tn = m.target_node
    osp = tuple(tn.shape.spatial_shape)
    assert osp == (2, 8, 8) and list(tn.shape.offsets) == [2, 7, 7]
    rng = np.random.RandomState(0)
    vol = rng.rand(1, 14, 40, 40).astype(np.float32)
    ids = rng.randint(0, 3, (1, 14, 40, 40)).astype(np.float32)       # a random 3-ID label cube
    smp = PatchSampler([vol], [ids], sp, tn.shape.strides, tn.shape.offsets, seed=1,
                       target_discrete_ix=[0])
    d, aff = smp.getbatch(1, 'train', affinities='affinity', nhood=nhood)
    assert d.is_cuda and tuple(aff.shape) == (1, 3) + osp
    loss = float(m.trainingstep(d, aff, optimiser='Adam')[0])
    assert np.isfinite(loss) and loss > 0
    plan = m.optimisers['Adam'].step.func
    a = host(aff)
    n_lab = int(((a >= 0) & (a < 2)).sum())
    assert n_lab == int((a >= 0).sum()) > 0
    assert abs(float(plan.scratch[m.prediction_node, 'stats'][1]) - n_lab) < 0.5
