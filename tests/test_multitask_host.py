"""Multi-task nets: several ``MultinoulliNLL`` terms, each over a ``Softmax`` of its own, under one
``AggregateLoss`` (reference loss.py:261-347 per term, 1357-1363 for the mix), and ``nm.split``
(reference node_basic.py:1335-1398) that cuts one target Input into the terms' targets.

Here: the float64 restatement that the GPU tests (tests/test_multitask_gpu.py) compare against,
pinned to the oracle and to torch autograd; wrong variants that must fail on the very inputs the
tests use; ``split``; the forms of ``AggregateLoss``; the C ABI; the save / rebuild round trip.
No GPU."""
import numpy as np
import pytest
import torch

from oracle import e2_oracle as O

EPS = 1e-5


def multi_nll(logits_list, targets_list, w):
    """The contract in float64, as an explicit loop over (term, item, position):

        T = 1 where target_k[n, 0, pos] is an integer class id in [0, c_k), else 0
        S_k = sum_{T=1} -log(p_target + EPS)     N_k = sum T     L_k = S_k / (N_k + EPS)
        total  = (1/K) sum_k w_k L_k
        coef_k = w_k / (K (N_k + EPS))
        dlogits_k[c] = T coef_k (-p_t / (p_t + EPS)) ([c == target] - p_c)

    every term with its OWN normaliser; a term with nothing labelled has L_k = 0, a zero gradient
    and still counts in K.  -> (total, [L_k], [N_k], [probs_k], [dlogits_k], [S_k])"""
    K = len(logits_list)
    assert K == len(targets_list) == len(w)
    Ls, Ns, Ps, Ds, Ss = [], [], [], [], []
    for k in range(K):
        lg = np.asarray(logits_list[k], np.float64)
        tg = np.asarray(targets_list[k], np.float64)
        n, c = lg.shape[:2]
        assert tg.shape == (n, 1) + lg.shape[2:], (lg.shape, tg.shape)
        lg2, tg2 = lg.reshape(n, c, -1), tg.reshape(n, -1)
        probs = np.zeros_like(lg2)
        labelled, s_sum = [], 0.0
        for i in range(n):
            for s in range(lg2.shape[2]):
                z = lg2[i, :, s]
                e = np.exp(z - z.max())
                p = e / e.sum()
                probs[i, :, s] = p
                t = tg2[i, s]
                if 0 <= t < c and t == np.floor(t):
                    labelled.append((i, s, int(t)))
                    s_sum -= np.log(p[int(t)] + EPS)
        N = len(labelled)
        coef = float(w[k]) / (K * (N + EPS))
        dl = np.zeros_like(lg2)
        for i, s, t in labelled:
            p = probs[i, :, s]
            onehot = np.zeros(c)
            onehot[t] = 1.0
            dl[i, :, s] = coef * (-p[t] / (p[t] + EPS)) * (onehot - p)
        Ls.append(s_sum / (N + EPS))
        Ns.append(N)
        Ss.append(s_sum)
        Ps.append(probs.reshape(lg.shape))
        Ds.append(dl.reshape(lg.shape))
    total = sum(float(w[k]) * Ls[k] for k in range(K)) / K
    return total, Ls, Ns, Ps, Ds, Ss


def plant(tg, c, rng):
    """runs of -1, ids >= c and non-integer ids: all unlabelled"""
    flat = tg.reshape(-1)
    flat[3:11] = -1
    flat[20:23] = c
    flat[30] = c + 4
    flat[40:43] = 0.5
    flat[rng.randint(0, flat.size, flat.size // 9)] = -1
    return tg


def case_inputs(classes=(3, 4, 2), spatial=((3, 7, 19),) * 3, n=2, seed=31, empty=None, thin=1):
    """logits randn * 3 and class ids per term.  Term ``thin`` keeps a label on about one
    position in 6 (clearly another count than its neighbours); term ``empty`` has none."""
    rng = np.random.RandomState(seed)
    lgs, tgs = [], []
    for k, (c, sp) in enumerate(zip(classes, spatial)):
        lgs.append((rng.randn(n, c, *sp) * 3).astype(np.float32))
        tg = plant(rng.randint(0, c, (n, 1) + tuple(sp)).astype(np.float32), c, rng)
        if k == thin:
            tg[rng.rand(*tg.shape) > 1.0 / 6] = -1
        elif k > 0:
            tg[rng.rand(*tg.shape) < 0.15 * k] = -1
        if k == empty:
            tg[:] = -1
        tgs.append(tg)
    return lgs, tgs


W3 = np.array([2.154, 0.42, 0.42], np.float32) * 3 / np.float32(2.154 + 0.42 + 0.42)

# the inputs of the CPU comparisons: different class counts, different labelled counts, and (the
# second set) one head with nothing labelled
SMALL = dict(classes=(3, 4, 2), spatial=((1, 5, 11),) * 3, n=2, seed=33)


def relerr(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


# ---- 1. the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("empty", [None, 2])
def test_restatement_equals_the_oracle_term_by_term(empty):
    lgs, tgs = case_inputs(empty=empty, **SMALL)
    total, Ls, Ns, Ps, Ds, Ss = multi_nll(lgs, tgs, W3)
    K = 3
    assert len(set(Ns)) == 3 and (Ns[2] == 0) == (empty == 2) and Ns[1] < Ns[0] // 3
    want_total = 0.0
    for k in range(K):
        c = lgs[k].shape[1]
        t = tgs[k]
        t1 = np.where((t >= 0) & (t < c) & (t == np.floor(t)), t, -1).astype(np.float32)
        if Ns[k] == 0:
            assert Ls[k] == 0.0 and not Ds[k].any()
            continue
        loss_ref, dl_ref, p_ref = O.nll_loss_and_grad(lgs[k], t1)
        assert abs(Ls[k] - loss_ref) <= 1e-12 * abs(loss_ref)
        assert np.abs(Ps[k] - p_ref).max() <= 1e-14
        assert np.abs(Ds[k] - dl_ref * float(W3[k]) / K).max() <= 1e-12 * np.abs(dl_ref).max()
        want_total += float(W3[k]) * loss_ref
    assert abs(total - want_total / K) <= 1e-12 * abs(total)


@pytest.mark.parametrize("empty", [None, 2])
def test_restatement_equals_torch_autograd_of_the_formula(empty):
    lgs, tgs = case_inputs(empty=empty, **SMALL)
    total, Ls, Ns, Ps, Ds, _ = multi_nll(lgs, tgs, W3)
    xs = [torch.tensor(l.astype(np.float64), requires_grad=True) for l in lgs]
    tot = 0.0
    for k, x in enumerate(xs):
        c = x.shape[1]
        p = torch.softmax(x, dim=1)
        t = torch.tensor(tgs[k].astype(np.float64))
        onehot = (t == torch.arange(c, dtype=torch.float64).view(1, c, 1, 1, 1)).to(torch.float64)
        L = -(onehot * torch.log(p + EPS)).sum() / (onehot.sum() + EPS)
        assert abs(float(L.detach()) - Ls[k]) <= 1e-12 * max(abs(Ls[k]), 1e-30) and int(onehot.sum()) == Ns[k]
        tot = tot + float(W3[k]) * L
    tot = tot / 3
    tot.backward()
    assert abs(float(tot.detach()) - total) <= 1e-12 * abs(total)
    for k, x in enumerate(xs):
        assert np.abs(x.grad.numpy() - Ds[k]).max() <= 1e-12 * max(np.abs(Ds[k]).max(), 1e-30)
        if Ns[k] == 0:
            assert not x.grad.numpy().any() and np.isfinite(x.grad.numpy()).all()


def test_nothing_labelled_anywhere_is_zero_and_finite():
    lgs, tgs = case_inputs(**SMALL)
    total, Ls, Ns, _, Ds, _ = multi_nll(lgs, [np.full_like(t, -1) for t in tgs], W3)
    assert total == 0.0 and Ns == [0, 0, 0] and all(L == 0.0 for L in Ls)
    assert all(not d.any() and np.isfinite(d).all() for d in Ds)


def f32_variant(lgs, tgs, w, variant=None):
    """a vectorised float32 implementation of the contract (variant None) and of six plausible
    mistakes -> (total, [dlogits_k])"""
    f = np.float32
    K = len(lgs)
    rows = []
    for lg, tg in zip(lgs, tgs):
        c = lg.shape[1]
        e = np.exp(lg - lg.max(axis=1, keepdims=True)).astype(f)
        p = (e / e.sum(axis=1, keepdims=True)).astype(f)
        onehot = (tg == np.arange(c, dtype=f).reshape(1, c, 1, 1, 1)).astype(f)
        pt = (p * onehot).sum(axis=1, keepdims=True)
        lab = onehot.sum(axis=1, keepdims=True)
        if variant == 'eps_outside_log':
            S = f(-(lab * (np.log(np.maximum(pt, f(1e-30))) + f(EPS))).sum())
            g = -lab * (onehot - p)
        else:
            S = f(-(lab * np.log(pt + f(EPS))).sum())
            g = -lab * pt / (pt + f(EPS)) * (onehot - p)
        rows.append((S, f(lab.sum()), g.astype(f)))
    n_all = f(sum(r[1] for r in rows))
    k_eff = f(K)
    if variant == 'empty_head_dropped':
        k_eff = f(sum(1 for r in rows if r[1] > 0))
    total, dls = f(0), []
    for (S, N, g), wk in zip(rows, w):
        wk = f(1) if variant == 'weights_ignored' else f(wk)
        den = N + f(EPS)
        if variant == 'one_normaliser':
            den = n_all + f(EPS)
        if variant == 'weights_on_count':
            den = wk * N + f(EPS)
            wk = f(1)
        scale = wk / den if variant == 'missing_1_over_K' else wk / (k_eff * den)
        total += S * scale
        dls.append(g * scale)
    return total, dls


VARIANTS = ['one_normaliser', 'missing_1_over_K', 'weights_ignored', 'weights_on_count',
            'eps_outside_log', 'empty_head_dropped']


def passes(lgs, tgs, w, variant):
    """the comparison of the GPU op tests: loss 1e-5, dlogits 1e-5 of the largest magnitude"""
    total, _, _, _, Ds, _ = multi_nll(lgs, tgs, w)
    got, dls = f32_variant(lgs, tgs, w, variant)
    ok = abs(float(got) - total) <= 1e-5 * abs(total)
    return ok and all(relerr(d, r) < 1e-5 for d, r in zip(dls, Ds) if np.abs(r).max() > 0)


def test_the_float32_form_passes_and_six_wrong_variants_fail_on_these_inputs():
    full = case_inputs(**SMALL)
    with_empty = case_inputs(empty=2, **SMALL)
    assert passes(*full, W3, None) and passes(*with_empty, W3, None)
    for v in VARIANTS:
        inputs = with_empty if v == 'empty_head_dropped' else full
        assert not passes(*inputs, W3, v), v
    # the GPU shapes too (tests/test_multitask_gpu.py builds its references from case_inputs)
    gpu = case_inputs()
    assert passes(*gpu, W3, None)
    for v in VARIANTS[:5]:
        assert not passes(*gpu, W3, v), v
    assert not passes(*case_inputs(empty=0), W3, 'empty_head_dropped')


# ---- 2. split ----------------------------------------------------------------------------------------
def three_head_net(batch=None, classes=(3, 4, 3), weights=W3, sp=(9, 26, 26), names=None):
    """one trunk, len(classes) (1,1,1) 'lin' heads with a Softmax and a sparse NLL each, one target
    Input split along 'f', the Concat of the softmaxes as prediction, Errors on head 0"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(7)
    K = len(classes)
    inp = nm.Input((batch, 1) + tuple(sp), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 8, (1, 3, 3), (1, 2, 2))
    out = nm.Conv(out, 8, (3, 3, 3))
    sms = [nm.Softmax(nm.Conv(out, c, (1, 1, 1), activation_func='lin', name='head%d' % k),
                      name='probs%d' % k) for k, c in enumerate(classes)]
    target = nm.Input_like(sms[0], override_f=K, name='target')
    parts = nm.split(target, 'f', n_out=K, name=names if names is not None else 'split')
    nlls = [nm.MultinoulliNLL(s, t, target_is_sparse=True, name='nll%d' % k)
            for k, (s, t) in enumerate(zip(sms, parts))]
    loss = nm.AggregateLoss(nlls, mixing_weights=weights, name='loss')
    pred = nm.Concat(sms, name='pred')
    errors = nm.Errors(sms[0], parts[0], target_is_sparse=True)
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=pred,
                          prediction_ext=[loss, errors, pred])
    return model, nlls, sms, parts


def test_split_parts_are_views_of_the_unsplit_target():
    m, nlls, sms, parts = three_head_net()
    assert [p.name for p in parts] == ['split', 'split1', 'split2']
    assert all(type(p).__name__ == 'SplitPart' and not p.is_source for p in parts)
    assert [(p.lo, p.hi) for p in parts] == [(0, 1), (1, 2), (2, 3)]
    for p in parts:
        assert p.shape.shape == [None, 1, 7, 10, 10] and tuple(p.shape.tags) == ('b', 'f', 'z', 'x', 'y')
        assert p.parent is m.target_node and p.computational_cost == 0
    assert m.target_node.shape.shape == [None, 3, 7, 10, 10]
    assert [n.name for n in m.loss_node.input_nodes] == ['raw', 'target']
    assert m.prediction_node.shape.shape == [None, 10, 7, 10, 10]
    _, _, _, named = three_head_net(names=['barrier', 'object', 'myelin'])
    assert [p.name for p in named] == ['barrier', 'object', 'myelin']


def test_split_index_and_n_out_forms_and_errors():
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    t = nm.Input((2, 6, 4, 5, 5), 'b,f,z,x,y', name='t')
    a = nm.split(t, n_out=3)
    assert [(p.lo, p.hi) for p in a] == [(0, 2), (2, 4), (4, 6)] and a[1].shape['f'] == 2
    b = nm.split(t, 'f', index=[1, 4], name=['x1', 'x2', 'x3'])
    assert [(p.lo, p.hi) for p in b] == [(0, 1), (1, 4), (4, 6)] and b[1].shape.shape == [2, 3, 4, 5, 5]
    c = nm.split(t, index=2)
    assert [(p.lo, p.hi) for p in c] == [(0, 2), (2, 6)]
    assert isinstance(a, tuple)
    with pytest.raises(ValueError):
        nm.split(t, axis='s', n_out=2)                  # an axis the shape does not have
    with pytest.raises(ValueError):
        nm.split(t, n_out=4)                            # 6 % 4
    with pytest.raises(ValueError):
        nm.split(t, index=[2, 6])                       # past the axis
    with pytest.raises(NotImplementedError, match="feature axis"):
        nm.split(t, axis='x', n_out=5)
    with pytest.raises(NotImplementedError, match="strip_singleton_dims"):
        nm.split(t, n_out=6, strip_singleton_dims=True)


# ---- 3. AggregateLoss ------------------------------------------------------------------------------
def test_the_new_form_is_recognised_and_the_weights_are_a_frozen_parameter():
    m, nlls, sms, parts = three_head_net()
    agg = m.loss_node
    assert agg.multi_nll and not agg.elementwise and list(agg.parent) == nlls
    mw = agg.params['mixing_weights']
    assert not mw.apply_train and np.allclose(mw.get_value(), W3)
    assert 'loss_mixing_weights' in m.nontrainable_params
    assert all(n.term_value is None and n.n_labelled is None for n in nlls)
    from elektronn2_amd import neuromancer as nm
    assert nm.AggregateLoss(nlls[:2]).multi_nll                       # default weights
    assert not nm.AggregateLoss(nlls[0]).multi_nll                    # the single form is untouched


def test_every_other_list_with_an_nll_still_raises_as_before():
    from elektronn2_amd import neuromancer as nm
    m, nlls, sms, parts = three_head_net(batch=1)
    trunk = sms[0].parent.parent
    se = nm.SquaredLoss(sms[0].parent, nm.Input_like(sms[0].parent, name='tr'))
    weighted = nm.MultinoulliNLL(sms[1], parts[1], target_is_sparse=True, class_weights=[1, 2, 3, 4])
    again = nm.MultinoulliNLL(sms[0], parts[0], target_is_sparse=True)       # a softmax used twice
    sm6 = nm.Softmax(nm.Conv(trunk, 6, (1, 1, 1), activation_func='lin'), n_indep=3)
    indep = nm.MultinoulliNLL(sm6, nm.Input_like(sm6, override_f=3, name='t3'), target_is_sparse=True)
    sm2 = nm.Softmax(nm.Conv(trunk, 6, (1, 1, 1), activation_func='lin'), n_indep=3, n_class=2)
    malis = nm.MalisNLL(sm2, nm.Input_like(sm2, override_f=3, name='aff'),
                        nm.Input_like(sm2, override_f=1, name='seg'),
                        nhood=np.eye(3, dtype=np.int32))
    for terms in ([nlls[0], se], [nlls[0], nlls[0]], [nlls[0], weighted], [nlls[0], indep],
                  [nlls[0], malis], [nlls[0], again]):
        with pytest.raises(NotImplementedError, match="take no scale"):
            nm.AggregateLoss(terms)
    nine = nlls + [nm.MultinoulliNLL(
        nm.Softmax(nm.Conv(trunk, 2, (1, 1, 1), activation_func='lin')), parts[0],
        target_is_sparse=True) for _ in range(6)]
    assert nm.AggregateLoss(nine[:8]).multi_nll
    with pytest.raises(NotImplementedError, match="take no scale"):
        nm.AggregateLoss(nine)


# ---- 4. the C ABI and the graph description --------------------------------------------------------------
def test_c_abi_declares_exports_and_binds_the_new_entry_points():
    import ctypes
    import os
    import __graft_entry__ as g
    from test_cabi import declared_symbols
    g.build()
    from elektronn2_amd import backend
    lib = ctypes.CDLL(os.path.join(g.ROOT, "elektronn2_amd", "libe2hip.so"))
    for s in ('e2_nll_multi_fwd', 'e2_nll_mix', 'e2_nll_multi_bwd', 'e2_multihead_supported',
              'e2_multihead_fwd', 'e2_multihead_bwd_workspace_bytes', 'e2_multihead_bwd'):
        assert s in declared_symbols(), s
        assert hasattr(lib, s), s
        assert s in backend.EXPORTED_SYMBOLS, s
    for f in ('nll_multi_fwd', 'nll_mix', 'nll_multi_bwd', 'multihead_supported', 'multihead_fwd',
              'multihead_bwd_ws_bytes', 'multihead_bwd'):
        assert callable(getattr(backend.Context, f))
    header = open(os.path.join(g.ROOT, "include", "e2hip.h")).read()
    assert "coef_j = w_j / (K (N_j + 1e-5))" in header            # the contract text
    assert "sum ncls_j <= 16" in header
    # the support predicate runs on the host
    ok = backend.Context.multihead_supported
    assert ok(37, (3, 4, 3)) and ok(64, (2, 2)) and ok(300, (4,) * 4) and ok(200, (2,) * 8) and ok(512, (8, 8))
    assert not ok(64, (9, 8)) and not ok(64, (2,) * 9) and not ok(513, (2, 2)) and not ok(64, (3, 1))
    assert not ok(64, (4,)) and not ok(0, (2, 2))
    assert backend.Context.multihead_bwd_ws_bytes((2, 37, 3, 7, 13), 10) == 4 * 18 * (10 * 37 + 10)


def test_fuse_multihead_is_a_plan_option_and_on_by_default():
    from elektronn2_amd.neuromancer import options
    assert options.SPEC['fuse_multihead'][0] == 'E2_FUSE_MULTIHEAD'
    assert options.snapshot()['fuse_multihead'] is True
    assert options.snapshot(dict(fuse_multihead=False))['fuse_multihead'] is False
    with options.plan_options(fuse_multihead=False):
        assert options.snapshot()['fuse_multihead'] is False


def test_a_three_head_graph_round_trips_through_save_and_rebuild(tmp_path):
    from elektronn2_amd.neuromancer.model import modelload
    w = [1.5, 0.25, 1.25]
    m, nlls, sms, parts = three_head_net(batch=1, weights=w)
    f = str(tmp_path / "multi.mdl")
    m.save(f)
    m2 = modelload(f, name='rebuilt_multi')
    assert list(m2.nodes.keys()) == list(m.nodes.keys())
    for name, node in m.nodes.items():
        assert type(m2.nodes[name]) is type(node) and m2.nodes[name].shape.shape == node.shape.shape
    agg = m2.loss_node
    assert agg.multi_nll and [n.name for n in agg.parent] == ['nll0', 'nll1', 'nll2']
    assert np.array_equal(agg.params['mixing_weights'].get_value(), np.array(w, np.float32))
    for p, q in zip(parts, [m2.nodes[p.name] for p in parts]):
        assert type(q).__name__ == 'SplitPart' and (q.lo, q.hi) == (p.lo, p.hi)
        assert q.parent is m2.target_node
    assert type(m2.prediction_node).__name__ == 'Concat'
    assert [p.name for p in m2.prediction_node.parent] == [s.name for s in sms]
    assert [n.name for n in m2.loss_node.input_nodes] == ['raw', 'target']
    for (ka, pa), (kb, pb) in zip(m.loss_node.all_trainable_params.items(),
                                  m2.loss_node.all_trainable_params.items()):
        assert ka == kb and np.array_equal(pa.get_value(), pb.get_value())
