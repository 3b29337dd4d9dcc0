"""MultinoulliNLL over several independent softmaxes -- ``Softmax(parent, n_indep=E)`` under
``MultinoulliNLL(..., target_is_sparse=True)`` (reference loss.py:82-92, 275-285, 338-346):
construction, the shape check, the combinations that stay rejected, the C ABI, the graph
description round trip, and the float64 restatement of the contract that the GPU tests
(tests/test_nll_indep_gpu.py) compare against.  No GPU."""
import numpy as np
import pytest

from oracle import e2_oracle as O

EPS = 1e-5


def grouped_nll(logits, target, n_indep):
    """The contract in float64, as an explicit loop over (item, group, position):

        T = 1 where target[n, g, pos] is an integer class id in [0, k), else 0
        loss = sum_{T=1} -log(p[n, g*k + target, pos] + EPS) / (sum T + EPS)      (ONE count)
        dlogit[n, g*k + c, pos] = T * (-1/(n_lab + EPS) * p_t/(p_t + EPS)) * ([c == target] - p_c)

    with p the softmax INSIDE group g.  -> (loss, dlogits, probs, n_lab, loss_sum)"""
    lg = np.asarray(logits, np.float64)
    tg = np.asarray(target, np.float64)
    N, F = lg.shape[:2]
    E = int(n_indep)
    assert F % E == 0 and tg.shape == (N, E) + lg.shape[2:], (lg.shape, tg.shape, E)
    k = F // E
    lg2, tg2 = lg.reshape(N, F, -1), tg.reshape(N, E, -1)
    S = lg2.shape[2]
    probs = np.zeros_like(lg2)
    labelled = []                                   # (n, g, pos, class)
    loss_sum = 0.0
    for n in range(N):
        for g in range(E):
            for s in range(S):
                z = lg2[n, g * k:(g + 1) * k, s]
                e = np.exp(z - z.max())
                p = e / e.sum()
                probs[n, g * k:(g + 1) * k, s] = p
                t = tg2[n, g, s]
                if 0 <= t < k and t == np.floor(t):
                    c = int(t)
                    labelled.append((n, g, s, c))
                    loss_sum -= np.log(p[c] + EPS)
    n_lab = len(labelled)
    dl = np.zeros_like(lg2)
    for n, g, s, c in labelled:
        p = probs[n, g * k:(g + 1) * k, s]
        coef = -1.0 / (n_lab + EPS) * p[c] / (p[c] + EPS)
        onehot = np.zeros(k)
        onehot[c] = 1.0
        dl[n, g * k:(g + 1) * k, s] = coef * (onehot - p)
    return (loss_sum / (n_lab + EPS), dl.reshape(lg.shape), probs.reshape(lg.shape), n_lab,
            loss_sum)


def grouped_errors(probs, target, n_indep):
    """Errors for n_indep > 1 (loss.py:737-748, 789-814): the argmax inside each group against
    int16(target), mean over (item, group, position)"""
    p = np.asarray(probs)
    N, F = p.shape[:2]
    k = F // n_indep
    cls = p.reshape((N, n_indep, k) + p.shape[2:]).argmax(axis=2)
    return float(np.mean(cls != np.asarray(target).astype(np.int16)))


def indep_net(E, k, batch=None, sp=(5, 18, 18), target_shape=None, **nll_kw):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    inp = nm.Input((batch, 1) + sp, 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 6, (1, 3, 3))
    out = nm.Conv(out, E * k, (1, 1, 1), activation_func='lin', name='head')
    probs = nm.Softmax(out, n_indep=E)
    if target_shape is None:
        target = nm.Input_like(probs, override_f=E, name='target')
    else:
        target = nm.Input(target_shape, 'b,f,z,x,y', name='target')
    kw = {key: (v(probs) if callable(v) else v) for key, v in nll_kw.items()}
    sparse = kw.pop('target_is_sparse', True)
    nll = nm.MultinoulliNLL(probs, target, target_is_sparse=sparse, **kw)
    loss = nm.AggregateLoss(nll, name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss,
                          prediction_node=probs)
    return model, nll, probs


@pytest.mark.parametrize("E,k", [(3, 2), (2, 3)])
def test_construction_under_an_aggregate_loss(E, k):
    """(on the code before this feature: NotImplementedError)"""
    m, nll, probs = indep_net(E, k)
    assert (probs.n_indep, probs.n_class) == (E, k) and (nll.n_indep, nll.n_class) == (E, k)
    assert probs.shape.shape == [None, E * k, 5, 16, 16]
    assert m.target_node.shape.shape == [None, E, 5, 16, 16]
    assert nll.shape.shape == [None, 1, 5, 16, 16]
    assert not nll.weighted and not m.loss_node.elementwise
    assert [n.name for n in m.loss_node.input_nodes] == ['raw', 'target']
    m, nll, _ = indep_net(E, k, batch=2)
    assert m.target_node.shape.shape == [2, E, 5, 16, 16]


@pytest.mark.parametrize("bad", [(None, 1, 5, 16, 16), (None, 6, 5, 16, 16), (None, 3, 5, 16, 15),
                                 (None, 3, 4, 16, 16), (2, 3, 5, 16, 16)])
def test_wrong_target_shape_is_a_value_error_that_names_both_shapes(bad):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    inp = nm.Input((None, 1, 5, 18, 18), 'b,f,z,x,y', name='raw')
    probs = nm.Softmax(nm.Conv(inp, 6, (1, 3, 3), activation_func='lin'), n_indep=3)
    target = nm.Input(bad, 'b,f,z,x,y', name='target')
    with pytest.raises(ValueError) as e:
        nm.MultinoulliNLL(probs, target, target_is_sparse=True)
    msg = str(e.value)
    assert str(probs.shape) in msg and str(target.shape) in msg, msg
    with pytest.raises(ValueError):                          # no feature axis at all
        nm.MultinoulliNLL(probs, nm.Input((None, 5, 16, 16), 'b,z,x,y', name='t'),
                          target_is_sparse=True)


def _mask(name):
    def make(probs):
        from elektronn2_amd import neuromancer as nm
        return nm.Input((probs.shape['b'], probs.n_class), 'b,f', name=name)
    return make


def _example_w(probs):
    from elektronn2_amd import neuromancer as nm
    sh = [s for s, t in zip(probs.shape.shape, probs.shape.tags) if t != 'f']
    return nm.Input(sh, 'b,z,x,y', name='ew')


def _class_w_node(probs):
    from elektronn2_amd import neuromancer as nm
    return nm.Input((probs.n_class,), 'f', name='cw')


@pytest.mark.parametrize("kw", [dict(class_weights=[1.0, 2.0]),
                                dict(class_weights=_class_w_node),
                                dict(example_weights=_example_w),
                                dict(mask_class_labeled=_mask('ll')),
                                dict(mask_class_not_present=_mask('np'))],
                         ids=['class_weights', 'class_weights_node', 'example_weights',
                              'mask_class_labeled', 'mask_class_not_present'])
def test_weights_and_masks_stay_rejected_for_n_indep(kw):
    with pytest.raises(NotImplementedError) as e:
        indep_net(3, 2, **kw)
    assert 'n_indep' in str(e.value)


def test_dense_targets_and_weak_training_stay_rejected():
    with pytest.raises(NotImplementedError) as e:
        indep_net(3, 2, target_is_sparse=False)
    assert 'dense' in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        indep_net(3, 2, weakness=0.1)
    assert 'weak' in str(e.value)
    # and n_indep = 1 keeps accepting its weights
    from test_weighted_nll_host import _net
    _, nll, _ = _net(class_weights=[1.0, 4.0])
    assert nll.weighted and nll.n_indep == 1


def test_c_abi_declares_exports_and_binds_the_grouped_pair():
    import ctypes
    import os
    import __graft_entry__ as g
    from test_cabi import declared_symbols
    g.build()
    from elektronn2_amd import backend
    lib = ctypes.CDLL(os.path.join(g.ROOT, "elektronn2_amd", "libe2hip.so"))
    for s in ('e2_softmax_nll_grouped_fwd', 'e2_softmax_nll_grouped_bwd'):
        assert s in declared_symbols(), s
        assert hasattr(lib, s), s
        assert s in backend.EXPORTED_SYMBOLS, s
    assert callable(backend.Context.softmax_nll_grouped_fwd)
    assert callable(backend.Context.softmax_nll_grouped_bwd)


def test_serialise_rebuild_keeps_the_graph(tmp_path):
    from elektronn2_amd.neuromancer.model import modelload
    m, nll, probs = indep_net(3, 2, batch=1)
    d = m.serialise()
    sm = [n for n in d['nodes'] if n[0] == probs.name][0]
    assert sm[3].get('n_indep') == 3 or 3 in sm[2], sm
    f = str(tmp_path / "indep.mdl")
    m.save(f)
    m2 = modelload(f, name='rebuilt')
    assert list(m2.nodes.keys()) == list(m.nodes.keys())
    nll2 = m2.nodes[nll.name]
    assert type(nll2).__name__ == 'MultinoulliNLL' and (nll2.n_indep, nll2.n_class) == (3, 2)
    assert m2.nodes[probs.name].n_indep == 3
    assert m2.target_node.shape.shape == [1, 3, 5, 16, 16]
    assert [n.name for n in m2.loss_node.input_nodes] == ['raw', 'target']
    for (ka, pa), (kb, pb) in zip(m.loss_node.all_trainable_params.items(),
                                  m2.loss_node.all_trainable_params.items()):
        assert ka == kb and np.array_equal(pa.get_value(), pb.get_value())


def test_restatement_equals_the_oracle_for_one_group():
    """E = 1 is the loss the project already trusts (oracle.e2_oracle.nll_loss_and_grad)"""
    rng = np.random.RandomState(5)
    lg = (rng.randn(2, 3, 2, 4, 5) * 3).astype(np.float32)
    tg = rng.randint(0, 3, (2, 1, 2, 4, 5)).astype(np.float32)
    tg[0, 0, 0, 0, :3] = -1
    loss_ref, dl_ref, p_ref = O.nll_loss_and_grad(lg, tg)
    loss, dl, p, n_lab, _ = grouped_nll(lg, tg, 1)
    assert n_lab == int((tg >= 0).sum())
    assert abs(loss - loss_ref) <= 1e-12 * abs(loss_ref)
    assert np.abs(p - p_ref).max() <= 1e-14
    assert np.abs(dl - dl_ref).max() <= 1e-12 * np.abs(dl_ref).max()


def test_restatement_has_one_normaliser_and_ignores_what_is_not_a_class_id():
    rng = np.random.RandomState(6)
    E, k = 3, 2
    lg = (rng.randn(1, E * k, 1, 3, 4) * 2).astype(np.float32)
    tg = rng.randint(0, k, (1, E, 1, 3, 4)).astype(np.float32)
    tg[0, 1] = -1                                            # a whole group unlabelled
    tg[0, 0, 0, 0, 0], tg[0, 0, 0, 0, 1], tg[0, 2, 0, 0, 0] = k, 0.5, 7.0
    loss, dl, p, n_lab, loss_sum = grouped_nll(lg, tg, E)
    assert n_lab == 2 * 12 - 3
    assert np.all(dl[0, 2:4] == 0) and np.all(dl[0, 0:2, 0, 0, :2] == 0) and np.all(dl[0, 4:6, 0, 0, 0] == 0)
    # every group's probabilities sum to one; the loss is the per-group sums over ONE count
    assert np.abs(p.reshape(1, E, k, -1).sum(axis=2) - 1).max() < 1e-14
    parts = 0.0
    for g in (0, 2):
        t1 = np.where((tg[:, g:g + 1] >= 0) & (tg[:, g:g + 1] < k) & (tg[:, g:g + 1] == np.floor(tg[:, g:g + 1])),
                      tg[:, g:g + 1], -1)
        l_g, _, _, n_g, s_g = grouped_nll(lg[:, g * k:(g + 1) * k], t1, 1)
        parts += s_g
    assert abs(parts - loss_sum) < 1e-12 * abs(loss_sum)
    assert abs(loss - loss_sum / (n_lab + EPS)) < 1e-15
    # central differences of the loss agree with the stated gradient
    h = 1e-6
    for idx in [(0, 0, 0, 1, 1), (0, 5, 0, 2, 3), (0, 3, 0, 0, 0)]:
        a, b = lg.astype(np.float64), lg.astype(np.float64)
        a[idx] += h
        b[idx] -= h
        num = (grouped_nll(a, tg, E)[0] - grouped_nll(b, tg, E)[0]) / (2 * h)
        assert abs(num - dl[idx]) < 1e-8, (idx, num, dl[idx])
    # nothing labelled: loss 0, gradient exactly 0
    loss0, dl0, _, n0, _ = grouped_nll(lg, np.full_like(tg, -1), E)
    assert loss0 == 0.0 and n0 == 0 and not dl0.any()


def test_errors_restatement_takes_the_argmax_inside_each_group():
    p = np.zeros((1, 4, 1, 1, 2))
    p[0, :, 0, 0, 0] = [0.9, 0.1, 0.2, 0.8]          # classes (0, 1)
    p[0, :, 0, 0, 1] = [0.4, 0.6, 0.7, 0.3]          # classes (1, 0)
    t = np.zeros((1, 2, 1, 1, 2), np.float32)
    t[0, :, 0, 0, 0] = [0, 1]
    t[0, :, 0, 0, 1] = [1, 1]
    assert grouped_errors(p, t, 2) == 0.25
