"""Activations shared between nodes (fan-out), host side (no GPU): the graphs of
tests/wiring_cases.py, the order in which the backward pass reaches the consumers of every fan-out
node, and the reference side of tests/test_wiring_gpu.py -- on the float64 reference alone, dropping
or doubling the gradient that flows back along ONE consumer edge moves some parameter gradient by
more than 10x the GPU bound (of that gradient's largest entry), for every fan-out node and every
edge of every net.  So a launch that overwrites where it has to add, adds where it has to
overwrite, or a fusion that fails to stand down cannot pass the GPU comparison."""
import numpy as np
import pytest

import wiring_cases as W
from wiring_cases import CASES, CASE_IDS, TOL


def _moved(g, g0):
    return float(np.abs(g - g0).max() / max(np.abs(g0).max(), 1e-30))


# ---- 1. the graphs ---------------------------------------------------------------------------------
def test_add_and_automerge_add_bookkeeping():
    from elektronn2_amd import neuromancer as nm
    m = W.build('unet_add')
    mg = m.nodes['merge']
    assert type(mg).__name__ == 'Add'
    assert [type(p).__name__ for p in mg.parent] == ['UpConv', 'Crop']      # (lo_res, hi_res)
    assert mg.parent[1].parent is m.nodes['c1'] and tuple(mg.parent[1].crop) == (0, 2, 2)
    assert tuple(mg.shape.shape) == tuple(mg.parent[0].shape.shape) == (2, 6, 4, 12, 12)
    assert mg.computational_cost == 0 and mg.param_count == 0
    assert nm.UpConvMerge is nm.AutoMerge
    with pytest.raises(ValueError, match="merge_mode"):
        nm.AutoMerge(m.nodes['c1'], m.nodes['low'], 6, merge_mode='mul')
    with pytest.raises(AssertionError):
        nm.Add(m.nodes['c0'], m.nodes['c1'])                                 # shapes differ
    # a node given twice is one child of its parent
    m = W.build('twice')
    assert list(m.nodes['a'].children) == ['s'] and list(m.nodes['cr'].children) == ['cat']
    assert m.nodes['cat'].shape['f'] == 2 * m.nodes['cr'].shape['f']


@pytest.mark.parametrize("name,flip", CASES, ids=CASE_IDS)
def test_backward_order_of_the_consumers(name, flip):
    """which consumer writes a fan-out node's gradient first, by the rule of Plan._bwd_nodes (the
    GPU tests assert the same of the plan)"""
    m = W.build(name, flip)
    ws = W.writers(m, W.backward_order(m))
    for node, lst in ws.items():
        print("%s%s: d/d%s written by %s" % (name, " (flipped)" if flip else "", node,
                                              ", then ".join("%s[%d] (%s)" % w for w in lst)))
    assert dict((k, v[0][0]) for k, v in ws.items()) == W.FIRST[name, flip]
    # every fan-out node has a trainable Conv upstream (or is one)
    for node in ws:
        assert any(type(n).__name__ == 'Conv' and n.param_count
                   for n in m.nodes[node].all_parents.values())


def test_every_writer_kind_comes_first_and_later():
    first, later = set(), set()
    for name, flip in CASES:
        m = W.build(name, flip)
        for lst in W.writers(m, W.backward_order(m)).values():
            first.add(lst[0][2])
            later.update(w[2] for w in lst[1:])
    assert first >= set(W.GRAPH_KINDS), sorted(set(W.GRAPH_KINDS) - first)
    assert later >= set(W.GRAPH_KINDS), sorted(set(W.GRAPH_KINDS) - later)


def test_a_flip_changes_the_order_not_the_function():
    """both orders of a net are one function of the same parameters: same loss, same gradients"""
    for name in W.FLIPPED:
        r0, r1 = W.reference(name, False), W.reference(name, True)
        m0, m1 = W.build(name, False), W.build(name, True)
        assert W.FIRST[name, False] != W.FIRST[name, True]
        g0 = dict(zip(m0.loss_node.all_trainable_params.keys(), r0['grads0']))
        g1 = dict(zip(m1.loss_node.all_trainable_params.keys(), r1['grads0']))
        if name in ('unet_add', 'unet_cat', 'mh_third', 'cat_copy'):
            continue            # (other creation order or channel order: another function)
        assert abs(r0['loss0'] - r1['loss0']) <= 1e-12 * abs(r0['loss0']), name
        assert sorted(g0) == sorted(g1)
        for k in g0:
            assert _moved(g1[k], g0[k]) <= 1e-9, (name, k)


# ---- 2. a wrong sum cannot pass ----------------------------------------------------------------------
@pytest.mark.parametrize("name,flip", CASES, ids=CASE_IDS)
def test_a_dropped_or_doubled_edge_is_far_off(name, flip):
    r = W.reference(name, flip)
    m = W.build(name, flip)
    names = list(m.loss_node.all_trainable_params.keys())
    assert np.isfinite(r['loss0']) and all(np.abs(g).max() > 0 for g in r['grads0'])
    fans = W.fanouts(m)
    assert sorted(n.name for n, _ in fans) == sorted(W.FIRST[name, flip])
    for node, edges in fans:
        for c, slot in edges:
            for scale in (0.0, 2.0):
                ref = W.WRef(m, edge=(node.name, c.name, slot, scale))
                loss, pred = ref.loss_and_grads(*W.batch(r))
                assert loss == r['loss0'] and np.array_equal(pred, r['pred0'])     # forward: unchanged
                moved = [_moved(g, g0) for g, g0 in zip(ref.grads(), r['grads0'])]
                k = int(np.argmax(moved))
                print("%s%s: edge %s -> %s[%d] x %g moves d/d%s by %.3g of its largest entry"
                      % (name, " (flipped)" if flip else "", node.name, c.name, slot, scale,
                         names[k], moved[k]))
                assert moved[k] > 10 * TOL
    # the steps move: every step's loss differs from the one before
    for k in range(1, W.N_STEPS):
        assert abs(r['losses'][k] - r['losses'][k - 1]) > 0


def test_residual_figures():
    """the figures of the `residual` net on the gradients of `a` (which every edge of `a` reaches)"""
    r = W.reference('residual')
    m = W.build('residual')
    names = list(m.loss_node.all_trainable_params.keys())
    iw, ib = names.index('a_w'), names.index('a_b')
    for c in ('b', 's', 'd'):
        ref = W.WRef(m, edge=('a', c, 0, 0.0))
        ref.loss_and_grads(*W.batch(r))
        g = ref.grads()
        mw, mb = _moved(g[iw], r['grads0'][iw]), _moved(g[ib], r['grads0'][ib])
        print("residual: edge a -> %s dropped: d/dw %.3g, d/db %.3g" % (c, mw, mb))
        assert mw > 10 * TOL and mb > 10 * TOL
