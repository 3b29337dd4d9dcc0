"""Parameters shared between nodes (``w=<other>.w``, ``b=...``, ``gamma=...``), host side (no GPU):
registration and bookkeeping (NeuralLayer._register_param, "shared from elsewhere"), values seen
through either node, ``save`` -> ``modelload`` of the ``{"__param__": [node, key]}`` form, and the
reference side of tests/test_shared_params_gpu.py: for every net there, the two contributions to a
shared gradient add up to the tied gradient, and each alone is far from it -- so a dropped or a
doubled contribution cannot pass the GPU comparison."""
import numpy as np
import pytest

import shared_param_cases as S
from shared_param_cases import NETS, TOL, borrowed


def _nm():
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    return nm


def _count(p):
    return int(np.prod(p.get_value().shape))


# ---- 1. registration --------------------------------------------------------------------------------
def _pair(nm, kind, keys):
    """(owner a, sharing b): b takes the parameters ``keys`` from a"""
    bn = 'train' if 'gamma' in keys else False
    if kind == 'Conv':
        inp = nm.Input((1, 3, 4, 12, 12), 'b,f,z,x,y', name='raw')
        a = nm.Conv(inp, 3, (1, 3, 3), batch_normalisation=bn, name='a')
        kw = {k: getattr(a, k) for k in keys}
        b = nm.Conv(a, 3, (1, 3, 3), (1, 2, 2), batch_normalisation=bn, name='b', **kw)
    elif kind == 'UpConv':
        inp = nm.Input((1, 3, 4, 6, 6), 'b,f,z,x,y', name='raw')
        a = nm.UpConv(inp, 3, (1, 2, 2), batch_normalisation=bn, name='a')
        kw = {k: getattr(a, k) for k in keys}
        b = nm.UpConv(a, 3, (1, 2, 2), batch_normalisation=bn, name='b', identity_init=False, **kw)
    else:
        inp = nm.Input((2, 6), 'b,f', name='raw')
        a = nm.Perceptron(inp, 6, batch_normalisation=bn, name='a')
        kw = {k: getattr(a, k) for k in keys}
        b = nm.Perceptron(a, 6, batch_normalisation=bn, name='b', **kw)
    return a, b


@pytest.mark.parametrize("kind", ['Conv', 'UpConv', 'Perceptron'])
@pytest.mark.parametrize("keys", [('w',), ('b',), ('w', 'b'), ('gamma',), ('w', 'b', 'gamma')],
                         ids=lambda k: '+'.join(k))
def test_a_node_takes_parameters_of_another(kind, keys):
    nm = _nm()
    a, b = _pair(nm, kind, keys)
    own = [k for k in ('w', 'b') + (('gamma',) if 'gamma' in keys else ()) if k not in keys]
    for k in keys:
        assert getattr(b, k) is getattr(a, k)
        assert k not in b.params and a.params[k] is getattr(a, k)
    for k in own:
        assert getattr(b, k) is not getattr(a, k) and b.params[k] is getattr(b, k)
    # counted where it lives, once in every list of the graph
    assert a.param_count == sum(_count(p) for p in a.params.values() if p.apply_train)
    assert b.param_count == sum(_count(getattr(b, k)) for k in own)
    every = list(b.all_trainable_params.values())
    assert len(set(id(p) for p in every)) == len(every)
    for k in keys:
        assert sum(p is getattr(a, k) for p in every) == 1
    assert b.all_params_count == a.param_count + b.param_count
    # set_value through either node is seen by both
    for k in keys:
        v = getattr(a, k).get_value()
        getattr(b, k).set_value(v + 1.0)
        assert np.array_equal(getattr(a, k).get_value(), v + 1.0)
        getattr(a, k).set_value(v - 2.0)
        assert np.array_equal(getattr(b, k).get_value(), v - 2.0)


def test_shape_mismatch_and_constant_forms():
    nm = _nm()
    inp = nm.Input((1, 3, 4, 12, 12), 'b,f,z,x,y', name='raw')
    a = nm.Conv(inp, 3, (1, 3, 3), name='a')
    with pytest.raises(ValueError, match="Shape mismatch"):
        nm.Conv(a, 4, (1, 3, 3), w=a.w)                   # (4, 3, 1, 3, 3) wanted
    with pytest.raises(ValueError, match="Shape mismatch"):
        nm.Conv(a, 3, (1, 1, 1), w=a.w)
    with pytest.raises(ValueError, match="Shape mismatch"):
        nm.Conv(a, 4, (1, 3, 3), b=a.b)
    with pytest.raises(ValueError, match="Shape mismatch"):
        nm.UpConv(a, 3, (1, 2, 2), w=a.w)
    with pytest.raises(ValueError, match="Shape mismatch"):
        nm.Perceptron(nm.Input((2, 6), 'b,f', name='flat'), 6, b=a.b)
    with pytest.raises(ValueError, match="must be either"):
        nm.Conv(a, 3, (1, 3, 3), w="a.w")
    # constants stay out of the trainable lists: the [array, 'const'] form, and a ConstantParam
    # handed on to a second node
    wv = np.full((3, 3, 1, 3, 3), 0.25, np.float32)
    c = nm.Conv(a, 3, (1, 3, 3), w=[wv, 'const'], name='c')
    assert c.w.constant and not c.w.apply_train and c.params['w'] is c.w
    assert np.array_equal(c.w.get_value(), wv)
    d = nm.Conv(c, 3, (1, 3, 3), w=c.w, name='d')
    assert d.w is c.w and 'w' not in d.params
    every = list(d.all_trainable_params.values())
    assert not any(p is c.w for p in every)
    assert sum(p is a.w for p in every) == 1 and any(p is d.b for p in every)
    assert c.param_count == 3 and d.param_count == 3       # their biases
    with pytest.raises(ValueError, match="constant"):
        c.set_param_values(dict(w=wv))
    t = nm.Conv(d, 3, (1, 3, 3), w=[wv, 'trainable'], name='t')
    assert t.w.apply_train and t.params['w'] is t.w


# ---- 2. the nets of the GPU tests -------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NETS))
def test_model_lists_hold_a_shared_parameter_once(name):
    m = S.build(name)
    a, b = m.nodes['a'], m.nodes['b']
    keys = NETS[name][2]
    assert sorted((n.name, k) for n, k, _ in borrowed(m)) == sorted(('b', k) for k in keys)
    tp = m.trainable_params
    assert len(set(id(p) for p in tp)) == len(tp)
    assert [id(p) for p in tp] == [id(p) for p in m.loss_node.all_trainable_params.values()]
    for k in keys:
        assert sum(p is getattr(a, k) for p in tp) == 1
    total = sum(n.param_count for n in m.nodes.values())
    assert total == sum(_count(p) for p in tp) == m.loss_node.all_params_count
    assert b.param_count == sum(_count(p) for p in b.params.values() if p.apply_train)
    assert all(getattr(b, k) is not p for k in keys for p in b.params.values())


@pytest.mark.parametrize("name", ['S1', 'S3', 'S7', 'S8'])
def test_values_round_trip_through_the_model(name):
    m = S.build(name)
    a, b = m.nodes['a'], m.nodes['b']
    keys = NETS[name][2]
    vals = m.get_param_values()
    assert all(k in vals['a'] and k not in vals['b'] for k in keys)
    changed = {n: {k: v + 0.5 for k, v in d.items()} for n, d in vals.items()}
    m.set_param_values(changed)
    for k in keys:
        assert np.array_equal(getattr(b, k).get_value(), vals['a'][k] + 0.5)
    back = m.get_param_values()
    for n, d in changed.items():
        for k, v in d.items():
            assert np.array_equal(back[n][k], v)
    m.set_param_values(m.get_param_values(as_list=True))      # the list form, in node order
    assert np.array_equal(getattr(b, keys[0]).get_value(), changed['a'][keys[0]])


@pytest.mark.parametrize("name", sorted(NETS))
def test_save_and_modelload_keep_the_sharing(name, tmp_path):
    from elektronn2_amd import neuromancer as nm
    m = S.build(name)
    keys = NETS[name][2]
    graph = {n[0]: n for n in m.serialise()['nodes']}
    for k in keys:
        assert graph['b'][3][k] == {"__param__": ['a', k]}
    f = str(tmp_path / "shared.mdl")
    m.save(f)
    m2 = nm.modelload(f, name='again')
    a2, b2 = m2.nodes['a'], m2.nodes['b']
    assert a2 is not m.nodes['a']
    for k in keys:
        assert getattr(b2, k) is getattr(a2, k) and k not in b2.params
        assert getattr(a2, k) is not getattr(m.nodes['a'], k)
    assert [n for n in m2.nodes] == [n for n in m.nodes]
    assert len(m2.trainable_params) == len(m.trainable_params)
    for p, q in zip(m.trainable_params, m2.trainable_params):
        assert p is not q and np.array_equal(p.get_value(), q.get_value())
    for k in keys:
        v = getattr(a2, k).get_value()
        getattr(a2, k).set_value(v * 2 + 1)
        assert np.array_equal(getattr(b2, k).get_value(), v * 2 + 1)
        assert np.array_equal(getattr(m.nodes['a'], k).get_value(), v)       # the saved model: untouched
    # the reloaded graph computes what the saved one did
    r = S.reference(name)
    for k in keys:
        getattr(a2, k).set_value(getattr(m.nodes['a'], k).get_value())
    ref2 = S.SRef(m2)
    loss, pred = ref2.loss_and_grads(r['x'], r['t'])
    assert loss == r['loss0'] and np.array_equal(pred, r['pred0'])
    for g, g0 in zip(ref2.grads(), r['grads0']):
        assert np.array_equal(g, g0)
    # into an existing graph: values land in both users
    m3 = S.build(name)
    for p in m3.trainable_params:
        p.set_value(p.get_value() * 0)
    nm.modelload(f, m3)
    for p, q in zip(m.trainable_params, m3.trainable_params):
        assert np.array_equal(p.get_value(), q.get_value())


# ---- 3. the untied twin: what the GPU comparison can tell apart -------------------------------------
@pytest.mark.parametrize("name", sorted(NETS))
def test_contributions_add_up_and_each_alone_is_far_off(name):
    r = S.reference(name)
    assert r['twin_loss0'] == r['loss0']
    assert len(r['contrib']) == len(NETS[name][2])
    for tied, ga, gb in r['contrib']:
        top = np.abs(tied).max()
        assert np.abs(ga + gb - tied).max() <= 1e-12 * top
        for part in (ga, gb):
            # the sum without the other contribution, and with this one twice
            far = np.abs(part).max() / top
            print("%s %s: one contribution is %.3g of the largest gradient entry" % (name, tied.shape, far))
            assert far > 10 * TOL
            if name in S.BF16_NETS:        # the bf16 variant of the GPU tests, with ITS gradient bound
                assert far > 10 * S.BF16_GRAD
    # the steps move: every shared parameter changes by far more than the GPU bound resolves
    for k in range(1, S.N_STEPS):
        assert abs(r['losses'][k] - r['losses'][k - 1]) > 0
