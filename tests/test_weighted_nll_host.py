"""MultinoulliNLL with class / example weights and the lazy-labelling masks (reference
loss.py:172-259): construction, shapes, input order, parameter listing and the graph
description round trip.  No GPU."""
import numpy as np
import pytest


def _net(n_class=2, batch=None, sp=(7, 47, 47), **nll_kw):
    """neuro3d_lite-shaped net whose loss takes ``nll_kw``; values that are callables get the
    Softmax node (to build Inputs of matching shape)"""
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    inp = nm.Input((batch, 1) + sp, 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 8, (1, 4, 4), (1, 2, 2))
    out = nm.Conv(out, 8, (1, 1, 1))
    out = nm.Conv(out, n_class, (1, 1, 1), activation_func='lin')
    probs = nm.Softmax(out)
    target = nm.Input_like(probs, override_f=1, name='target')
    kw = {k: (v(probs) if callable(v) else v) for k, v in nll_kw.items()}
    nll = nm.MultinoulliNLL(probs, target, target_is_sparse=True, **kw)
    loss = nm.AggregateLoss(nll, name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss,
                          prediction_node=probs)
    return model, nll, probs


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


def test_each_weight_argument_constructs():
    """(on the code before this feature every one of these raised NotImplementedError)"""
    m, nll, _ = _net(class_weights=[1.0, 4.0])
    assert nll.class_weights is nll.params['class_weights']
    assert np.array_equal(nll.class_weights.get_value(), np.array([1, 4], np.float32))
    m, nll, _ = _net(class_weights=_class_w_node)
    assert nll.class_weights.name == 'cw' and 'class_weights' not in nll.params
    m, nll, _ = _net(example_weights=_example_w)
    assert nll.example_weights.name == 'ew'
    m, nll, _ = _net(mask_class_labeled=_mask('ll'))
    assert nll.mask_class_labeled.name == 'll' and nll.mask_class_not_present is None
    m, nll, _ = _net(mask_class_not_present=_mask('np'))
    assert nll.mask_class_not_present.name == 'np'
    assert nll.weighted
    m, nll, _ = _net()
    assert not nll.weighted


def test_shapes_input_order_and_parameter_listing():
    m, nll, probs = _net(n_class=3, class_weights=[1.0, 2.0, 3.0], example_weights=_example_w,
                         mask_class_labeled=_mask('ll'), mask_class_not_present=_mask('np'))
    # the reference's parent order (loss.py:218-235): pred, target, [class weight node],
    # example weights, mask_class_labeled, mask_class_not_present
    assert [n.name for n in m.loss_node.input_nodes] == ['raw', 'target', 'ew', 'll', 'np']
    assert nll.shape.shape == [None, 1, 7, 22, 22] and nll.shape.tags == probs.shape.tags
    assert nll.example_weights.shape.shape == [None, 7, 22, 22]
    assert nll.mask_class_labeled.shape.shape == [None, 3]
    nt = m.nontrainable_params
    assert [k for k in nt if 'class_weights' in k] == ['nll_class_weights']
    assert nt['nll_class_weights'] is nll.class_weights and not nll.class_weights.apply_train
    assert all(p is not nll.class_weights for p in m.trainable_params)
    # class weights as a node: an extra batch input between the target and the example weights
    m, nll, probs = _net(class_weights=_class_w_node, example_weights=_example_w,
                         mask_class_labeled=_mask('ll'))
    assert [n.name for n in m.loss_node.input_nodes] == ['raw', 'target', 'cw', 'ew', 'll']
    assert not [k for k in m.nontrainable_params if 'class_weights' in k]


def test_device_shapes_of_the_weight_inputs():
    """plan.out_shape maps 'f' and 'b' + spatial (no 'f') to the 5-D device layout and keeps
    rejecting every other axis order"""
    from elektronn2_amd import neuromancer as nm
    from elektronn2_amd.neuromancer.plan import Plan
    m, nll, probs = _net(class_weights=_class_w_node, example_weights=_example_w,
                         mask_class_labeled=_mask('ll'))

    class P(object):
        batch = 3
    assert Plan.out_shape(P, nll.class_weights) == (1, 2, 1, 1, 1)
    assert Plan.out_shape(P, nll.example_weights) == (3, 1, 7, 22, 22)
    assert Plan.out_shape(P, nll.mask_class_labeled) == (3, 2, 1, 1, 1)
    assert Plan.out_shape(P, nm.Input((None, 9, 9), 'b,x,y', name='ew2d')) == (3, 1, 1, 9, 9)
    with pytest.raises(NotImplementedError):
        Plan.out_shape(P, nm.Input((None, 9, 2), 'b,x,f', name='bad'))
    with pytest.raises(NotImplementedError):
        Plan.out_shape(P, nm.Input((4, 9), 'f,x', name='bad2'))


def test_bad_lengths_and_shapes_raise_value_error():
    from elektronn2_amd import neuromancer as nm
    with pytest.raises(ValueError):
        _net(class_weights=[1.0, 2.0, 3.0])                     # 2 classes
    with pytest.raises(ValueError):
        _net(class_weights=lambda p: nm.Input((3,), 'f', name='cw'))
    with pytest.raises(ValueError):
        _net(mask_class_labeled=lambda p: nm.Input((None, 3), 'b,f', name='ll'))
    with pytest.raises(ValueError):
        _net(mask_class_not_present=lambda p: nm.Input((2,), 'f', name='np'))
    with pytest.raises(ValueError):
        _net(example_weights=lambda p: nm.Input((None, 7, 22, 21), 'b,z,x,y', name='ew'))
    with pytest.raises(ValueError):
        _net(example_weights=lambda p: nm.Input((None, 1, 7, 22, 22), 'b,f,z,x,y', name='ew'))


def test_unsupported_options_are_still_rejected():
    from elektronn2_amd import neuromancer as nm
    for kw in (dict(weakness=0.1), dict(weakness=0.1, class_weights=[1.0, 2.0])):
        with pytest.raises(NotImplementedError) as e:
            _net(**kw)
        msg = str(e.value)
        assert 'weak' in msg
        assert not any(w in msg for w in ('class', 'example', 'mask'))
    nm.model_manager.reset()
    inp = nm.Input((None, 1, 7, 47, 47), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 4, (1, 4, 4), (1, 2, 2), activation_func='lin')
    probs = nm.Softmax(out)
    target = nm.Input_like(probs, name='target')
    with pytest.raises(NotImplementedError) as e:
        nm.MultinoulliNLL(probs, target, target_is_sparse=False)
    assert 'dense' in str(e.value) and 'weight' not in str(e.value) and 'mask' not in str(e.value)
    probs2 = nm.Softmax(out, n_indep=2, name='sm2')
    t2 = nm.Input_like(probs2, override_f=2, name='target2')
    with pytest.raises(NotImplementedError) as e:
        nm.MultinoulliNLL(probs2, t2, target_is_sparse=True, class_weights=[1.0, 2.0])
    assert 'n_indep' in str(e.value) and 'weight' not in str(e.value) and 'mask' not in str(e.value)


def test_serialise_rebuild_keeps_class_weights(tmp_path):
    from elektronn2_amd.neuromancer.model import modelload
    m, nll, _ = _net(class_weights=[1.0, 4.0], example_weights=_example_w,
                     mask_class_labeled=_mask('ll'), mask_class_not_present=_mask('np'))
    nll.class_weights.set_value(np.array([0.25, 3.5], np.float32))     # differs from the ctor's
    d = m.serialise()
    kw = [n for n in d['nodes'] if n[0] == 'nll'][0][3]
    assert kw['mask_class_labeled'] == {"__node__": "ll"} and kw['example_weights'] == {"__node__": "ew"}
    f = str(tmp_path / "w.mdl")
    m.save(f)
    m2 = modelload(f, name='rebuilt')
    assert list(m2.nodes.keys()) == list(m.nodes.keys())
    nll2 = m2.nodes['nll']
    assert np.array_equal(nll2.class_weights.get_value(), np.array([0.25, 3.5], np.float32))
    assert not nll2.class_weights.apply_train
    assert [n.name for n in m2.loss_node.input_nodes] == ['raw', 'target', 'ew', 'll', 'np']
    assert 'nll_class_weights' in m2.nontrainable_params
