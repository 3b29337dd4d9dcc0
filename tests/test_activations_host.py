"""Activations beyond relu / lin, host side (no GPU): the names Conv / UpConv / Perceptron accept
(computations.py:57-134), shape / stride / fov bookkeeping, bias initialisation per name
(neural.py:174-190 of the reference), the rejected names, the save -> modelload round trip, the
``backend.ACT`` table -- and the float64 restatement of the functions and their slopes
(``act_f`` / ``act_df`` / ``act_torch``), which tests/test_activations_gpu.py imports as the
reference of every comparison there (never the kernels).  The restatement is checked here against
torch-CPU's own functions and autograd."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from elektronn2_amd.neuromancer.neural import check_activation

# name -> E2_ACT_* of include/e2hip.h
CANON = {'lin': 0, 'linear': 0, 'relu': 1, 'tanh': 2, 'sigmoid': 3, 'sig': 3, 'logistic': 3,
         'abs': 4, 'elu': 5, 'selu': 6, 'soft+': 7}
ACCEPTED = tuple(CANON)
NEW = tuple(n for n in ACCEPTED if n not in ('relu', 'lin'))
REJECTED = ('prelu', 'maxout 2', 'concentration', 'radius', 'softmax', 'gelu')
SELU_A = 1.6732632423543772848170429916717          # computations.py:96-97
SELU_S = 1.0507009873554804934193349852946
KINKED = (1, 4, 6)                                  # relu, abs, selu: the slope jumps at 0


# ---- the float64 restatement -------------------------------------------------------------------
def act_f(name, v):
    """f(v) in float64 NumPy, in forms that neither overflow nor cancel"""
    check_activation(name)
    k = CANON[name]
    v = np.asarray(v, np.float64)
    a = np.abs(v)
    neg = np.minimum(v, 0.0)
    if k == 0:
        return v.copy()
    if k == 1:
        return 0.5 * (v + a)                        # T.nnet.relu
    if k == 2:
        e = np.expm1(-2.0 * a)                      # tanh |v| = -e / (e + 2)
        return np.sign(v) * (-e / (e + 2.0))
    if k == 3:
        e = np.exp(-a)
        return np.where(v >= 0, 1.0, e) / (1.0 + e)
    if k == 4:
        return a
    if k == 5:
        return np.where(v > 0, v, np.expm1(neg))
    if k == 6:
        return SELU_S * np.where(v > 0, v, SELU_A * np.expm1(neg))
    return np.maximum(v, 0.0) + np.log1p(np.exp(-a))


def act_df(name, v):
    """the slope used in the backward pass (the table of the activation section of DESIGN.md);
    at v = 0: relu 0.5, abs 0, elu / selu the second branch of switch(v > 0, ..)"""
    check_activation(name)
    k = CANON[name]
    v = np.asarray(v, np.float64)
    neg = np.minimum(v, 0.0)
    if k == 0:
        return np.ones_like(v)
    if k == 1:
        return np.where(v > 0, 1.0, np.where(v == 0, 0.5, 0.0))
    if k == 2:
        f = act_f(name, v)
        return 1.0 - f * f
    if k == 3:
        f = act_f(name, v)
        return f * (1.0 - f)
    if k == 4:
        return np.sign(v)
    if k == 5:
        return np.where(v > 0, 1.0, np.exp(neg))
    if k == 6:
        return np.where(v > 0, SELU_S, SELU_S * SELU_A * np.exp(neg))
    return act_f('sigmoid', v)


class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, name):
        ctx.save_for_backward(v)
        ctx.name = name
        return torch.from_numpy(np.ascontiguousarray(act_f(name, v.detach().numpy())))

    @staticmethod
    def backward(ctx, g):
        v, = ctx.saved_tensors
        return g * torch.from_numpy(np.ascontiguousarray(act_df(ctx.name, v.detach().numpy()))), None


def act_torch(name, v):
    """the restatement as a differentiable float64 torch-CPU op (slopes: act_df)"""
    assert v.dtype == torch.float64
    return _Act.apply(v, name)


TORCH_F = {2: torch.tanh, 3: torch.sigmoid, 4: torch.abs, 5: F.elu, 6: F.selu,
           7: lambda v: F.softplus(v, threshold=1e6), 1: torch.relu, 0: lambda v: v}


def test_restatement_agrees_with_torch_and_takes_the_stated_slopes_at_zero():
    rng = np.random.RandomState(3)
    v = np.concatenate([rng.randn(4000) * 8.0, np.float64([30, -30, 100, -100, 1e-42, -1e-42, 1e-3, -1e-3])])
    v = v[np.abs(v) > 1e-50]                              # away from the kinks
    for name in ACCEPTED:
        k = CANON[name]
        t = torch.tensor(v, requires_grad=True)
        want = TORCH_F[k](t)
        want.sum().backward()
        got = act_f(name, v)
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(act_df(name, v))), name
        assert np.abs(got - want.detach().numpy()).max() <= 1e-12 * max(1.0, np.abs(got).max()), name
        assert np.abs(act_df(name, v) - t.grad.numpy()).max() <= 1e-12, name
        # the differentiable wrapper hands exactly these to autograd
        t2 = torch.tensor(v, requires_grad=True)
        y = act_torch(name, t2)
        (y * torch.tensor(np.arange(v.size) % 3 + 1.0)).sum().backward()
        assert np.array_equal(y.detach().numpy(), got), name
        assert np.array_equal(t2.grad.numpy(), act_df(name, v) * (np.arange(v.size) % 3 + 1.0)), name
    z = np.float64([0.0, -0.0])
    assert np.array_equal(act_df('relu', z), [0.5, 0.5])
    assert np.array_equal(act_df('abs', z), [0.0, 0.0])
    assert np.array_equal(act_df('elu', z), [1.0, 1.0])
    assert np.array_equal(act_df('selu', z), [SELU_S * SELU_A] * 2)
    assert np.array_equal(act_df('tanh', z), [1.0, 1.0])
    assert np.array_equal(act_df('sigmoid', z), [0.25, 0.25])
    assert np.array_equal(act_df('soft+', z), [0.5, 0.5])
    for alias, name in (('sig', 'sigmoid'), ('logistic', 'sigmoid'), ('linear', 'lin')):
        assert np.array_equal(act_f(alias, v), act_f(name, v))
        assert np.array_equal(act_df(alias, v), act_df(name, v))


# ---- the front end -----------------------------------------------------------------------------
def _nodes(act):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(5)
    inp = nm.Input((1, 1, 6, 20, 20), 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, 8, (1, 3, 3), activation_func=act, name='c0')
    c1 = nm.Conv(c0, 8, (1, 3, 3), (1, 2, 2), activation_func=act, name='c1')
    c2 = nm.Conv(c1, 16, (3, 3, 3), activation_func=act, batch_normalisation='train', name='c2')
    up = nm.UpConv(c2, 6, (1, 2, 2), activation_func=act, name='up')
    mrg = nm.UpConvMerge(c0, c2, 12, upconv_kwargs=dict(activation_func=act), name='mrg')
    x2 = nm.Input((4, 10), 'b,f', name='x2')
    pc = nm.Perceptron(x2, 5, activation_func=act, name='pc')
    return nm, dict(c0=c0, c1=c1, c2=c2, up=up, mrg=mrg, pc=pc)


@pytest.mark.parametrize("act", NEW)
def test_every_accepted_name_builds_and_bookkeeping_equals_relu(act):
    nm, new = _nodes(act)
    desc = dict((k, (list(n.shape.shape), list(np.ravel(n.shape.strides)), list(np.ravel(n.shape.fov)),
                     n.shape.tags)) for k, n in new.items())
    mup = [n for n in new['mrg'].parent if type(n).__name__ in ('UpConv', 'Crop')]
    up_of_merge = mup[0] if type(mup[0]).__name__ == 'UpConv' else mup[0].parent
    assert up_of_merge.activation_func == act
    for k in ('c0', 'c1', 'c2', 'up', 'pc'):
        n = new[k]
        assert n.activation_func == act                 # the string as given
        assert ("act='%s'" % act) in repr(n) or k == 'pc'
        assert n._plain_act() == (act == 'linear')
        assert n._lin_act() == ('linear' if act == 'linear' else 'lin')
    nm, old = _nodes('relu')
    for k, n in old.items():
        assert desc[k] == (list(n.shape.shape), list(np.ravel(n.shape.strides)),
                           list(np.ravel(n.shape.fov)), n.shape.tags), k
        assert k == 'mrg' or n._plain_act()
    # Conv.make_dual passes the name on
    nm, new = _nodes(act)
    dual = new['c1'].make_dual(new['c1'])
    assert type(dual).__name__ == 'UpConv' and dual.activation_func == act


@pytest.mark.parametrize("act", ACCEPTED)
def test_bias_initialisation_per_name(act):
    """neural.py:174-190 of the reference compares STRINGS: 'relu' -> const 1 / fov, the literal
    'sigmoid' -> const 0.5, everything else (the aliases 'sig' / 'logistic' included) -> 'fix-uni'
    1e-6; a fresh UpConv zeroes its bias (identity_init)"""
    nm, n = _nodes(act)
    for k in ('c0', 'c1', 'c2', 'pc'):
        b = n[k].b.get_value()
        assert b.dtype == np.float32 and b.shape == (n[k].n_f,)
        if act == 'relu':
            fov = 1 if k == 'pc' else int(np.prod(n[k].filter_shape))
            assert np.allclose(b, 1.0 / fov), (k, b)
        elif act == 'sigmoid':
            assert np.array_equal(b, np.full_like(b, 0.5)), (k, b)
        else:
            assert np.all(np.abs(b) <= 1e-6) and np.abs(b).max() > 0 and len(set(b.tolist())) > 1, (k, b)
    assert np.array_equal(n['up'].b.get_value(), np.zeros(6, np.float32))


@pytest.mark.parametrize("bad", REJECTED)
def test_rejected_names_raise_and_list_the_accepted_ones(bad):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    inp = nm.Input((1, 1, 6, 20, 20), 'b,f,z,x,y', name='raw')
    x2 = nm.Input((4, 10), 'b,f', name='x2')
    makers = [lambda: nm.Conv(inp, 4, (1, 3, 3), activation_func=bad),
              lambda: nm.UpConv(inp, 4, (1, 2, 2), activation_func=bad),
              lambda: nm.Perceptron(x2, 4, activation_func=bad)]
    for make in makers:
        with pytest.raises(NotImplementedError) as e:
            make()
        for name in ACCEPTED:
            assert repr(name) in str(e.value), (name, str(e.value))


def _net(acts):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    inp = nm.Input((None, 1, 7, 47, 47), 'b,f,z,x,y', name='raw')
    out = nm.Conv(inp, 6, (1, 4, 4), (1, 2, 2), activation_func=acts[0])
    out = nm.Conv(out, 8, (3, 3, 3), (1, 2, 2), activation_func=acts[1])
    out = nm.Conv(out, 8, (1, 3, 3), activation_func=acts[2])
    out = nm.Conv(out, 2, (1, 1, 1), activation_func='lin')
    probs = nm.Softmax(out)
    target = nm.Input_like(probs, override_f=1, name='target')
    loss = nm.AggregateLoss(nm.MultinoulliNLL(probs, target, target_is_sparse=True), name='loss')
    model = nm.model_manager.getmodel()
    model.designate_nodes(input_node=inp, target_node=target, loss_node=loss, prediction_node=probs)
    return model


def test_save_and_modelload_keep_the_strings(tmp_path):
    from elektronn2_amd.neuromancer.model import modelload
    for i, acts in enumerate((('tanh', 'logistic', 'soft+'), ('sig', 'selu', 'abs'), ('elu', 'sigmoid', 'linear'))):
        m = _net(acts)
        f = str(tmp_path / ("act%d.mdl" % i))
        m.save(f)
        m2 = modelload(f, name='rebuilt%d' % i)
        convs = [n for n in m2.nodes.values() if type(n).__name__ == 'Conv']
        assert tuple(n.activation_func for n in convs) == acts + ('lin',)
        for n in convs:
            assert np.array_equal(n.b.get_value(), m.nodes[n.name].b.get_value())
        m3 = modelload(f, name='bigger%d' % i, imposed_patch_size=(9, 60, 58), imposed_batch_size=2)
        assert tuple(n.activation_func for n in m3.nodes.values()
                     if type(n).__name__ == 'Conv') == acts + ('lin',)


def test_backend_table_covers_exactly_the_accepted_names():
    from elektronn2_amd import backend
    from elektronn2_amd.neuromancer import neural
    assert dict(backend.ACT) == CANON
    assert set(neural._HIP_ACTS) == set(ACCEPTED)
    assert sorted(set(backend.ACT.values())) == list(range(8))
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "include", "e2hip.h")).read()
    m = re.search(r"enum \{ E2_ACT_LIN = 0, E2_ACT_RELU = 1, ([A-Z0-9_, \n]+)\};", hdr)
    assert m, "the E2_ACT_* enum of include/e2hip.h"
    rest = [w.strip() for w in m.group(1).split(',') if w.strip()]
    assert rest == ['E2_ACT_TANH', 'E2_ACT_SIGMOID', 'E2_ACT_ABS', 'E2_ACT_ELU', 'E2_ACT_SELU',
                    'E2_ACT_SOFTPLUS']
    assert {'e2_act_fwd', 'e2_act_bwd'} <= set(backend.EXPORTED_SYMBOLS)
