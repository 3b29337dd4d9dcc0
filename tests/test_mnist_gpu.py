"""BASELINE config 1 (examples/mnist.py, the reference's own CPU-runnable case) through the
HIP path: 2-D convs (unit z axis) with train-mode batch normalisation, Perceptrons, softmax /
NLL on 'b,f' tensors -- loss, probabilities, every parameter gradient (through the batch
statistics), Adam steps with gamma's 3x weight decay and the running-statistics updates,
against oracle/mnist_oracle.py (torch float64 autograd of the restated forward pass).  The ops of
csrc/dense_bn.hip on their own: tests/test_batchnorm_gpu.py."""
import numpy as np
import pytest

from oracle import e2_oracle as O
from oracle import mnist_oracle as MO

pytestmark = pytest.mark.gpu
TOL = 1e-4
HYP = dict(lr=2e-4, mom=0.9, beta2=0.99, wd=0.5e-3)        # examples/mnist.py:18-23


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def all_params(m):
    """name -> value of every parameter (trainable and running statistics)"""
    out = {}
    for node in m.nodes.values():
        for k, p in node.params.items():
            if k in ('w', 'b', 'gamma', 'mean', 'std'):
                out['%s_%s' % (node.name, k)] = p.get_value()
    return out


def test_mnist_config_parity():
    from elektronn2_amd import nets, neuromancer as nm
    nm.model_manager.reset()
    np.random.seed(11)
    m = nets.mnist()
    m.set_opt_meta_params('Adam', HYP)
    rng = np.random.RandomState(2)
    x = rng.rand(20, 1, 26, 26).astype(np.float32)
    t = rng.randint(0, 10, (20, 1)).astype(np.float32)
    P = all_params(m)
    assert set(P) == {'conv_w', 'conv_b', 'conv_gamma', 'conv_mean', 'conv_std',
                      'conv1_w', 'conv1_b', 'conv1_gamma', 'conv1_mean', 'conv1_std',
                      'conv2_w', 'conv2_b', 'conv2_gamma', 'conv2_mean', 'conv2_std',
                      'dot_w', 'dot_b', 'dot1_w', 'dot1_b'}
    loss_ref, grads_ref, probs_ref, stats = MO.loss_and_grads(P, x, t)

    assert abs(float(m.loss(x, t)) - loss_ref) / abs(loss_ref) < TOL
    pr = m.predict(x)
    assert pr.shape == (20, 10) and rel(pr, probs_ref) < TOL
    l2, err, pr2 = m.predict_ext(x, t)
    assert abs(float(l2) - loss_ref) / abs(loss_ref) < TOL
    assert abs(float(err) - MO.classification_errors(probs_ref, t)) < 1e-6
    names = list(m.loss_node.all_trainable_params.keys())
    g = m.gradients(x, t)
    assert len(g) == len(names) == 13
    for nme, gv in zip(names, g):
        assert rel(gv, grads_ref[nme]) < TOL, nme
    # loss / prediction / gradient functions leave the running statistics alone
    P1 = all_params(m)
    for k in P:
        assert np.array_equal(P[k], P1[k]), k

    # three Adam steps: gamma with three times the weight decay, running statistics
    reg = {k: p.apply_reg for k, p in m.loss_node.all_trainable_params.items()}
    assert reg['conv_gamma'] == 3.0 and reg['conv_w'] is True and reg['conv_b'] is False
    Q = {k: np.asarray(v, np.float64) for k, v in P.items()}
    M = {k: np.zeros_like(Q[k]) for k in names}
    S = {k: np.zeros_like(Q[k]) for k in names}
    for step in range(1, 4):
        xs = rng.rand(20, 1, 26, 26).astype(np.float32)
        ts = rng.randint(0, 10, (20, 1)).astype(np.float32)
        lref, gref, _, st = MO.loss_and_grads(Q, xs, ts)
        for k in names:
            Q[k], M[k], S[k] = O.adam_step(Q[k], gref[k], M[k], S[k], step, HYP['lr'],
                                           HYP['mom'], HYP['beta2'], HYP['wd'], reg[k])
        for nme, (mean, std) in zip(('conv', 'conv1', 'conv2'), st):
            Q[nme + '_mean'] = 0.9995 * Q[nme + '_mean'] + 0.0005 * mean
            Q[nme + '_std'] = 0.9995 * Q[nme + '_std'] + 0.0005 * std
        loss = float(m.trainingstep(xs, ts, optimiser='Adam')[0])
        assert abs(loss - lref) / abs(lref) < TOL, step
    P3 = all_params(m)
    for k in P3:
        tol = 1e-5 if k.endswith(('_mean', '_std')) else 5e-4
        assert rel(P3[k], Q[k]) < tol, k
    assert not np.array_equal(P3['conv_mean'], P['conv_mean'])     # the statistics moved
