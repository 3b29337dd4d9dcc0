"""GaussianRV and its AEVB prior, host side (no GPU): the NumPy float64 restatement of the noise
contract of include/e2hip.h (on the Philox restatement of tests/test_dropout_host.py), the formulas
of the four entry points pinned to torch-CPU float64 autograd with eps held fixed, the statistics of
the restated noise, and the node logic (various.py:32-151).  tests/test_gauss_rv_gpu.py imports the
restatement from here: it is the reference of every comparison there, never the kernels."""
import numpy as np
import pytest
import torch

from test_dropout_host import philox4x32_10, LO, S32

# the statistics case.  The seed is the first one tried: the restatement passes both bounds with it
# on the CPU (|mean| = 8.6e-4 < 4.9e-3, |var - 1| = 2.7e-3 < 6.9e-3)
STAT = dict(seed=(7 << 32) + 1234, counter=5, stream=3)
STAT_N = 1 << 20


def restated_normals(n, seed, counter, stream):
    """eps[j], j = 0 .. n-1, in float64 -- include/e2hip.h, the noise contract"""
    q = np.arange((int(n) + 3) // 4, dtype=np.uint64)
    z = np.zeros_like(q)
    w = philox4x32_10((q & LO, q >> S32, z + np.uint64(int(stream) & 0xffffffff),
                       z + np.uint64(int(counter) & 0xffffffff)),
                      (int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff))
    eps = np.empty((q.size, 4), np.float64)
    for k in (0, 2):
        ua = ((w[k] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        ub = (w[k + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(ua))
        eps[:, k], eps[:, k + 1] = r * np.cos(2.0 * np.pi * ub), r * np.sin(2.0 * np.pi * ub)
    return eps.reshape(-1)[:int(n)]


def restated(mu, ls, eps=0.0, dout=0.0, coef=1.0):
    """the sample z and its (dmu, dlog_sig) for the output gradient ``dout``; the element-wise prior
    (its mean is the term of the mix) and (dmu, dlog_sig) of ``coef`` times its sum"""
    return dict(z=mu + np.exp(ls) * eps, rv_bwd=(dout, dout * eps * np.exp(ls)),
                prior=0.5 * (mu ** 2 + np.exp(2.0 * ls) - 1.0 - 2.0 * ls),
                prior_bwd=(coef * mu, coef * (np.exp(2.0 * ls) - 1.0)))


def test_formulas_against_float64_autograd_with_eps_held_fixed():
    mu, ls, g = np.random.RandomState(1).randn(3, 2, 3, 5)
    eps = restated_normals(30, 11, 2, 1).reshape(2, 3, 5)
    got = restated(mu, ls, eps, g, 0.37)
    tm, tl = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (mu, ls))
    z = tm + torch.exp(tl) * torch.tensor(eps)
    prior = 0.5 * (tm ** 2 + torch.exp(tl) ** 2 - 1 - 2 * tl)
    for val, out, key in ((z, z, 'rv_bwd'), (prior, 0.37 * prior, 'prior_bwd')):
        assert np.allclose(got['z' if val is z else 'prior'], val.detach().numpy(), rtol=1e-13, atol=1e-15)
        grads = torch.autograd.grad(out, (tm, tl), torch.tensor(g) if val is z else torch.ones_like(out))
        for a, b in zip(got[key], grads):
            assert np.allclose(a, b.numpy(), rtol=1e-13, atol=1e-15), key


def test_statistics_of_the_restated_noise():
    """N normals: the mean has standard deviation 1 / sqrt(N), the variance sqrt(2 / N)"""
    eps = restated_normals(STAT_N, **STAT)
    print("mean %.3e var - 1 %.3e" % (eps.mean(), eps.var() - 1.0))
    assert np.isfinite(eps).all() and abs(eps.mean()) < 5.0 / np.sqrt(STAT_N)
    assert abs(eps.var() - 1.0) < 5.0 * np.sqrt(2.0 / STAT_N)
    # a function of (seed, counter, stream, j) alone: a prefix is a prefix, every word matters
    assert np.array_equal(restated_normals(37, **STAT), eps[:37])
    for key in STAT:
        assert np.abs(restated_normals(64, **dict(STAT, **{key: STAT[key] + 1})) - eps[:64]).max() > 0.5


FORMS = [((2, 6), 'b,f'), ((2, 6, 5, 7), 'b,f,x,y'), ((2, 6, 5, 7), 'b,f,y,x'), ((2, 6, 3, 5, 7), 'b,f,z,x,y')]


@pytest.mark.parametrize("shape,tags", FORMS, ids=[f[1] for f in FORMS])
def test_shapes_cost_and_priorlayer(shape, tags):
    from elektronn2_amd import neuromancer as nm
    nm.model_manager.reset()
    both = nm.Input(shape, tags, name='both')
    for mu, ls in (nm.split(both, 'f', n_out=2), (nm.Input_like(both, name='m'), nm.Input_like(both, name='l'))):
        z = nm.GaussianRV(mu, ls, name='z' + mu.name)
        assert tuple(z.shape.shape) == tuple(mu.shape.shape) and tuple(z.shape.tags) == tuple(mu.shape.tags)
        assert z.computational_cost == mu.shape.stripnone_prod         # various.py:91-96
        prior = z.make_priorlayer()
        assert isinstance(prior, nm.GaussianAEVBPrior) and prior.name == z.name + "_prior"
        assert prior.mu is mu and prior.log_sig is ls and prior.n_samples == 0
        loss = nm.AggregateLoss([nm.SquaredLoss(z, nm.Input_like(z, name='t')), prior], mixing_weights=[1.0, 0.5])
        assert loss.elementwise and prior.term_value is None


def test_refusals_and_exported_symbols():
    from elektronn2_amd import backend, neuromancer as nm
    nm.model_manager.reset()
    mu = nm.Input((2, 3, 4, 5, 6), 'b,f,z,x,y', name='mu')
    with pytest.raises(ValueError, match="equal shapes"):
        nm.GaussianRV(mu, nm.Input((2, 4, 4, 5, 6), 'b,f,z,x,y', name='ls4'))
    ls = nm.Input_like(mu, name='ls')
    for make in (lambda: nm.GaussianRV(mu, ls, n_samples=3), lambda: nm.GaussianAEVBPrior(mu, ls, 2)):
        with pytest.raises(NotImplementedError, match="'s' sample axis"):
            make()
    with pytest.raises(NotImplementedError, match="are supported"):
        nm.GaussianRV(nm.Input((2, 3, 4), 'b,f,x', name='m1'), nm.Input((2, 3, 4), 'b,f,x', name='l1'))
    with pytest.raises(ValueError, match="mixes at most 8"):
        nm.AggregateLoss([nm.GaussianRV(mu, ls, name='z%d' % k).make_priorlayer() for k in range(9)])
    assert {"e2_gaussrv_fwd", "e2_gaussrv_bwd", "e2_aevb_prior_fwd",
            "e2_aevb_prior_bwd"} <= set(backend.EXPORTED_SYMBOLS)
