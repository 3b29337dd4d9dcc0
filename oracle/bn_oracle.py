"""TEST INFRASTRUCTURE ONLY (imported by tests/ alone; never by the product).

Batch normalisation + activation (csrc/dense_bn.hip: e2_batchnorm_act_fwd / _bwd) and the
Perceptron's dot product (e2_dense_fwd / dgrad / wgrad) restated in closed form with NumPy --
forward AND backward written out by hand, nothing taken from autograd (tests/test_batchnorm_host.py
pins these formulas against torch float64 autograd of oracle/mnist_oracle.py's ``batchnorm`` and
against a plain loop over channels).  The tensors are (n, f, *spatial); the statistics run over
every axis but ``f`` (axis 1).

Forward (neural.py:681-711, 352-378 of the reference)
    train:   mean_c = E[x],  s0_c = sqrt(E[(x - mean)^2])  (population),  std_c = s0_c + 1e-6
    predict: mean_c, std_c are the stored statistics
    pre = (gamma / std) x + b - gamma mean / std,   out = act(pre),   act in {'lin', 'relu'}
    save = (mean, std) -- the std INCLUDING the 1e-6
    running statistics (train, as extra updates of a step function):
        m <- 0.9995 m + 0.0005 mean,   s <- 0.9995 s + 0.0005 std

Backward, with xhat = (x - mean) / std and dpre = dout * act'(pre), relu'(0) = 0.5
(computations.py:81-82: relu(x) = 0.5 (x + |x|)):
    dbias_c  = sum dpre,     dgamma_c = sum dpre xhat
    predict: dx = (gamma / std) dpre                               (the statistics are constants)
    train:   dx = (gamma / std) (dpre - E[dpre] - xhat E[dpre xhat] std / s0)
             from d mean / d x_i = 1 / cnt and d s0 / d x_i = (x_i - mean) / (cnt s0)

THE CONSTANT-CHANNEL RULE IS THE PROJECT'S CHOICE.  Where the variance of a channel is exactly 0
(every element equal, or cnt = 1) the symbolic gradient of the reference is 0 * inf: xhat = 0 and
d s0 / d x = 0 / 0.  The kernel takes the term through the standard deviation as 0 there,
    dx = (gamma / std) (dpre - E[dpre]),
which is the limit of the train formula along any direction that keeps the channel constant, and
this file states the same rule; no reference number exists for it.

Every function computes in ``dtype``: float64 gives the reference, float32 a restatement of the
same arithmetic in the kernels' precision (NumPy's pairwise sums, not the kernels' order) that the
GPU tests derive their computed bounds from.  ``one_pass=True`` replaces the two-pass variance by
E[x^2] - mean^2 -- the rewrite the offset-input test exists to catch, never a reference.
"""
import numpy as np

EPS = 1e-6
MOMENTUM = 0.0005


def _bsh(x):
    return (1, -1) + (1,) * (x.ndim - 2)


def _red(x):
    return (0,) + tuple(range(2, x.ndim))


def batch_stats(x, dtype=np.float64, one_pass=False):
    """(mean, bare standard deviation s0, std = s0 + 1e-6) per channel, computed in ``dtype``"""
    x = np.asarray(x, dtype)
    red = _red(x)
    cnt = dtype(np.prod([x.shape[i] for i in red]))
    mean = (x.sum(axis=red, dtype=dtype) / cnt).astype(dtype)
    if one_pass:
        var = ((x * x).sum(axis=red, dtype=dtype) / cnt - mean * mean).astype(dtype)
        var = np.maximum(var, dtype(0))
    else:
        d = x - mean.reshape(_bsh(x))
        var = ((d * d).sum(axis=red, dtype=dtype) / cnt).astype(dtype)
    s0 = np.sqrt(var).astype(dtype)
    return mean, s0, (s0 + dtype(EPS)).astype(dtype)


def act_slope(pre, act):
    if act == 'lin':
        return np.ones_like(pre)
    assert act == 'relu', act
    one, half, zero = pre.dtype.type(1), pre.dtype.type(0.5), pre.dtype.type(0)
    return np.where(pre > 0, one, np.where(pre == 0, half, zero))


def forward(x, gamma, bias, act='relu', stats=None, dtype=np.float64, one_pass=False):
    """``stats`` None: train mode; else (mean, std): predict mode with those statistics.
    Returns dict(out, pre, mean, s0, std, save); s0 is None in predict mode."""
    x = np.asarray(x, dtype)
    g, b = np.asarray(gamma, dtype), np.asarray(bias, dtype)
    if stats is None:
        mean, s0, std = batch_stats(x, dtype, one_pass)
    else:
        mean, std, s0 = np.asarray(stats[0], dtype), np.asarray(stats[1], dtype), None
    sh = _bsh(x)
    pre = (g / std).reshape(sh) * x + (b - g * mean / std).reshape(sh)
    out = pre if act == 'lin' else np.maximum(pre, dtype(0))
    assert act in ('lin', 'relu'), act
    return dict(out=out, pre=pre, mean=mean, s0=s0, std=std, save=np.concatenate([mean, std]))


def running_update(run_mean, run_std, mean, std, dtype=np.float64):
    """the extra updates of a step function; ``std`` includes the 1e-6"""
    keep, new = dtype(1 - MOMENTUM), dtype(MOMENTUM)
    return (keep * np.asarray(run_mean, dtype) + new * np.asarray(mean, dtype),
            keep * np.asarray(run_std, dtype) + new * np.asarray(std, dtype))


def backward(dout, x, gamma, bias, mean, std, train, act='relu', dtype=np.float64, s0=None):
    """(dx, dgamma, dbias) from the statistics the forward used (``save``).  ``s0``: the bare
    standard deviation of a train-mode forward (default std - 1e-6, as the kernel recovers it)."""
    x, dout = np.asarray(x, dtype), np.asarray(dout, dtype)
    g, b = np.asarray(gamma, dtype), np.asarray(bias, dtype)
    mean, std = np.asarray(mean, dtype), np.asarray(std, dtype)
    sh, red = _bsh(x), _red(x)
    cnt = dtype(np.prod([x.shape[i] for i in red]))
    a = g / std
    pre = a.reshape(sh) * x + (b - g * mean / std).reshape(sh)
    dpre = dout * act_slope(pre, act)
    xhat = (x - mean.reshape(sh)) / std.reshape(sh)
    dbias = dpre.sum(axis=red, dtype=dtype)
    dgamma = (dpre * xhat).sum(axis=red, dtype=dtype)
    if not train:
        return a.reshape(sh) * dpre, dgamma, dbias
    s0 = (std - dtype(EPS)) if s0 is None else np.asarray(s0, dtype)
    live = s0 > 0                                    # the constant-channel rule (module docstring)
    m_dx = np.where(live, (dgamma / cnt) * (std / np.where(live, s0, dtype(1))), dtype(0))
    dx = a.reshape(sh) * (dpre - (dbias / cnt).reshape(sh) - xhat * m_dx.reshape(sh))
    return dx.astype(dtype), dgamma, dbias


def fwd_bwd(x, gamma, bias, dout, act='relu', stats=None, dtype=np.float64, one_pass=False):
    """one forward and its backward; dict of forward() plus dx, dgamma, dbias"""
    r = forward(x, gamma, bias, act, stats, dtype, one_pass)
    r['dx'], r['dgamma'], r['dbias'] = backward(dout, x, gamma, bias, r['mean'], r['std'],
                                                stats is None, act, dtype, s0=r['s0'])
    return r


def numpy_loop_forward(x, gamma, bias, act='relu'):
    """train-mode forward channel by channel with Python sums (shares no code with the above)"""
    x = np.asarray(x, np.float64)
    out = np.empty_like(x)
    mean, std = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    for c in range(x.shape[1]):
        vals = [float(v) for n in range(x.shape[0]) for v in x[n, c].ravel()]
        m = sum(vals) / len(vals)
        s = (sum((v - m) ** 2 for v in vals) / len(vals)) ** 0.5 + EPS
        mean[c], std[c] = m, s
        for n in range(x.shape[0]):
            y = float(gamma[c]) / s * x[n, c] + float(bias[c]) - float(gamma[c]) * m / s
            out[n, c] = np.maximum(y, 0) if act == 'relu' else y
    return out, mean, std


# ---- the Perceptron's sums in the kernels' order -----------------------------------------------
def dense_f32_sequential(a, b, base=None):
    """a (p, q) . b (q, r) in float32 with the kernels' arithmetic: one accumulator per output,
    acc <- fma(a[i, t], b[t, j], acc) for t = 0 .. q - 1 in order (the product of two float32 is
    exact in float64; the sum is rounded to float32 once per term), then ``base + acc`` where the
    launch accumulates.  What the long-k bound of the GPU test is derived from."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for t in range(a.shape[1]):
        acc = (a[:, t:t + 1].astype(np.float64) * b[t:t + 1, :].astype(np.float64)
               + acc.astype(np.float64)).astype(np.float32)
    return acc if base is None else (np.asarray(base, np.float32) + acc).astype(np.float32)
