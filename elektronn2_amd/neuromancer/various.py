"""The stochastic nodes of elektronn2/neuromancer/various.py that make a conv net a variational
autoencoder (various.py:32-151):

``GaussianRV(mu, log_sig)`` -- the re-parameterised sample z = mu + exp(log_sig) * eps with
eps ~ N(0, 1) -- and ``GaussianAEVBPrior``, made by ``GaussianRV.make_priorlayer()``: the KL term
0.5 (mu^2 + sig^2 - 1 - 2 log_sig), one more element-wise term of an ``AggregateLoss`` beside the
reconstruction loss.

Device side (csrc/gauss_rv.hip; the noise contract is in include/e2hip.h): eps comes from the
counter-based generator of the dropout gates, one Philox block per four elements.  The backward pass
makes it again from the same (seed, counter, stream) instead of reading a stored copy.  The model
owns the generator state and the plan issues its one tick per step, shared with dropout
(``Model.set_dropout_seed`` seeds both).  As in the reference the node samples in EVERY function
that evaluates it, prediction included: it has no mean-only mode.

``mu`` and ``log_sig`` may be two nodes (two Perceptron heads on one trunk) or the two ``split``
parts of one node (a ``(1,1,1)`` Conv to 2F features): the kernels then read and write channel
slices of one buffer.  ``n_samples > 0`` (the ``'s'`` sample axis) raises NotImplementedError, as
that axis does for every loss node.
"""
from __future__ import annotations

from .node_basic import Node
from .loss import _ElementLoss

__all__ = ['GaussianRV', 'GaussianAEVBPrior']

_TAG_FORMS = (('b', 'f'), ('b', 'f', 'x', 'y'), ('b', 'f', 'y', 'x'), ('b', 'f', 'z', 'x', 'y'))


def _check_parents(who, mu, log_sig, n_samples):
    if n_samples:
        raise NotImplementedError("%s: n_samples > 0 adds the 's' sample axis, which is outside "
                                  "the HIP hot path" % who)
    tags = tuple(mu.shape.tags)
    if tags not in _TAG_FORMS:
        raise NotImplementedError("%s: parents of %s; 'b,f', 'b,f,x,y' / 'b,f,y,x' and 'b,f,z,x,y' "
                                  "are supported" % (who, ",".join(tags)))
    if tuple(log_sig.shape.shape) != tuple(mu.shape.shape) or tuple(log_sig.shape.tags) != tags:
        raise ValueError("%s: mu and log_sig must have equal shapes, got %s and %s"
                         % (who, mu.shape, log_sig.shape))


def _slots(plan, mu, log_sig):
    """((dmu, accumulate), (dlog_sig, accumulate)): each parent's output gradient (None: not
    wanted) and whether it already holds another consumer's contribution"""
    out = []
    for n in (mu, log_sig):
        if plan.needs_grad(n):
            g, first = plan.grad_slot(n)
            out.append((g, not first))
        else:
            out.append((None, False))
    return out


class GaussianRV(Node):
    """various.py:32-106.  A sample from separable Gaussians of mean ``mu`` and standard deviation
    exp(``log_sig``); differentiable wrt both through the re-parameterisation."""
    _writes_part_grad = True        # (its backward writes any strided gradient view: SplitPart)

    def __init__(self, mu, log_sig, n_samples=0, name="state", print_repr=True):
        super(GaussianRV, self).__init__((mu, log_sig), name, print_repr)
        self.mu = mu
        self.log_sig = log_sig
        self.n_samples = n_samples
        _check_parents(type(self).__name__, mu, log_sig, n_samples)

    def _calc_shape(self):
        self.shape = self.parent[0].shape.copy()

    def _calc_comp_cost(self):
        self.computational_cost = self.parent[0].shape.stripnone_prod

    def make_priorlayer(self):
        """the node that computes the Auto-Encoding-Variational-Bayes prior of this one
        (various.py:98-106): a term of an AggregateLoss"""
        return GaussianAEVBPrior(self.mu, self.log_sig, self.n_samples, name=self.name + "_prior")

    def _plan_alloc(self, plan):
        for n in self.parent:
            if plan.out.get(n) is None:
                raise NotImplementedError("GaussianRV: the output of '%s' is not materialised by "
                                          "the plan" % (n.name,))
        plan.alloc_out(self)

    def _plan_fwd(self, plan):
        plan.ctx.gaussrv_fwd(plan.out[self.mu], plan.out[self.log_sig], plan.out[self],
                             plan.model.dropout_state_dev(), plan.dropout_stream(self))

    def _plan_bwd(self, plan):
        (dm, am), (ds, asg) = _slots(plan, self.mu, self.log_sig)
        if dm is None and ds is None:
            return
        plan.ctx.gaussrv_bwd(plan.grad[self], plan.out[self.log_sig], dm, ds,
                             plan.model.dropout_state_dev(), plan.dropout_stream(self),
                             acc_mu=am, acc_sig=asg)


class GaussianAEVBPrior(_ElementLoss):
    """various.py:111-151.  0.5 (mu^2 + exp(2 log_sig) - 1 - 2 log_sig) per element: an L2 norm on
    ``mu`` and a constraint on sigma that favours 1 and goes to infinity for sigma -> 0.  Made by
    ``GaussianRV.make_priorlayer()``.  In the mix it is a plain mean over all elements, as
    GaussianNLL is; launches of its own (e2_aevb_prior_fwd / e2_aevb_prior_bwd)."""
    kind = 'gauss_nll'        # (its row of e2_loss_mix: L = S1 / n_tot)
    _writes_part_grad = True

    def __init__(self, mu, log_sig, n_samples=0, name="prior", print_repr=True):
        super(GaussianAEVBPrior, self).__init__((mu, log_sig), name, print_repr)
        self.mu = mu
        self.pred = mu
        self.log_sig = log_sig
        self.n_samples = n_samples
        self._last_plan = None
        _check_parents(type(self).__name__, mu, log_sig, n_samples)

    def _calc_shape(self):
        self.shape = self.parent[0].shape.copy()

    def _plan_fwd(self, plan):
        plan.ctx.aevb_prior_fwd(plan.out[self.mu], plan.out[self.log_sig],
                                plan.scratch[self, 'partials'])

    def _plan_bwd(self, plan):
        agg = plan.scratch.get((self, 'agg'))
        if agg is None:
            raise NotImplementedError("GaussianAEVBPrior '%s' outside an AggregateLoss has no "
                                      "gradient" % (self.name,))
        node, k = agg
        (dm, am), (ds, asg) = _slots(plan, self.mu, self.log_sig)
        if dm is None and ds is None:
            return
        plan.ctx.aevb_prior_bwd(plan.out[self.mu], plan.out[self.log_sig],
                                plan.scratch[node, 'coef'][k:k + 1], dm, ds, acc_mu=am, acc_sig=asg)
