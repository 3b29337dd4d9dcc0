"""Softmax / MultinoulliNLL / SquaredLoss / AbsLoss / BinaryNLL / GaussianNLL / AggregateLoss /
Errors with the reference's constructor signatures (elektronn2/neuromancer/loss.py:33-93,
141-351, 693-826, 829-887, 953-1101, 1215-1370).

HIP execution covers the pattern every BASELINE config uses:
``AggregateLoss(MultinoulliNLL(Softmax(lin-Conv), target, target_is_sparse=True))``
which reduces to  loss = sum_labelled -log(p_target + 1e-5) / (n_labelled + 1e-5)
(the pred.size / n_class / mean factors of loss.py:342-346,1357-1363 cancel), and its
weighted form (loss.py:172-212, 261-347): ``class_weights`` (a sequence -> a non-trainable
parameter the kernels read in place, or an ``Input((n_class,), 'f')``), ``example_weights``
(an Input of the target's shape without the class axis) and the lazy-labelling masks
``mask_class_labeled`` / ``mask_class_not_present`` (Inputs ``(b, n_class)``):
    loss = (-sum T w e log(p + eps) - sum M w e log(1 - p + eps)) / (sum T + S sum M + eps),
    T = onehot(target) * mask_class_labeled, M = mask_class_not_present, S = positions per item.
The weight Inputs are ordinary inputs of the loss node: extra positional arguments of
``trainingstep(data, target, *extras)`` in the order of ``loss_node.input_nodes``, slices of the
plan's input arena (and of an input-ring slot).  Whichever kernel the plan chose for the loss --
the fused tail (csrc/tail.hip), the fused head (csrc/head.hip) or the generic pair
(csrc/softmax_nll.hip) -- takes the weights (the ``_w`` entry points of include/e2hip.h).
The weighted tail launch is f32 only: in bf16 mode (``set_mfma_dtype('bf16')``) a neuro3d-style net
with a weighted loss needs the plan option ``bf16_tail`` off (the separate kernels then run; the
choice of the path never depends on the weights, so the launch reports an error otherwise).
Weak training and dense targets are outside the hot path and raise NotImplementedError.

``Softmax(n_indep = E > 1)`` (independent softmaxes over consecutive feature groups,
loss.py:82-92) trains under ``MultinoulliNLL(..., target_is_sparse=True)`` with a target
``(b, E, spatial...)`` -- what ``data.PatchSampler.getbatch(affinities='affinity')`` returns --
(loss.py:275-285, 338-346):
    loss = sum over the labelled (item, group, position) of -log(p_target + 1e-5)
           / (n_labelled + 1e-5),      ONE count over all groups,
one forward and one backward launch for all groups (csrc/softmax_nll.hip).  The fused head and
tail step aside for such a softmax; class / example weights and the class masks with
``n_indep > 1`` raise NotImplementedError (the reference broadcasts a length-n_class vector
against E * n_class features).  ``Errors`` of such a net compares the argmax inside each group
(loss.py:737-748).  The same Softmax also serves ``MalisNLL`` (loss.py:560-690):
forward and gradient on the device, the MALIS counts by the host C++ of csrc/malis.cpp between
the forward and the backward segment of the step.

Element-wise losses (csrc/loss_elem.hip): ``SquaredLoss``, ``AbsLoss``, ``BinaryNLL``,
``GaussianNLL`` over any prediction node whose output the plan materialises (a Conv with any
activation, UpConv, Perceptron, a Concat ...), with a target of the prediction's shape, and
``AggregateLoss`` over 1..8 of them with ``mixing_weights``:
    total = (1/K) sum_k w_k L_k,   L_k as in the table of include/e2hip.h ("element-wise losses").
Each term is one forward launch that leaves per-work-group sums in a slab; the AggregateLoss node
owns one small launch that turns the slabs into the term values, the labelled counts, the gradient
coefficients and the total; each term's backward launch writes (or adds to) its prediction's output
gradient.  ``margin``, ``scale_correction`` and ``mixing_weights`` are non-trainable parameters the
kernels read in place.  Mixing these with a MultinoulliNLL / MalisNLL raises NotImplementedError
(their fused launches take no scale), and so does the ``'s'`` sample axis.

The rest of the reference's loss nodes (loss.py:96-138, 890-950, 1104-1212), terms of the same mix:
``BetaNLL(mode, concentration, target)``, the negative log density of a Beta distribution, is an
element-wise loss with entry points of its own (e2_beta_nll_fwd / e2_beta_nll_bwd, csrc/
loss_elem.hip, with an f32 digamma for the gradient) and a plain mean over all elements, like
GaussianNLL; ``mode`` and ``concentration`` are used as given (c > 2, 0 < m < 1 is the caller's
business: a 'sigmoid' head, a 'soft+' head plus an offset).  ``EuclideanDistance(pred, target)``
(the L2 norm over the feature axis, NaN as 0) and ``RampLoss(d_low, d_big, margin=...)`` (the hinge
mean_f max(d_low - d_big + margin, 0): over two distances the triplet loss) are ordinary nodes with
a ONE-feature output the plan materialises (csrc/loss_map.hip); both parents of either may be
network branches and receive gradients.  As a parent of an ``AggregateLoss`` such a map is one
more term: the aggregate sums it into a slab (e2_mean_fwd) in front of its mix launch and writes
coef_k into the map's gradient (e2_mean_bwd) ahead of the map's own backward;
``term_value`` / ``n_labelled`` (all elements of the map) work as for the others.  Where a distance
is 0, or was a NaN, its gradient is an exact 0 in every feature (the reference: 0/0).
``OneHot(target, n_class)`` turns a class-id target into ``n_class`` features of 0 / 1 (exact
equality, no gradient): the target of a SquaredLoss / BinaryNLL over an n_class-feature
prediction.  ``BlockedMultinoulliNLL`` is not provided: the reference's computes MultinoulliNLL.

Multi-task nets: ``AggregateLoss`` over 2..8 distinct ``MultinoulliNLL`` terms (sparse targets,
``n_indep = 1``, unweighted), each over a ``Softmax`` of its own -- usually K ``(1,1,1)`` 'lin' heads
on one trunk, the targets cut from one Input by ``node_basic.split`` -- is the form ``multi_nll``:
    L_k = sum_labelled -log(p_target + 1e-5) / (N_k + 1e-5),   each term its OWN count N_k,
    total = (1/K) sum_k w_k L_k;  a term with nothing labelled is 0, has a zero gradient, counts in K.
The aggregate owns the launches: all heads, softmaxes, sums and gradients in one launch pair
(csrc/multihead.hip; plan option ``fuse_multihead``, every head Conv of the classifier-head form on
one trunk, sum of the classes <= 16) or, all-or-none, the heads as ordinary conv launches and the
generic pair e2_nll_multi_fwd / e2_nll_multi_bwd over their logits (csrc/softmax_nll.hip); between
them one small launch (e2_nll_mix) that reads ``mixing_weights`` on the device.  After a step each
term's ``term_value`` / ``n_labelled`` hold its L_k and N_k.  Any other list that contains a
MultinoulliNLL / MalisNLL raises as before.
"""
from __future__ import annotations

import numpy as np

from .graphutils import TaggedShape, floatX
from .node_basic import Node, Sym
from .variables import VariableParam

__all__ = ['Softmax', 'MultinoulliNLL', 'MalisNLL', 'SquaredLoss', 'AbsLoss', 'BinaryNLL',
           'GaussianNLL', 'BetaNLL', 'OneHot', 'EuclideanDistance', 'RampLoss', 'AggregateLoss',
           'Classification', 'Errors']

MAX_LOSS_TERMS = 8     # E2_MAX_LOSS_TERMS of include/e2hip.h

EPS = 1e-5     # loss.py:30


class Softmax(Node):
    def __init__(self, parent, n_class='auto', n_indep=1, name="softmax", print_repr=True):
        super(Softmax, self).__init__(parent, name, print_repr)
        n_f = parent.shape['f']
        if hasattr(parent, 'activation_func'):
            if parent.activation_func != 'lin':
                raise ValueError("The parent of a Softmax-node must have a "
                                 "linear activation function.")
        if n_class == 'auto':
            if n_f % n_indep == 0:
                n_class = n_f // n_indep
            else:
                raise ValueError("Cannot create %i-fold %i-class softmax from %i features."
                                 % (n_indep, n_f // n_indep, n_f))
        elif n_class * n_indep != n_f:
            raise ValueError("Cannot create %i-fold %i-class softmax " % (n_indep, n_class))
        self.n_class = n_class
        self.n_indep = n_indep

    def _calc_comp_cost(self):
        self.computational_cost = self.parent.shape.stripnone_prod

    def _plan_alloc(self, plan):
        plan.alloc_out(self)
        plan.scratch[self, 'stats'] = plan.zeros_flat(2)
        plan.scratch[self, 'dummy_t'] = None

    def _plan_fwd(self, plan):
        # probs only; when an NLL node hangs on this softmax it re-runs the same
        # kernel with the target and also fills the loss statistics.
        if plan.scratch.get((self, 'fused_nll')):
            agg = self._multi_agg(plan)
            if agg is not None and agg._last_softmax(plan) is self:
                # several NLL terms under one aggregate: its forward launch writes every term's
                # probabilities.  It is issued HERE, where the last of its softmaxes stands in
                # the plan -- behind every head's logits, in front of every reader of the
                # probabilities (a Concat prediction, Errors), whatever the order of the outputs
                agg._emit_fwd(plan)
            return
        head = self._head(plan)
        if head is not None:                 # conv + softmax in one kernel
            plan.ctx.head_fwd(plan.out[head.parent], plan.param(head.w), plan.param(head.b),
                              None, plan.out[self], None)
            return
        t = plan.scratch.get((self, 'dummy_t'))
        if t is None:
            sh = list(plan.out_shape(self))
            sh[1] = 1
            t = plan.full(tuple(sh), -1.0)
            plan.scratch[self, 'dummy_t'] = t
        lg, pr, k = plan.out[self.parent], plan.out[self], self.n_class
        for i in range(self.n_indep):            # loss.py:82-92: one softmax per group
            sl = slice(i * k, (i + 1) * k)
            plan.ctx.softmax_nll_fwd(lg[:, sl], t, pr[:, sl], plan.scratch[self, 'stats'])

    def _head(self, plan):
        """the parent Conv when it runs as a fused classifier head (csrc/head.hip)"""
        p = self.parent
        f = getattr(p, '_fused_head', None)
        return p if (f is not None and f(plan) is self) else None

    def _multi_agg(self, plan):
        """the AggregateLoss of this plan that has a MultinoulliNLL over this softmax as one of
        several terms -- its launches then make the probabilities, the loss and the gradient --
        or None"""
        for c in self.children.values():
            if isinstance(c, MultinoulliNLL) and c._multi(plan) is not None:
                return c._multi(plan)[0]
        return None

    def _plan_bwd(self, plan):
        if plan.scratch.get((self, 'fused_nll')) or plan.scratch.get((self, 'loss_writes_dlogits')):
            return            # the NLL node wrote d(loss)/d(logits) directly
        raise NotImplementedError("gradient through a bare Softmax node")


class MultinoulliNLL(Node):
    def __init__(self, pred, target, target_is_sparse=False, class_weights=None,
                 example_weights=None, weakness=0, mask_class_labeled=None,
                 mask_class_not_present=None, name="nll", print_repr=True):
        parents = [pred, target]              # (parent order: loss.py:218-235)
        cw_param = None
        if class_weights is not None:
            if isinstance(class_weights, Node):
                parents.append(class_weights)
            else:
                cw_param = VariableParam(value=np.array(class_weights, dtype=floatX),
                                         name="class_weights", dtype=floatX,
                                         apply_train=False)
        for extra in (example_weights, mask_class_labeled, mask_class_not_present):
            if extra is not None:
                if not isinstance(extra, Node):
                    raise ValueError("example_weights and the class masks must be Nodes")
                parents.append(extra)
        super(MultinoulliNLL, self).__init__(parents, name, print_repr)
        if not isinstance(pred, Softmax):
            raise ValueError("The prob input to a MultinoulliNLL-node must be "
                             "a Softmax-Node.")
        if pred.n_indep != 1 and (len(parents) > 2 or cw_param is not None):
            # (the reference broadcasts a length-n_class vector against n_indep * n_class features)
            raise NotImplementedError("MultinoulliNLL over n_indep > 1 takes the plain sparse "
                                      "target only: the other options have no defined meaning "
                                      "for several independent softmaxes")
        if weakness:
            raise NotImplementedError("weak training (weakness != 0) is outside the HIP "
                                      "hot path")
        if not target_is_sparse:
            raise NotImplementedError("dense (one-hot) targets are outside the HIP hot path")
        self.target = target
        self.pred = pred
        self.axis = pred.shape.tag2index('f')
        self.n_class = pred.n_class
        self.n_indep = pred.n_indep
        self.target_is_sparse = target_is_sparse
        k = self.n_class
        if self.n_indep != 1:
            want = tuple(self.n_indep if t == 'f' else s
                         for s, t in zip(pred.shape.shape, pred.shape.tags))
            if tuple(target.shape.tags) != tuple(pred.shape.tags) or \
                    tuple(target.shape.shape) != want:
                raise ValueError("MultinoulliNLL over %i independent softmaxes: the sparse target "
                                 "must be %s (one class id per softmax) for the prediction %s, "
                                 "got %s" % (self.n_indep, want, pred.shape, target.shape))
        if cw_param is not None:
            if cw_param.shape != (k,):
                raise ValueError("class_weights: %i values given, the prediction has %i "
                                 "classes" % (int(np.prod(cw_param.shape)), k))
            self.params['class_weights'] = cw_param
            class_weights = cw_param
        elif class_weights is not None:
            if tuple(class_weights.shape.tags) != ('f',) or \
                    tuple(class_weights.shape.shape) != (k,):
                raise ValueError("class_weights node: an Input((%i,), 'f') is needed, got %s"
                                 % (k, class_weights.shape))
        for what, m in (('mask_class_labeled', mask_class_labeled),
                        ('mask_class_not_present', mask_class_not_present)):
            if m is not None and (tuple(m.shape.tags) != ('b', 'f') or m.shape['f'] != k
                                  or m.shape['b'] != pred.shape['b']):
                raise ValueError("%s: an Input((%r, %i), 'b,f') is needed, got %s"
                                 % (what, pred.shape['b'], k, m.shape))
        if example_weights is not None:
            tags = tuple(t for t in pred.shape.tags if t != 'f')
            shape = tuple(s for s, t in zip(pred.shape.shape, pred.shape.tags) if t != 'f')
            if tuple(example_weights.shape.tags) != tags or \
                    tuple(example_weights.shape.shape) != shape:
                raise ValueError("example_weights: an Input(%s, '%s') is needed (the target's "
                                 "shape without the class axis), got %s"
                                 % (shape, ",".join(tags), example_weights.shape))
        self.class_weights = class_weights
        self.example_weights = example_weights
        self.weakness = 0
        self.mask_class_labeled = mask_class_labeled
        self.mask_class_not_present = mask_class_not_present
        self._last_plan = None

    def _multi(self, plan):
        """(aggregate, k): this node is term k of an ``AggregateLoss`` of the ``multi_nll`` form
        that belongs to this plan -- the aggregate then owns every launch of the term -- else
        None"""
        key = (self, 'multi')
        if key not in plan.scratch:
            r = None
            for c in self.children.values():
                if getattr(c, 'multi_nll', False) and any(n is c for n in plan.nodes):
                    r = (c, [i for i, p in enumerate(c.parent) if p is self][0])
                    break
            plan.scratch[key] = r
        return plan.scratch[key]

    def _mix_value(self, what):
        plan = self._last_plan
        agg = None if plan is None else plan.scratch.get((self, 'multi'))
        if agg is None:
            return None
        plan.stream.synchronize()
        return plan.scratch[agg[0], what][agg[1]].item()

    @property
    def term_value(self):
        """as a term of a multi-NLL AggregateLoss: this term's L of the last step / evaluation,
        before the mixing weight (None before the first, and for a single loss)"""
        v = self._mix_value('term_loss')
        return None if v is None else np.float32(v)

    @property
    def n_labelled(self):
        """as a term of a multi-NLL AggregateLoss: labelled target positions of the last step /
        evaluation (None before the first, and for a single loss)"""
        v = self._mix_value('count')
        return None if v is None else int(round(v))

    @property
    def weighted(self):
        return any(v is not None for v in (self.class_weights, self.example_weights,
                                           self.mask_class_labeled,
                                           self.mask_class_not_present))

    def _weights(self, plan):
        """the e2_nll_weights descriptor of this plan (None: the unweighted entry points).  It
        names device buffers -- the class-weight parameter's slice of the parameter arena, the
        weight Inputs' slices of the input arena -- that the kernels read when they run: new
        values need no new capture."""
        if not self.weighted:
            return None
        w = plan.scratch.get((self, 'weights'))
        if w is None:
            from .. import backend
            cw = self.class_weights
            if isinstance(cw, VariableParam):
                cw = plan.param(cw).reshape(-1)
            elif cw is not None:
                cw = plan.out[cw].reshape(-1)
            dev = lambda node: None if node is None else plan.out[node]
            lab, npr = dev(self.mask_class_labeled), dev(self.mask_class_not_present)
            w = backend.nll_weights(class_w=cw, example_w=dev(self.example_weights),
                                    labelled=None if lab is None else lab.reshape(lab.shape[0], -1),
                                    not_present=None if npr is None else npr.reshape(npr.shape[0], -1))
            plan.scratch[self, 'weights'] = w
        return w

    def _calc_shape(self):
        self.shape = self.parent[0].shape.updateshape(self.axis, 1)

    def _calc_comp_cost(self):
        self.computational_cost = self.parent[0].shape.stripnone_prod

    def _plan_alloc(self, plan):
        plan.scratch[self.pred, 'fused_nll'] = True
        if self._multi(plan) is not None:     # (the aggregate allocates and launches)
            plan.out[self] = None
            return
        plan.scratch[self, 'loss'] = plan.zeros_flat(1)
        head = self.pred._head(plan)
        if head is not None and plan.training and self._tail(plan) is None:
            nb = plan.ctx.head_bwd_ws_bytes(plan.out_shape(head.parent), self.n_class)
            plan.scratch[self, 'head_ws'] = plan.empty_flat(nb // 4 + 16)
        plan.out[self] = None        # the element-wise nll array is never materialised

    def _tail(self, plan):
        """the (1,1,1) relu Conv in front of the fused head when the pair runs as ONE launch,
        forward and backward (csrc/tail.hip, Conv._tail), else None"""
        head = self.pred._head(plan)
        if head is None:
            return None
        c = head.parent
        f = getattr(c, '_tail', None)
        t = f(plan) if f is not None else None
        return c if (t is not None and t[2] is self) else None

    def _plan_fwd(self, plan):
        if self._multi(plan) is not None:
            return
        stats = plan.scratch[self.pred, 'stats']
        tail = self._tail(plan)
        if tail is not None:
            # forward AND backward of [1x1x1 conv + relu] -> head -> loss: probabilities,
            # stats[1] = #labelled, the conv's pre-activation gradient, its parent's output
            # gradient; the partial sums wait in the workspace for the backward half
            head = self.pred._head(plan)
            par = tail.parent
            plan.join_side()
            dx = plan.grad[par] if plan.needs_grad(par) else None
            gm = tail._tail_gm(plan) if dx is not None else None
            kw = {}
            if gm is not None:
                # the parent's activation backward rides along: the launch writes the parent's
                # zero-padded gradient buffer (interior) and its bias gradient's slots
                dx = plan.scratch[par, 'dy']
                kw = dict(gm_mode=gm[0], gm_src=gm[1], gm_bias=gm[2])
            with plan.loss_grad_mode():
                plan.scratch[self, 'tail_slots'] = plan.ctx.tail_fwd_bwd(
                    plan.out[par], plan.scratch[tail, 'wp_f'], plan.scratch.get((tail, 'wp_d')),
                    plan.param(tail.b), plan.param(head.w).reshape(head.n_f, -1),
                    plan.param(head.b), plan.out[self.target], plan.out[self.pred],
                    plan.scratch[tail, 'dy'], dx, stats, plan.scratch[tail, 'tail_ws'],
                    weights=self._weights(plan), **kw)
            return
        plan.zero_early(stats)
        head = self.pred._head(plan)
        if head is not None:
            plan.ctx.head_fwd(plan.out[head.parent], plan.param(head.w), plan.param(head.b),
                              plan.out[self.target], plan.out[self.pred], stats,
                              weights=self._weights(plan))
            return
        if self.n_indep != 1:                # every group in one launch (csrc/softmax_nll.hip)
            plan.ctx.softmax_nll_grouped_fwd(plan.out[self.pred.parent], plan.out[self.target],
                                             plan.out[self.pred], self.n_indep, stats)
            return
        plan.ctx.softmax_nll_fwd(plan.out[self.pred.parent], plan.out[self.target],
                                 plan.out[self.pred], stats, weights=self._weights(plan))

    def _plan_bwd(self, plan):
        if self._multi(plan) is not None:
            return
        with plan.loss_grad_mode():
            self._plan_bwd_launches(plan)

    def _plan_bwd_launches(self, plan):
        head = self.pred._head(plan)
        tail = self._tail(plan)
        if tail is not None:
            # (behind the zero fill of the gradient arena: the slots are ADDED into it)
            par = tail.parent
            gm = tail._tail_gm(plan) if plan.needs_grad(par) else None
            plan.ctx.tail_reduce(plan.scratch[tail, 'tail_ws'], plan.scratch[self, 'tail_slots'],
                                 tail.n_f, head.n_f, plan.pgrad(head.w).reshape(head.n_f, -1),
                                 plan.pgrad(head.b), plan.pgrad(tail.b),
                                 plan.scratch[self.pred, 'stats'], plan.scratch[self, 'loss'],
                                 db_parent=plan.pgrad(par.b) if gm is not None else None)
            return
        if head is not None:
            dst, first = (plan.grad_slot(head.parent) if plan.needs_grad(head.parent)
                          else (None, True))
            plan.ctx.head_bwd(plan.out[head.parent], plan.param(head.w), plan.out[self.pred],
                              plan.out[self.target], plan.scratch[self.pred, 'stats'], dst,
                              not first, plan.pgrad(head.w), plan.pgrad(head.b),
                              plan.scratch[self, 'loss'], ws=plan.scratch[self, 'head_ws'],
                              weights=self._weights(plan))
            return
        logits = self.pred.parent
        dst, first = plan.grad_slot(logits)
        if not first:
            raise NotImplementedError("logits consumed by several nodes")
        if self.n_indep != 1:
            plan.ctx.softmax_nll_grouped_bwd(plan.out[self.pred], plan.out[self.target],
                                             self.n_indep, plan.scratch[self.pred, 'stats'], dst,
                                             plan.scratch[self, 'loss'])
            return
        plan.ctx.softmax_nll_bwd(plan.out[self.pred], plan.out[self.target],
                                 plan.scratch[self.pred, 'stats'], dst,
                                 plan.scratch[self, 'loss'], weights=self._weights(plan))

    def loss_value(self, plan):
        """device scalar: loss_sum / (n_labelled + EPS)  (weighted: (sum_up + sum_dn) / (n_tot + EPS))."""
        s = plan.scratch[self.pred, 'stats']
        return s[0] / (s[1] + EPS)


class MalisNLL(Node):
    """loss.py:560-690.  ``pred``: Softmax with ``n_indep`` = #edges and 2 classes
    (feature 2e = "disconnected", 2e+1 = affinity of edge e), ``aff_gt`` (1, E, z, x, y)
    and ``seg_gt`` (1, 1, z, x, y) Input nodes, ``nhood`` (E, 3).

    total loss (after AggregateLoss's mean; the nll.size factors cancel, loss.py:664-670)
        = -sum(pos * log(p_aff + EPS) + neg * log(p_dis + EPS)) / (n_pos + n_neg + EPS)
    with the MALIS counts as constants of the gradient (malisop.py:114-120).  The counts
    come from the host (csrc/malis.cpp, Kruskal is sequential): the step is cut after
    the forward pass, the affinities go to the host, the counts come back, the loss
    kernel and the backward pass follow as a second captured segment.  After each step
    ``rand_index``, ``false_splits``, ``false_merges``, ``pos_count``, ``neg_count``
    hold the values of the reference's inspection outputs (loss.py:672-682)."""

    def __init__(self, pred, aff_gt, seg_gt, nhood, unrestrict_neg=True, class_weights=None,
                 example_weights=None, name="nll", print_repr=True):
        super(MalisNLL, self).__init__([pred, aff_gt, seg_gt], name, print_repr)
        if not isinstance(pred, Softmax):
            raise ValueError("The prob input to a MultinoulliNLL-node must be "
                             "a Softmax-Node.")
        if pred.shape['b'] != 1:
            raise NotImplementedError("Malis can only be used with batch size 1.")
        if class_weights is not None or example_weights is not None:
            raise NotImplementedError("class / example weights are outside the HIP hot path")
        if pred.n_class != 2:
            raise NotImplementedError("MalisNLL needs 2-class softmaxes (one per edge)")
        self.aff_gt = aff_gt
        self.seg_gt = seg_gt
        self.pred = pred
        self.nhood = np.asarray(nhood, dtype=np.int32)
        if self.nhood.shape != (pred.n_indep, 3):
            raise ValueError("nhood must be (%i, 3) for this prediction" % pred.n_indep)
        self.unrestrict_neg = unrestrict_neg
        self.axis = pred.shape.tag2index('f')
        self.n_class = pred.n_class
        self.n_indep = pred.n_indep
        self.class_weights = None
        self.example_weights = None
        self.rand_index = self.false_splits = self.false_merges = None
        self.pos_count = self.neg_count = None

    def _calc_shape(self):
        self.shape = self.parent[0].shape.updateshape(self.axis, 1)

    def _calc_comp_cost(self):
        self.computational_cost = self.parent[0].shape.stripnone_prod

    def _plan_alloc(self, plan):
        plan.scratch[self.pred, 'loss_writes_dlogits'] = True
        sh = plan.out_shape(self.pred)
        n = self.n_indep * int(np.prod(sh[2:]))
        plan.scratch[self, 'pos'] = plan.zeros_flat(n)
        plan.scratch[self, 'neg'] = plan.zeros_flat(n)
        plan.scratch[self, 'norm'] = plan.zeros_flat(4)
        plan.scratch[self, 'loss'] = plan.zeros_flat(1)
        plan.out[self] = None

    def _plan_fwd(self, plan):
        pass                   # everything happens after the host step

    def _plan_host(self, plan):
        """affinities -> host, MALIS counts (two Kruskal passes) -> device"""
        import torch
        from .. import malis
        plan.stream.synchronize()
        probs = plan.out[self.pred]
        aff = probs[0, 1::2].cpu().numpy()
        aff_gt = plan.out[self.aff_gt][0].cpu().numpy().astype(np.int16)
        seg_gt = plan.out[self.seg_gt][0, 0].cpu().numpy().astype(np.int32)
        pos, neg = malis.malis_weights(aff, aff_gt, seg_gt, self.nhood, self.unrestrict_neg)
        n_pos, n_neg = float(pos.sum(dtype=np.float64)), float(neg.sum(dtype=np.float64))
        n_tot = n_pos + n_neg
        norm = np.array([1.0 / (n_tot + EPS), n_tot, n_pos, n_neg], np.float32)
        plan.scratch[self, 'pos'].copy_(torch.from_numpy(pos.astype(np.float32).ravel()))
        plan.scratch[self, 'neg'].copy_(torch.from_numpy(neg.astype(np.float32).ravel()))
        plan.scratch[self, 'norm'].copy_(torch.from_numpy(norm))
        self.pos_count, self.neg_count = pos, neg
        self.false_splits = int(pos[aff < 0.5].sum(dtype=np.uint64))
        self.false_merges = int(neg[aff > 0.5].sum(dtype=np.uint64))
        self.rand_index = np.float32((self.false_splits + self.false_merges) / (n_tot + EPS))

    def _launch(self, plan, dlogits):
        plan.ctx.fill(plan.scratch[self, 'loss'], 0.0)
        plan.ctx.malis_nll(plan.out[self.pred], plan.scratch[self, 'pos'],
                           plan.scratch[self, 'neg'], plan.scratch[self, 'norm'], dlogits,
                           plan.scratch[self, 'loss'])

    def _plan_fwd_post(self, plan):
        if not plan.training:
            self._launch(plan, None)

    def _plan_bwd(self, plan):
        logits = self.pred.parent
        dst, first = plan.grad_slot(logits)
        if not first:
            raise NotImplementedError("logits consumed by several nodes")
        self._launch(plan, dst)          # loss and d(loss)/d(logits) in one launch

    def loss_value(self, plan):
        return plan.scratch[self, 'loss'][0]


class _ElementLoss(Node):
    """What SquaredLoss / AbsLoss / BinaryNLL / GaussianNLL share: one term of an AggregateLoss
    that runs as e2_loss_fwd -> (the aggregate's e2_loss_mix) -> e2_loss_bwd.  After a step
    ``term_value`` (this term's L, before the mixing weight) and ``n_labelled`` hold what the
    reference shows among its ``_debug_outputs``."""
    kind = None

    def _check_shapes(self, pred, others):
        if 's' in pred.shape.tags:
            raise NotImplementedError("%s: the 's' sample axis is outside the HIP hot path"
                                      % type(self).__name__)
        for what, n in others:
            if tuple(n.shape.shape) != tuple(pred.shape.shape) or \
                    tuple(n.shape.tags) != tuple(pred.shape.tags):
                raise ValueError("%s: the %s must have the prediction's shape %s, got %s"
                                 % (type(self).__name__, what, pred.shape, n.shape))
        self._last_plan = None

    def _calc_comp_cost(self):
        self.computational_cost = self.parent[0].shape.stripnone_prod

    def _views(self, plan):
        """(pred, sig, target) device views"""
        return plan.out[self.pred], None, plan.out[self.target]

    def _grad_targets(self):
        """nodes whose output gradient this term writes: (pred,) or (mu, sig)"""
        return (self.pred,)

    def _term(self, plan):
        """the e2_loss_term descriptor of this plan: names the parameters' slices of the
        parameter arena, which the kernels read when they run (no new capture for new values)"""
        t = plan.scratch.get((self, 'term'))
        if t is None:
            from .. import backend
            dev = lambda p: None if p is None else plan.param(p).reshape(-1)
            t = backend.loss_term(self.kind, margin=dev(getattr(self, 'margin', None)),
                                  scale_correction=dev(getattr(self, 'scale_correction', None)),
                                  subtract_label_entropy=getattr(self, 'subtract_label_entropy', False),
                                  sig_is_log=getattr(self, 'sig_is_log', False))
            plan.scratch[self, 'term'] = t
        return t

    def _plan_alloc(self, plan):
        for n in self.parent:
            if plan.out.get(n) is None:
                raise NotImplementedError("%s: the output of '%s' is not materialised by the plan"
                                          % (type(self).__name__, n.name))
        pred = plan.out[self.pred]
        plan.scratch[self, 'partials'] = plan.empty_flat(4 * plan.ctx.loss_partials(pred))
        plan.scratch[self, 'n_tot'] = int(pred.numel())
        plan.out[self] = None        # the element-wise array is never materialised

    def _plan_fwd(self, plan):
        pred, sig, target = self._views(plan)
        plan.ctx.loss_fwd(self._term(plan), pred, sig, target, plan.scratch[self, 'partials'])

    def _plan_bwd(self, plan):
        agg = plan.scratch.get((self, 'agg'))
        if agg is None:
            raise NotImplementedError("%s '%s' outside an AggregateLoss has no gradient"
                                      % (type(self).__name__, self.name))
        node, k = agg
        coef = plan.scratch[node, 'coef'][k:k + 1]
        pred, sig, target = self._views(plan)
        slots = [plan.grad_slot(n) if plan.needs_grad(n) else (None, True)
                 for n in self._grad_targets()]
        if len(slots) == 1:
            slots.append((None, True))
        (dp, fp), (ds, fs) = slots
        if dp is None and ds is None:
            return
        if dp is not None and ds is not None and fp != fs:
            # (one of the two buffers already holds another consumer's gradient)
            self._launch_bwd(plan, pred, sig, target, coef, dp, None, not fp)
            self._launch_bwd(plan, pred, sig, target, coef, None, ds, not fs)
            return
        self._launch_bwd(plan, pred, sig, target, coef, dp, ds, not (fp if dp is not None else fs))

    def _launch_bwd(self, plan, pred, sig, target, coef, dp, ds, acc):
        plan.ctx.loss_bwd(self._term(plan), pred, sig, target, coef, dp, ds, acc)

    def _mix_value(self, what):
        plan = self._last_plan
        agg = None if plan is None else plan.scratch.get((self, 'agg'))
        if agg is None:
            return None
        plan.stream.synchronize()
        return plan.scratch[agg[0], what][agg[1]].item()

    @property
    def term_value(self):
        """this term's value L of the last step / evaluation (None before the first)"""
        v = self._mix_value('term_loss')
        return None if v is None else np.float32(v)

    @property
    def n_labelled(self):
        """unmasked target elements of the last step / evaluation (GaussianNLL: all elements)"""
        v = self._mix_value('count')
        return None if v is None else int(round(v))


class SquaredLoss(_ElementLoss):
    """loss.py:1014-1101.  0.5 (target - pred)^2 per element; ``margin``: elements with
    |target - pred| < margin do not count (and the margin is subtracted, as the reference does);
    ``scale_correction`` sc: times sc / (|target| + sc).  Targets of -666 are masked.  A falsy
    ``margin`` / ``scale_correction`` means none (loss.py:1045, 1052)."""
    kind = 'squared'

    def __init__(self, pred, target, margin=None, scale_correction=None, name="se",
                 print_repr=True):
        super(SquaredLoss, self).__init__((pred, target), name, print_repr)
        self.target = target
        self.pred = pred
        self._check_shapes(pred, [('target', target)])
        if margin:
            margin = VariableParam(value=margin, name="margin", dtype=floatX, apply_train=False)
            self.params['margin'] = margin
        else:
            margin = None
        self.margin = margin
        if scale_correction:
            scale_correction = VariableParam(value=scale_correction, name="scale_correction",
                                             dtype=floatX, apply_train=False)
            self.params['scale_correction'] = scale_correction
        else:
            scale_correction = None
        self.scale_correction = scale_correction

    def _calc_shape(self):
        self.shape = self.parent[0].shape.updateshape(self.pred.shape.tag2index('f'), 1)


class AbsLoss(SquaredLoss):
    """loss.py:1215-1276.  |target - pred| per element, ``margin`` as for SquaredLoss;
    ``scale_correction`` sc: times sc |target| + 1.  The slope at target == pred is 0."""
    kind = 'abs'

    def __init__(self, pred, target, margin=None, scale_correction=None, name="absloss",
                 print_repr=True):
        super(AbsLoss, self).__init__(pred, target, margin=margin,
                                      scale_correction=scale_correction, name=name,
                                      print_repr=print_repr)


class BinaryNLL(_ElementLoss):
    """loss.py:953-1011.  -(t log(p + EPS) + (1 - t) log(1 - p + EPS)) per element with
    x log y = 0 where x == 0; ``subtract_label_entropy`` also subtracts the target's own entropy
    (no gradient).  Targets of -666 are masked."""
    kind = 'binary_nll'

    def __init__(self, pred, target, subtract_label_entropy=False, name="binary_nll",
                 print_repr=True):
        super(BinaryNLL, self).__init__((pred, target), name, print_repr)
        self.target = target
        self.pred = pred
        self.pred_shape = pred.shape
        self.subtract_label_entropy = bool(subtract_label_entropy)
        self._check_shapes(pred, [('target', target)])


class GaussianNLL(_ElementLoss):
    """loss.py:829-887.  0.5 log(2 pi) + log sig + 0.5 ((target - mu) / sig)^2 per element;
    ``sig_is_log``: ``sig`` holds log(sigma).  No mask."""
    kind = 'gauss_nll'

    def __init__(self, mu, sig, target, sig_is_log=False, name="g_nll", print_repr=True):
        super(GaussianNLL, self).__init__((mu, sig, target), name, print_repr)
        self.target = target
        self.mu = mu
        self.pred = mu
        self.sig = sig
        self.sig_is_log = bool(sig_is_log)
        self._check_shapes(mu, [('sig', sig), ('target', target)])

    def _views(self, plan):
        return plan.out[self.mu], plan.out[self.sig], plan.out[self.target]

    def _grad_targets(self):
        return (self.mu, self.sig)


class BetaNLL(_ElementLoss):
    """loss.py:890-950.  The negative log density of a Beta distribution given by its ``mode`` m
    and ``concentration`` c, at a target x in [0, 1], plus softplus(-c), per element:
    a = m (c - 2) + 1, b = (1 - m)(c - 2) + 1,
    -[lgamma(a + b) - lgamma(a) - lgamma(b) + (a - 1) log(x + EPS) + (b - 1) log(1 - x + EPS)].
    No mask.  ``mode`` and ``concentration`` are used as given (the reference's "exp(.) + 2" remark
    is stale): feed ``mode`` from a 'sigmoid' node and ``concentration`` from a 'soft+' node plus an
    offset, so that c > 2 and 0 < m < 1; outside that domain nothing is guarded.  Entry points of
    its own (e2_beta_nll_fwd / e2_beta_nll_bwd); in the mix it is a plain mean over all elements,
    as GaussianNLL is."""
    kind = 'gauss_nll'        # (its row of e2_loss_mix: L = S1 / n_tot)

    def __init__(self, mode, concentration, target, name="beta_nll", print_repr=True):
        super(BetaNLL, self).__init__((mode, concentration, target), name, print_repr)
        self.target = target
        self.mode = mode
        self.pred = mode
        self.concentration = concentration
        self._check_shapes(mode, [('concentration', concentration), ('target', target)])

    def _views(self, plan):
        return plan.out[self.mode], plan.out[self.concentration], plan.out[self.target]

    def _grad_targets(self):
        return (self.mode, self.concentration)

    def _plan_fwd(self, plan):
        mode, conc, target = self._views(plan)
        plan.ctx.beta_nll_fwd(mode, conc, target, plan.scratch[self, 'partials'])

    def _launch_bwd(self, plan, mode, conc, target, coef, dm, dc, acc):
        plan.ctx.beta_nll_bwd(mode, conc, target, coef, dm, dc, acc)


class OneHot(Node):
    """loss.py:96-138.  A class-id target (one feature) as ``n_class`` features of 0 / 1: what a
    SquaredLoss / BinaryNLL over an ``n_class``-feature prediction is held against.  The equality
    is exact: negative, fractional or NaN ids and ids >= n_class give a column of zeros.  One
    launch (e2_onehot, csrc/loss_map.hip), no gradient."""

    def __init__(self, target, n_class, axis='f', name="onehot", print_repr=True):
        super(OneHot, self).__init__(target, name, print_repr)
        if axis != 'f':
            raise NotImplementedError("OneHot: the class axis is the feature axis 'f'")
        if 's' in target.shape.tags:
            raise NotImplementedError("OneHot: the 's' sample axis is outside the HIP hot path")
        if target.shape['f'] != 1:
            raise ValueError("OneHot: the target must have one feature (the class id), got %s"
                             % (target.shape,))
        if int(n_class) < 1:
            raise ValueError("OneHot: n_class = %r" % (n_class,))
        self.target = target
        self.axis = target.shape.tag2index('f')
        self.n_class = int(n_class)

    def _calc_shape(self):
        self.shape = self.parent.shape.updateshape(self.axis, self.n_class)

    def _plan_alloc(self, plan):
        if plan.needs_grad(self):
            raise NotImplementedError("OneHot '%s': trainable parameters upstream of a class-id "
                                      "target (the node has no gradient)" % (self.name,))
        if plan.out.get(self.parent) is None:
            raise NotImplementedError("OneHot: the output of '%s' is not materialised by the plan"
                                      % (self.parent.name,))
        plan.alloc_out(self)

    def _plan_fwd(self, plan):
        plan.ctx.onehot(plan.out[self.parent], plan.out[self])

    def _plan_bwd(self, plan):
        pass


class _MapLoss(Node):
    """What EuclideanDistance / RampLoss share: an ordinary node whose output -- a ONE-feature map
    made over the feature axis of two parents of one shape -- the plan materialises, and whose two
    parents may BOTH need a gradient (csrc/loss_map.hip).  Under an AggregateLoss the term is the
    mean of the map: the aggregate issues e2_mean_fwd / e2_mean_bwd for it, and ``term_value`` /
    ``n_labelled`` (all elements of the map: there is no mask) work as for the element-wise
    losses."""

    def _check_shapes(self, a, b):
        if 's' in a.shape.tags:
            raise NotImplementedError("%s: the 's' sample axis is outside the HIP hot path"
                                      % type(self).__name__)
        if a is b:
            # (the value is a constant; both gradient views of one launch would be one buffer)
            raise ValueError("%s: both parents are the node '%s'" % (type(self).__name__, a.name))
        if tuple(a.shape.shape) != tuple(b.shape.shape) or \
                tuple(a.shape.tags) != tuple(b.shape.tags):
            raise ValueError("%s: both parents must have one shape, got %s and %s"
                             % (type(self).__name__, a.shape, b.shape))
        self._last_plan = None

    def _calc_shape(self):
        self.shape = self.parent[0].shape.updateshape(self.parent[0].shape.tag2index('f'), 1)

    def _calc_comp_cost(self):
        self.computational_cost = self.parent[0].shape.stripnone_prod

    def _term(self, plan):
        """the descriptor e2_loss_mix reads for the mean of this map: a plain mean over n_tot
        elements is the mix's GAUSS_NLL row (include/e2hip.h)"""
        t = plan.scratch.get((self, 'term'))
        if t is None:
            from .. import backend
            t = plan.scratch[self, 'term'] = backend.loss_term('gauss_nll')
        return t

    def _plan_alloc(self, plan):
        for n in self.parent:
            if plan.out.get(n) is None:
                raise NotImplementedError("%s: the output of '%s' is not materialised by the plan"
                                          % (type(self).__name__, n.name))
        plan.alloc_out(self)

    def _slots(self, plan):
        """((buffer or None, accumulate), ...) of the two parents' output gradients"""
        r = []
        for n in self.parent:
            if plan.needs_grad(n):
                dst, first = plan.grad_slot(n)
                r.append((dst, not first))
            else:
                r.append((None, False))
        return r

    _mix_value = _ElementLoss._mix_value
    term_value = _ElementLoss.term_value

    @property
    def n_labelled(self):
        """all elements of the map (there is no mask): the host's n_tot of the plan that ran last,
        not the slab's float count, which is exact only below 2^24 elements"""
        if self._mix_value('count') is None:
            return None
        return self._last_plan.scratch[self, 'n_tot']


class EuclideanDistance(_MapLoss):
    """loss.py:1104-1151.  sqrt(sum_f (target - pred)^2) per position, one feature; a NaN result
    is 0.  ``pred`` and ``target`` may both be network branches.  Where the distance is 0 (or was
    a NaN) every feature's gradient is an exact 0 (the reference: 0/0)."""

    def __init__(self, pred, target, name="se", print_repr=True):
        super(EuclideanDistance, self).__init__((pred, target), name, print_repr)
        self.target = target
        self.pred = pred
        self._check_shapes(pred, target)

    def _plan_fwd(self, plan):
        plan.ctx.fdist_fwd(plan.out[self.pred], plan.out[self.target], plan.out[self])

    def _plan_bwd(self, plan):
        (dp, ap), (dt, at) = self._slots(plan)
        if dp is None and dt is None:
            return
        plan.ctx.fdist_bwd(plan.out[self.pred], plan.out[self.target], plan.out[self],
                           plan.grad[self], dp, dt, ap, at)


class RampLoss(_MapLoss):
    """loss.py:1154-1212.  mean_f max(d_low - d_big + margin, 0) per position (NaN as 0), one
    feature: over two EuclideanDistance nodes the triplet loss.  ``margin`` is a non-trainable
    parameter (0 when None) the kernels read in place.  The slope at exactly 0 is 1."""

    def __init__(self, d_low, d_big, name="se", print_repr=True, margin=None):
        super(RampLoss, self).__init__((d_low, d_big), name, print_repr)
        if margin is None:
            margin = 0
        margin = VariableParam(value=margin, name="margin", dtype=floatX, apply_train=False)
        self.params['margin'] = margin
        self.margin = margin
        self.d_low = d_low
        self.d_big = d_big
        self._check_shapes(d_low, d_big)

    def _plan_fwd(self, plan):
        plan.ctx.ramp_fwd(plan.out[self.d_low], plan.out[self.d_big],
                          plan.param(self.margin).reshape(-1), plan.out[self])

    def _plan_bwd(self, plan):
        (dl, al), (db, ab) = self._slots(plan)
        if dl is None and db is None:
            return
        plan.ctx.ramp_bwd(plan.out[self.d_low], plan.out[self.d_big],
                          plan.param(self.margin).reshape(-1), plan.grad[self], dl, db, al, ab)


class AggregateLoss(Node):
    def __init__(self, parent_nodes, mixing_weights=None, name="total_loss", print_repr=True):
        if not isinstance(parent_nodes, (tuple, list)):
            parent_nodes = [parent_nodes, ]
        super(AggregateLoss, self).__init__(parent_nodes, name, print_repr)
        if mixing_weights is None:
            mixing_weights = np.ones(len(parent_nodes))
        if isinstance(mixing_weights, (tuple, list, np.ndarray)):
            if len(parent_nodes) != len(mixing_weights):
                raise ValueError("Mismatch: len(parent_nodes)=%i, len(weights)=%i"
                                 % (len(parent_nodes), len(mixing_weights)))
            mixing_weights = VariableParam(value=np.array(mixing_weights, dtype=floatX),
                                           name="loss_mixing_weights", dtype=floatX,
                                           apply_train=False)
        else:
            raise ValueError("Unsupported weight format")
        self.params['mixing_weights'] = mixing_weights
        self.mixing_weights = mixing_weights
        # three forms: exactly one MultinoulliNLL / MalisNLL (their own launches make the loss),
        # 1..MAX_LOSS_TERMS element-wise losses mixed by this node's launch (csrc/loss_elem.hip;
        # a loss MAP -- EuclideanDistance, RampLoss -- counts as one: the term is the map's mean),
        # or 'multi_nll': 2..MAX_LOSS_TERMS distinct plain MultinoulliNLL terms, each over a
        # softmax of its own, run and mixed by this node's launches (csrc/softmax_nll.hip)
        self.elementwise = len(parent_nodes) > 0 and \
            all(isinstance(n, (_ElementLoss, _MapLoss)) for n in parent_nodes)
        self.multi_nll = (
            2 <= len(parent_nodes) <= MAX_LOSS_TERMS
            and all(isinstance(n, MultinoulliNLL) and n.n_indep == 1 and not n.weighted
                    for n in parent_nodes)
            and len(set(id(n) for n in parent_nodes)) == len(parent_nodes)
            and len(set(id(n.pred) for n in parent_nodes)) == len(parent_nodes))
        if self.multi_nll:
            return
        if self.elementwise:
            if len(parent_nodes) > MAX_LOSS_TERMS:
                raise ValueError("AggregateLoss: %i losses given, the HIP hot path mixes at most %i"
                                 % (len(parent_nodes), MAX_LOSS_TERMS))
        elif len(parent_nodes) != 1 and any(isinstance(n, (MultinoulliNLL, MalisNLL))
                                            for n in parent_nodes):
            raise NotImplementedError("a MultinoulliNLL / MalisNLL cannot be mixed with other "
                                      "losses: their fused tail / head launches take no scale")
        elif len(parent_nodes) != 1 or not isinstance(parent_nodes[0], (MultinoulliNLL, MalisNLL)):
            raise NotImplementedError("the HIP hot path aggregates exactly one "
                                      "MultinoulliNLL / MalisNLL loss, or 1..%i of SquaredLoss / "
                                      "AbsLoss / BinaryNLL / GaussianNLL" % MAX_LOSS_TERMS)

    def _calc_shape(self):
        self.shape = TaggedShape([1, ], ['f', ])

    def _calc_comp_cost(self):
        self.computational_cost = np.sum([inp.shape.stripnone_prod for inp in self.parent])

    def _fused_heads(self, plan):
        """multi_nll: the head Convs, in term order, when ALL terms run in the fused multi-head
        launches (csrc/multihead.hip): plan option fuse_multihead, every term's logits from a
        Conv of the classifier-head form (Conv._head_form), all of them on one trunk, within
        e2_multihead_supported.  Else None: the generic pair reads materialised logits."""
        key = (self, 'fused_heads')
        if key not in plan.scratch:
            heads = None
            convs = [n.pred.parent for n in self.parent]
            if (self.multi_nll and plan.opt['fuse_multihead']
                    and all(getattr(c, '_head_form', None) is not None
                            and c._head_form(plan) is n.pred for c, n in zip(convs, self.parent))
                    and not isinstance(convs[0].parent, (list, tuple))
                    and all(c.parent is convs[0].parent for c in convs)
                    and plan.ctx.multihead_supported(convs[0].parent.shape['f'],
                                                     [c.n_f for c in convs])):
                heads = convs
            plan.scratch[key] = heads
        return plan.scratch[key]

    def _plan_alloc(self, plan):
        plan.out[self] = None
        if self.multi_nll:
            heads = self._fused_heads(plan)
            if heads is not None and plan.training:
                nb = plan.ctx.multihead_bwd_ws_bytes(plan.out_shape(heads[0].parent),
                                                     sum(c.n_f for c in heads))
                plan.scratch[self, 'head_ws'] = plan.empty_flat(nb // 4 + 16)
            # one slab {S_0, N_0, S_1, N_1, ...}: every Softmax's 'stats' is its pair of it
            K = len(self.parent)
            slab = plan.zeros_flat(2 * K)
            plan.scratch[self, 'stats'] = slab
            for k, n in enumerate(self.parent):
                plan.scratch[n.pred, 'stats'] = slab[2 * k:2 * k + 2]
            for what in ('coef', 'term_loss', 'count'):
                plan.scratch[self, what] = plan.zeros_flat(MAX_LOSS_TERMS)
            plan.scratch[self, 'loss'] = plan.zeros_flat(1)
        if self.elementwise:
            for k, n in enumerate(self.parent):
                plan.scratch[n, 'agg'] = (self, k)
                n._last_plan = plan
                if isinstance(n, _MapLoss):       # (the mean of the map is this node's launch)
                    m = plan.out[n]
                    plan.scratch[n, 'partials'] = plan.empty_flat(4 * plan.ctx.loss_partials(m))
                    plan.scratch[n, 'n_tot'] = int(m.numel())
            for what in ('coef', 'term_loss', 'count'):
                plan.scratch[self, what] = plan.zeros_flat(MAX_LOSS_TERMS)
            plan.scratch[self, 'loss'] = plan.zeros_flat(1)

    def _last_softmax(self, plan):
        """multi_nll: the term's Softmax that stands last in the plan's node order"""
        preds = [n.pred for n in self.parent]
        return max(preds, key=lambda sm: [i for i, n in enumerate(plan.nodes) if n is sm][0])

    def _emit_fwd(self, plan):
        """multi_nll: every term's probabilities and sums in one launch, then the mix (also in
        forward-only plans: the total exists without a backward pass).  Issued by the last
        Softmax of the terms (Softmax._plan_fwd), not at this node's own place in the plan."""
        ps = list(self.parent)
        slab = plan.scratch[self, 'stats']
        plan.zero_early(slab)
        heads = self._fused_heads(plan)
        if heads is not None:          # trunk -> all logits -> softmaxes -> sums, one launch
            plan.ctx.multihead_fwd(plan.out[heads[0].parent],
                                   [plan.param(c.w).reshape(c.n_f, -1) for c in heads],
                                   [plan.param(c.b) for c in heads],
                                   [plan.out[n.target] for n in ps],
                                   [plan.out[n.pred] for n in ps], slab)
        else:
            plan.ctx.nll_multi_fwd([plan.out[n.pred.parent] for n in ps],
                                   [plan.out[n.target] for n in ps],
                                   [plan.out[n.pred] for n in ps], slab)
        plan.ctx.nll_mix(len(ps), slab, plan.param(self.mixing_weights).reshape(-1),
                         plan.scratch[self, 'coef'], plan.scratch[self, 'term_loss'],
                         plan.scratch[self, 'count'], plan.scratch[self, 'loss'])

    def _plan_fwd(self, plan):
        if not self.elementwise:           # (multi_nll: _emit_fwd, issued by the last Softmax)
            return
        ps = list(self.parent)
        for n in ps:
            if isinstance(n, _MapLoss):
                plan.ctx.mean_fwd(plan.out[n], plan.scratch[n, 'partials'])
        plan.ctx.loss_mix([n._term(plan) for n in ps], [plan.scratch[n, 'partials'] for n in ps],
                          [plan.scratch[n, 'n_tot'] for n in ps],
                          plan.param(self.mixing_weights).reshape(-1), plan.scratch[self, 'coef'],
                          plan.scratch[self, 'term_loss'], plan.scratch[self, 'count'],
                          plan.scratch[self, 'loss'])

    def _plan_bwd(self, plan):
        if self.multi_nll:
            ps = list(self.parent)
            heads = self._fused_heads(plan)
            if heads is not None:
                trunk = heads[0].parent
                dst, first = (plan.grad_slot(trunk) if plan.needs_grad(trunk) else (None, True))
                plan.ctx.multihead_bwd(plan.out[trunk],
                                       [plan.param(c.w).reshape(c.n_f, -1) for c in heads],
                                       [plan.out[n.pred] for n in ps],
                                       [plan.out[n.target] for n in ps],
                                       plan.scratch[self, 'coef'], dst, not first,
                                       [plan.pgrad(c.w).reshape(c.n_f, -1) for c in heads],
                                       [plan.pgrad(c.b) for c in heads],
                                       plan.scratch[self, 'head_ws'])
                return
            dsts = []
            for n in ps:
                logits = n.pred.parent
                if not plan.needs_grad(logits):
                    raise NotImplementedError("AggregateLoss: term '%s' has no trainable "
                                              "parameter upstream" % (n.name,))
                dst, first = plan.grad_slot(logits)
                if not first:
                    raise NotImplementedError("logits consumed by several nodes")
                dsts.append(dst)
            plan.ctx.nll_multi_bwd([plan.out[n.pred] for n in ps],
                                   [plan.out[n.target] for n in ps],
                                   plan.scratch[self, 'coef'], dsts)
            return
        # d(total)/d(nll) = mixing_weight(=1) / 1 ; folded into the NLL backward
        # (element-wise losses: coef[k], which each term's backward launch reads; a loss map's
        # own backward runs behind this node's: its output gradient is coef[k] everywhere)
        if self.elementwise:
            for k, n in enumerate(self.parent):
                if isinstance(n, _MapLoss) and plan.needs_grad(n):
                    dst, first = plan.grad_slot(n)
                    plan.ctx.mean_bwd(plan.scratch[self, 'coef'][k:k + 1], dst, not first)

    def loss_dev(self, plan):
        """the one-element device tensor that holds the step's loss"""
        if self.elementwise or self.multi_nll:
            for n in self.parent:
                n._last_plan = plan
            return plan.scratch[self, 'loss']
        return plan.scratch[self.parent[0], 'loss']

    def host_value(self, plan):
        if self.elementwise or self.multi_nll:
            return np.float32(self.loss_dev(plan).item())
        w = float(self.mixing_weights.get_value()[0])
        return np.float32(float(self.parent[0].loss_value(plan).item()) * w)


class Classification(Node):
    def __init__(self, pred, n_class='auto', n_indep='auto', name="cls", print_repr=True):
        super(Classification, self).__init__(pred, name, print_repr)
        if not isinstance(pred, Softmax):
            raise NotImplementedError("Classification of non-softmax predictions")
        self.n_class = pred.n_class
        self.n_indep = pred.n_indep
        self.sm_input = True
        self.pred = pred

    def _calc_shape(self):
        self.shape = self.parent.shape.updateshape(self.pred.shape.tag2index('f'),
                                                   self.n_indep)

    def _plan_alloc(self, plan):
        plan.out[self] = None

    def _plan_fwd(self, plan):
        pass


class _Errors(Node):
    def __init__(self, cls, target, target_is_sparse=False, name="errors", print_repr=True):
        super(_Errors, self).__init__([cls, target], name, print_repr)
        self.n_class = cls.n_class
        self.n_indep = cls.n_indep
        self.target = target
        self.cls = cls
        self.target_is_sparse = target_is_sparse
        if not target_is_sparse:
            raise NotImplementedError("dense targets are outside the HIP hot path")

    def _calc_shape(self):
        self.shape = TaggedShape([1, ], ['f', ])

    def _plan_alloc(self, plan):
        plan.out[self] = None

    def _plan_fwd(self, plan):
        pass

    def host_value(self, plan):
        """mean(int16(target) != argmax_f(pred))  (loss.py:789-817), the argmax inside each
        group of ``n_class`` features for ``n_indep > 1`` (loss.py:737-748); evaluated
        with torch ops on the device tensors, outside any captured graph."""
        import torch
        probs = plan.out[self.cls.pred]
        if self.n_indep != 1:
            sh = probs.shape
            cls = torch.argmax(probs.reshape(sh[0], self.n_indep, self.n_class, *sh[2:]), dim=2)
        else:
            cls = torch.argmax(probs, dim=1, keepdim=True)
        gt = plan.out[self.target].to(torch.int16).to(cls.dtype)
        return np.float32((gt != cls).float().mean().item())


def Errors(pred, target, target_is_sparse=False, n_class='auto', n_indep='auto',
           name="errors", print_repr=True):
    if not isinstance(pred, Classification):
        pred = Classification(pred, n_class=n_class, n_indep=n_indep,
                              name='cls for errors', print_repr=False)
    return _Errors(pred, target, target_is_sparse=target_is_sparse, name=name,
                   print_repr=print_repr)
