"""Batch creation from volumes resident on the GPU: the part of
``BatchCreatorImage.getbatch`` (data/cnndata.py:214-402) that is on the training path --
draw a cube, cut a (warped) patch and its centred target, grey-augment the image,
sub-sample the target by the net's output strides, and derive the target form the loss wants --
neighbourhood targets, affinities, NaN -> -666, lazy-label masks, the ``ignore_thresh``
rejection -- by HIP launches (csrc/targets.hip) on the patch that already lies in HBM: no target
tensor is copied to the host (``ignore_thresh`` reads one 4-byte count per patch back;
``affinities='malis'`` keeps its host step, as MalisNLL has one anyway).  Left out: the file /
HDF5 / KNOSSOS plumbing, ``target_vec_ix`` and the non-geometric blob augmentations."""
from __future__ import annotations

import numpy as np
import torch

from . import transformations
from .image import (DEFAULT_NHOOD, check_nhood, make_affinities, make_nhood_targets,
                    strided_extents)
from .transformations import WarpingOOBError


def grey_augment(d, channels, rng, ctx=None):
    """cnndata.py:42-60 on a device tensor (f, z, x, y):
    ``d[ch] = clip(d[ch] * alpha + c, 0, 1) ** gamma`` with alpha ~ 1 +- 0.15,
    c ~ +- 0.15, gamma ~ 2**U(-1, 1), one triple per listed channel; returns a new
    tensor (the patch is a fresh buffer anyway, so it is modified in place)."""
    if not channels:
        return d
    if ctx is None:
        from ..neuromancer.plan import get_ctx
        ctx = get_ctx()
    k = len(channels)
    alpha = 1 + (rng.rand(k) - 0.5) * 0.3
    c = (rng.rand(k) - 0.5) * 0.3
    gamma = 2.0 ** (rng.rand(k) * 2 - 1)
    for i, ch in enumerate(channels):
        ctx.grey_augment(d[ch], alpha[i], c[i], gamma[i])
    return d


class PatchSampler(object):
    """``getbatch(batch_size, source, grey_augment_channels, warp, warp_args)`` ->
    ``(data (b, f, z, x, y), target (b, f_t, z', x', y'))`` device tensors.

    data / targets: lists of (f, z, x, y) arrays (uploaded once); targets must be
    centred in their images.  ``patch_size`` = the input node's spatial shape,
    ``strides`` / ``offsets`` = the target node's (cnndata.py:134-140).  ``ll_masks``: one entry
    per cube, None or ``(mask_class_labeled, mask_class_not_present)`` (the ``ll_mask`` the
    reference reads from its label files, cnndata.py:511-519); ``getbatch(ret_ll_mask=True)``
    returns those of the cubes it drew."""

    @classmethod
    def from_nodes(cls, input_node, target_node=None, data=None, targets=None,
                   cube_prios=None, valid_cubes=None, aniso_factor=2, target_vec_ix=None,
                   target_discrete_ix=None, seed=None, border_mode='crop', d_path=None,
                   l_path=None, d_files=None, l_files=None, h5stream=False, zxy=True,
                   ll_masks=None):
        """The reference constructor protocol (``BatchCreatorImage(input_node,
        target_node, **data_init_kwargs)``, cnndata.py:110-176): the geometry is read from
        the nodes -- ``patch_size = input_node.shape.spatial_shape``, ``strides`` /
        ``offsets`` of ``target_node.shape`` (cnndata.py:134-140) -- so a reference
        config's ``data_init_kwargs`` dict drives it unchanged.  The cubes are given as
        in-memory arrays (``data`` / ``targets``: lists of (f, z, x, y)); the file keys of
        the dict (``d_path``, ``l_path``, ``d_files``, ``l_files``, ``h5stream``, ``zxy``,
        ``border_mode``) belong to the HDF5 loader, which is outside the hot path, and are
        accepted and ignored."""
        if target_node is None:
            raise ValueError("from_nodes: a target node is required (img-img mode)")
        if data is None or targets is None:
            raise ValueError("from_nodes: pass the cubes as data=[...], targets=[...] "
                             "(HDF5 loading is not part of this build)")
        if len(data) != len(targets):
            raise ValueError("d_files and l_files must be lists of same length!")
        if input_node.shape.ndim != target_node.shape.ndim:
            raise ValueError("img-scalar mode is outside the hot path")
        if target_vec_ix is not None:
            raise NotImplementedError("vector targets (target_vec_ix) are outside the hot path")
        return cls(data, targets, input_node.shape.spatial_shape, target_node.shape.strides,
                   target_node.shape.offsets, aniso_factor=aniso_factor,
                   target_discrete_ix=target_discrete_ix, seed=seed,
                   valid=valid_cubes if valid_cubes is not None else (),
                   cube_prios=cube_prios, ll_masks=ll_masks)

    @staticmethod
    def prepare_ll_masks(ll_masks, n_cubes, n_t):
        """The lazy-label masks per cube as one (n_cubes, 2, L) float32 array: an entry is None or
        ``(mask_class_labeled, mask_class_not_present)``, both 1-D of one common length L; None
        stands for ``(ones(L), zeros(L))`` and L = n_t (the target's feature count) where every
        entry is None (cnndata.py:518-519)."""
        if ll_masks is None:
            ll_masks = [None] * n_cubes
        ll_masks = list(ll_masks)
        if len(ll_masks) != n_cubes:
            raise ValueError("ll_masks: %d entries for %d cubes" % (len(ll_masks), n_cubes))
        given = []
        for e in ll_masks:
            if e is None:
                continue
            if len(e) != 2:
                raise ValueError("ll_masks: an entry is None or a pair (mask1, mask2)")
            pair = [np.asarray(m, np.float32) for m in e]
            if pair[0].ndim != 1 or pair[1].ndim != 1 or pair[0].shape != pair[1].shape:
                raise ValueError("ll_masks: the masks are 1-D and of one length")
            given.append(pair)
        L = given[0][0].shape[0] if given else int(n_t)
        if L < 1 or any(p[0].shape[0] != L for p in given):
            raise ValueError("ll_masks: the masks of all cubes must have one common length >= 1")
        out = np.empty((n_cubes, 2, L), np.float32)
        out[:, 0], out[:, 1] = 1.0, 0.0
        it = iter(given)
        for i, e in enumerate(ll_masks):
            if e is not None:
                out[i, 0], out[i, 1] = next(it)
        return out

    def __init__(self, data, targets, patch_size, strides, offsets, aniso_factor=2,
                 target_discrete_ix=None, seed=None, valid=(), cube_prios=None, ll_masks=None):
        from ..neuromancer.plan import get_ctx
        if len(data) != len(targets):
            raise ValueError("data and targets must be lists of same length!")
        ll = self.prepare_ll_masks(ll_masks, len(targets), np.shape(targets[0])[0])
        # NaN in a target cube (unlabelled voxels of a regression target) reaches the loss as -666
        # (cnndata.py:395-396); looked for once, here, on the host arrays
        self.has_nan = any(bool(np.isnan(np.asarray(a, np.float32)).any()) for a in targets)
        self.ctx = get_ctx()
        dev = self.ctx.device
        self.d = [torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev) for a in data]
        self.t = [torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev) for a in targets]
        self.valid = list(valid)
        self.train = [i for i in range(len(self.d)) if i not in self.valid]
        self.patch_size = tuple(int(p) for p in patch_size)
        self.strides = tuple(int(s) for s in strides)
        self.offsets = tuple(int(o) for o in offsets)
        self.target_ps = tuple(p - 2 * o for p, o in zip(self.patch_size, self.offsets))
        self.aniso_factor = aniso_factor
        self.target_discrete_ix = target_discrete_ix
        self.rng = np.random.RandomState(seed)
        if cube_prios is None:               # proportional to the cube sizes, cnndata.py:535-541
            w = np.array([self.t[i][0].numel() for i in self.train], np.float64)
        else:
            w = np.array([cube_prios[i] for i in self.train], np.float64)
        self._sampling_weight = np.hstack((0, np.cumsum(w / w.sum())))   # cnndata.py:576-583
        self.n_failed_warp = 0
        self.n_successful_warp = 0
        self.n_ignored = 0                   # patches that ignore_thresh threw away
        self._ll_host = ll
        self._ll_any_not_present = ll[:, 1].any(axis=1)
        self.ll_masks = torch.from_numpy(ll).to(dev)             # (cubes, 2, L)
        self._neg = torch.zeros(1, dtype=torch.int32, device=dev)

    def _drawcube(self, source):
        if source == 'train':
            p = self.rng.rand()
            i = self.train[int(np.flatnonzero(self._sampling_weight <= p)[-1])]
        elif source == 'valid':
            if not self.valid:
                raise ValueError("No validation set")
            i = self.valid[self.rng.randint(0, len(self.valid))]
        else:
            raise ValueError("Unknown data source")
        return i

    def _getcube(self, source):
        i = self._drawcube(source)
        return self.d[i], self.t[i]

    def _negative_fraction(self, patch):
        """(t < 0).mean() of one target patch: a count on the device, one 4-byte readback"""
        with torch.cuda.stream(self.ctx.stream):
            self._neg.zero_()
            self.ctx.count_negative(patch, self._neg)
            n_neg = int(self._neg.item())
        return np.float64(n_neg) / np.float64(patch.numel())

    def getbatch(self, batch_size=1, source='train', grey_augment_channels=None, warp=False,
                 warp_args=None, force_dense=False, affinities=False, nhood=None,
                 ignore_thresh=False, nhood_targets=False, ret_ll_mask=False):
        """cnndata.py:214-402.  ``affinities='malis'``: the batch is
        ``(images, aff, seg)`` for a MalisNLL loss -- affinity graph and relabelled IDs of
        the first target channel (cnndata.py:377-382; computed on the host, the ID
        volumes are small); ``'affinity'``: ``(images, aff)``, the affinity graph of the rounded,
        strided first target channel over ``nhood`` (None: the three unit edges), made by one
        launch on the device.

        ``nhood_targets``: True (the seven-edge neighbourhood of cnndata.py:357-363) or an (E, 3)
        array -- the first target channel becomes E channels, the full-resolution patch displaced
        by every edge (-1 where the shift leaves it), further channels are kept behind them.
        ``ignore_thresh``: a patch of a cube without a ``not_present`` mask whose share of
        negative targets exceeds it is discarded and a new cube drawn (cnndata.py:319-322).
        ``ret_ll_mask``: the lazy-label masks ``(bs, L)`` of the cubes drawn are appended, as
        device tensors that feed ``mask_class_labeled`` / ``mask_class_not_present``.
        The order is the reference's: nhood targets, stride, affinities, NaN -> -666 (only a
        sampler whose cubes hold NaN runs that replacement).  None of the options draws random
        numbers of its own."""
        grey_augment_channels = grey_augment_channels or []
        warp_args = dict(warp_args or {})
        n_f, n_t = self.d[0].shape[0], self.t[0].shape[0]
        dev = self.ctx.device
        if nhood_targets is None or nhood_targets is False:
            nh_t = None
        else:
            nh_t = check_nhood(DEFAULT_NHOOD if nhood_targets is True else nhood_targets,
                               self.target_ps)
        images = torch.empty((batch_size, n_f) + self.patch_size, dtype=torch.float32, device=dev)
        target = torch.empty((batch_size, n_t) + self.target_ps, dtype=torch.float32, device=dev)
        count = 0
        drawn = []
        while count < batch_size:
            cube = self._drawcube(source)
            d, t = self.d[cube], self.t[cube]
            if warp is True or warp == 1:
                do_warp = True
            elif 0 < warp < 1:
                do_warp = bool(self.rng.rand() < warp)
            else:
                do_warp = False
            args = dict(warp_args)
            if not do_warp:
                args['warp_amount'] = 0
            try:
                transformations.get_warped_slice(
                    d, self.patch_size, aniso_factor=self.aniso_factor, target=t,
                    target_ps=self.target_ps, target_discrete_ix=self.target_discrete_ix,
                    rng=self.rng, out=images[count], target_out=target[count], **args)
                self.n_successful_warp += 1
            except WarpingOOBError:
                self.n_failed_warp += 1
                continue
            # only if a threshold is set and the cube is labelled (cnndata.py:319-322)
            if ignore_thresh is not False and not self._ll_any_not_present[cube]:
                if self._negative_fraction(target[count:count + 1]) > ignore_thresh:
                    self.n_ignored += 1
                    continue
            if source == 'train':
                grey_augment(images[count], grey_augment_channels, self.rng, self.ctx)
            drawn.append(cube)
            count += 1
        stride = (1, 1, 1) if force_dense else self.strides
        nan_done = not self.has_nan
        if nh_t is not None:                 # the shift on the full-resolution patch, then the stride
            target = make_nhood_targets(target, nh_t, stride, self.ctx)
            stride, nan_done = (1, 1, 1), True
        if affinities == 'affinity':
            nh = check_nhood(np.eye(3, dtype=np.int32) if nhood is None else nhood)
            aff = torch.empty((batch_size, nh.shape[0]) + strided_extents(target.shape[2:], stride),
                              dtype=torch.float32, device=dev)
            self.ctx.target_affinity(target, nh, stride, aff)
            ret = [images, aff]
        else:
            if not nan_done:
                out = torch.empty(tuple(target.shape[:2]) + strided_extents(target.shape[2:], stride),
                                  dtype=torch.float32, device=dev)
                self.ctx.target_stride(target, stride, out)
                target = out
            elif not all(s == 1 for s in stride):
                target = target[:, :, ::stride[0], ::stride[1], ::stride[2]]
            if affinities == 'malis':
                ids =np.rint(target[:, 0].cpu().numpy()).astype(np.int32)
                aff, seg = make_affinities(ids, nhood)
                ret = [images, torch.from_numpy(aff.astype(np.float32)).to(dev),
                       torch.from_numpy(seg[:, None].astype(np.float32)).to(dev)]
            else:
                ret = [images, target]
        if ret_ll_mask:                      # (bs, L) each, of the cubes that were drawn
            ll = self.ll_masks[torch.as_tensor(drawn, dtype=torch.long).to(dev)]
            ret += [ll[:, 0].contiguous(), ll[:, 1].contiguous()]
        return tuple(ret)


class RingFeeder(object):
    """Keeps the input ring of a training plan (Plan.set_input_ring) filled ``k`` batches at a time,
    one launch ahead of ``Model.trainingsteps(k, ring=feeder.ring, sync=False)``:

        feeder = RingFeeder(sampler, model, 'Adam', k, grey_augment_channels=[0], warp=0.5)
        feeder.fill()                                   # the first k slots
        for b in range(n_launches):
            losses, t = model.trainingsteps(k, optimiser='Adam', ring=feeder.ring, sync=False)
            feeder.fill()                               # the other half, while the launch runs

    The ring has 2 k slots; ``fill`` writes the k slots the NEXT launch will read.  They were last
    read by the launch before the one just submitted, whose losses ``trainingsteps(sync=False)``
    has just waited for -- so the slots are free without any further synchronisation.  The
    reference's counterpart is the BackgroundProc queue in front of trainingstep
    (training/trainer.py:174-186)."""

    def __init__(self, sampler, model, optimiser, k, **getbatch_kwargs):
        opt = model.optimisers[optimiser]
        plan = opt.step.func
        if plan is None or not plan._built:
            raise RuntimeError("RingFeeder: call trainingstep once first (it builds the plan)")
        self.sampler, self.plan, self.k, self.kw = sampler, plan, int(k), getbatch_kwargs
        self.ring = torch.zeros(2 * self.k, plan.input_arena.numel(), device=plan.ctx.device)
        plan.set_input_ring(self.ring)
        self.next = plan.ring_position()        # the step that reads the next slot to fill
        self.batch = plan.batch

    def fill(self):
        n = self.ring.shape[0]
        for j in range(self.k):
            batch = self.sampler.getbatch(self.batch, 'train', **self.kw)
            row = self.ring[(self.next + j) % n]
            for node, src in zip(self.plan.inputs, batch):
                o, cnt = self.plan.input_slices[node]
                row[o:o + cnt].copy_(src.reshape(-1), non_blocking=True)
        self.next += self.k

