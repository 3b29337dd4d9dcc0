"""Target conversions of the data pipeline (reference: data/image.py)."""
from __future__ import annotations

import numpy as np

from .. import malis

MAX_EDGES = 64                  # kMaxEdges of csrc/targets.hip

# cnndata.py:357-363: the neighbourhood getbatch(nhood_targets=True) stands for
DEFAULT_NHOOD = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0],
                          [0, 0, 1], [0, 0, -1]], np.int32)


def make_affinities(labels, nhood=None, size_thresh=1):
    """data/image.py:30-77: affinity graph + locally relabelled segmentation of a batch
    of ID volumes ``labels`` (bs, z, x, y).  ID 0 is background (never connected);
    edges leaving the volume are 0.  Returns ``aff`` (bs, #edges, z, x, y) int16 and
    ``seg`` (bs, z, x, y) int16 = connected components of ``aff`` (components smaller
    than ``size_thresh`` -> 0)."""
    labels = np.asarray(labels)
    if nhood is None:
        nhood = np.eye(3, dtype=np.int32)
    nhood = np.asarray(nhood, np.int32)
    aff = np.zeros((labels.shape[0], nhood.shape[0]) + labels.shape[1:], np.int16)
    seg = np.zeros(labels.shape, np.int16)
    for i, l in enumerate(labels):
        aff[i] = malis.seg_to_affgraph(l, nhood)
        seg[i], _ = malis.affgraph_to_seg(aff[i], nhood, size_thresh)
    return aff, seg


def check_nhood(nhood, extents=None):
    """``nhood`` as an (E, 3) int32 array, 1 <= E <= 64.  With ``extents`` (z, x, y) -- the
    neighbourhood-target form -- every displacement must be shorter than its axis: the reference's
    slicing (data/image.py:92-100) is ill-defined beyond that."""
    nh = np.asarray(nhood)
    if nh.ndim != 2 or nh.shape[1] != 3:
        raise ValueError("nhood must be (E, 3), got %s" % (nh.shape,))
    if not np.array_equal(nh, np.rint(nh)):
        raise ValueError("nhood must hold whole displacements")
    nh = np.ascontiguousarray(nh, np.int32)
    if not 1 <= nh.shape[0] <= MAX_EDGES:
        raise ValueError("nhood has %d edges; the kernels take 1..%d" % (nh.shape[0], MAX_EDGES))
    if extents is not None:
        for k in range(3):
            if np.abs(nh[:, k]).max() >= int(extents[k]):
                raise ValueError("nhood moves %d along axis %d of extent %d"
                                 % (np.abs(nh[:, k]).max(), k, int(extents[k])))
    return nh


def strided_extents(sp, stride):
    return tuple(-(-int(n) // int(s)) for n, s in zip(sp, stride))


def make_nhood_targets(target, nhood, stride=(1, 1, 1), ctx=None):
    """data/image.py:80-102 on a device tensor ``target`` (b, 1, z, x, y): channel e of the result
    is the target displaced by ``nhood[e]`` -- out[:, e, p] = target[:, 0, p - nhood[e]] -- with -1
    where the shift leaves the patch.  One launch (e2_target_nhood), which also takes the output
    ``stride`` of the net and writes NaN as -666; further channels of ``target`` are appended
    (strided) as cnndata.py:367-369 does."""
    import torch
    if target.dim() != 5:
        raise NotImplementedError("make_nhood_targets: (b, 1, z, x, y) targets only")
    nh = check_nhood(nhood, target.shape[2:])
    if ctx is None:
        from ..neuromancer.plan import get_ctx
        ctx = get_ctx()
    out = torch.empty((target.shape[0], nh.shape[0] + target.shape[1] - 1)
                      + strided_extents(target.shape[2:], stride),
                      dtype=torch.float32, device=target.device)
    ctx.target_nhood(target, nh, stride, out)
    return out


def ecs_mode(ecs_as_barr):
    """the ``ecs_as_barr`` argument of ids2barriers -> the kernel's mode (0 none, 1 ECS is barrier,
    2 'new_class')"""
    if isinstance(ecs_as_barr, str):
        if ecs_as_barr != 'new_class':
            raise ValueError("ecs_as_barr: True, False or 'new_class', got %r" % (ecs_as_barr,))
        return 2
    return 1 if ecs_as_barr else 0


def ids2barriers(ids, dilute=(True, True, True), connectivity=(True, True, True),
                 ecs_as_barr=True, smoothen=False, ctx=None):
    """data/image.py:182-220 on the device: the barrier volume (1 where neighbouring IDs differ,
    two voxels wide, four where diluted; ``ecs_as_barr``: ID 0 is barrier too, or class 2 with
    'new_class') of a (z, x, y) ID volume, host array or device tensor.  Returns a float32 device
    tensor (z, x, y).  ``smoothen`` is a scipy filter on the host and not part of this build."""
    import torch
    if smoothen:
        raise NotImplementedError("ids2barriers: smoothen=True is a scipy filter, not built here")
    mode = ecs_mode(ecs_as_barr)
    if len(dilute) != 3 or len(connectivity) != 3:
        raise ValueError("ids2barriers: dilute and connectivity take three flags")
    if ctx is None:
        from ..neuromancer.plan import get_ctx
        ctx = get_ctx()
    if not isinstance(ids, torch.Tensor):
        ids = torch.from_numpy(np.array(ids, np.float32))
    if ids.dim() != 3:
        raise ValueError("ids2barriers: a (z, x, y) volume, got %s" % (tuple(ids.shape),))
    ids = ids.to(device=ctx.device, dtype=torch.float32)
    if ids.shape[2] > 1 and ids.stride(2) != 1:
        ids = ids.contiguous()
    out = torch.empty(tuple(ids.shape), dtype=torch.float32, device=ctx.device)
    ctx.ids2barriers(ids[None, None], dilute, connectivity, mode, out[None, None])
    return out
