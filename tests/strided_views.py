"""Output views inside watched storage (helpers of test_strided_outputs_gpu.py; no test module).

The training plan hands the kernels outputs that are NOT dense: the interior of a zero-framed
image (plan.alloc_out under pad_inplace), a channel slice of a concat buffer, the interior of a
padded gradient buffer.  ``make_view`` builds such a view inside a flat storage that is filled
with distinct finite floats, so that a store that misses the view -- a stray zero, a stray value,
a stray NaN -- changes bits that ``assert_outside_untouched`` compares.

Every view lies strictly inside its storage: in front of the first and behind the last element
of the buffer that holds the view there is one full plane (Hp * Wp floats) plus 4 floats (one
16-byte piece on either side of a row), so a misplaced store lands in checked memory.
"""
import numpy as np
import torch

#: name -> (frame (fd, fh, fw) around the view, channel slice [2:2+C] of C+3?, wanted offset of
#: the first element from a 16-byte boundary in floats or None)
GEOMS = {
    "dense":        ((0, 0, 0), False, 0),      # control
    "frame111":     ((1, 1, 1), False, 1),      # sh = W + 2, first element at an ODD float offset
    "frame022":     ((0, 2, 2), False, 2),      # sh = W + 4, offset 2 floats (mod 4)
    "cslice":       ((0, 0, 0), True, None),    # sc = D*H*W, sn = (C + 3) * sc
    "cslice_frame": ((1, 1, 3), True, None),    # sn, sc, sd, sh all differ from the dense strides
    # dense rows, strided planes (the form e2_conv3d_fwd_packed_act accepts): a frame of 2 planes
    # leaves sd == H*W, so 2 rows above and below each plane make sd = (H + 4) * W > H*W
    "planes":       ((2, 2, 0), False, None),
    "odd_base":     ((0, 0, 0), False, 1),      # dense strides, storage offset by 1 float
}
GEOM_NAMES = tuple(GEOMS)


def layout(shape5, geom):
    """the numbers make_view works with: strides (sn, sc, sd, sh) in floats, the offset of the
    view's first element in the storage, the margins in front of / behind the holding buffer
    and the storage size"""
    N, C, D, H, W = (int(v) for v in shape5)
    (fd, fh, fw), cslice, phase = GEOMS[geom]
    c0, ct = (2, C + 3) if cslice else (0, C)
    Dp, Hp, Wp = D + 2 * fd, H + 2 * fh, W + 2 * fw
    sh, sd = Wp, Hp * Wp
    sc = Dp * sd
    sn = ct * sc
    inner = c0 * sc + fd * sd + fh * sh + fw
    margin = (sd + 4 + 3) // 4 * 4                   # one plane + a 16-byte piece, whole pieces
    lead = margin
    if phase is not None:
        lead += (phase - (lead + inner)) % 4
    total = lead + N * sn + margin + 4
    return dict(strides=(sn, sc, sd, sh), offset=lead + inner, lead=lead, margin=margin,
                buffer=N * sn, total=total, plane=sd)


def make_view(shape5, geom, seed, device="cuda"):
    """(flat storage, 5-D view into it, clone of the storage, mask of the storage elements
    OUTSIDE the view).  The storage holds distinct finite non-zero floats (multiples of 1/64 up
    to 2^18, random order and signs): no NaN, no zero, no value twice."""
    L = layout(shape5, geom)
    total = L["total"]
    assert total < (1 << 24), "the fill pattern is exact (and distinct) below 2^24 elements"
    rng = np.random.RandomState(seed)
    vals = (rng.permutation(total) + 1).astype(np.float32) / np.float32(64.0)
    vals *= np.where(rng.rand(total) < 0.5, np.float32(-1.0), np.float32(1.0))
    sn, sc, sd, sh = L["strides"]
    N, C, D, H, W = (int(v) for v in shape5)
    offs = (L["offset"] + np.arange(N)[:, None, None, None, None] * sn
            + np.arange(C)[None, :, None, None, None] * sc
            + np.arange(D)[None, None, :, None, None] * sd
            + np.arange(H)[None, None, None, :, None] * sh
            + np.arange(W)[None, None, None, None, :])
    mask = np.ones(total, bool)
    mask[offs.ravel()] = False
    storage = torch.from_numpy(vals).to(device)
    view = storage.as_strided((N, C, D, H, W), (sn, sc, sd, sh, 1), L["offset"])
    return storage, view, storage.clone(), torch.from_numpy(mask).to(device)


def make_slabs(nslab, shape5, geom, seed, device="cuda"):
    """``nslab`` views of ``shape5`` behind one another in ONE watched storage (the partial-sum
    slabs of the split-K "parts" form): (storage, (nslab, N, C, D, H, W) view, clone, mask)"""
    N = int(shape5[0])
    storage, view, clone, mask = make_view((nslab * N,) + tuple(shape5[1:]), geom, seed, device)
    return storage, view.unflatten(0, (nslab, N)), clone, mask


def assert_outside_untouched(storage, clone, mask):
    """the int32 bit patterns of every storage element outside the view are what they were"""
    bad = (storage.view(torch.int32) != clone.view(torch.int32)) & mask
    if bool(bad.any()):
        at = bad.nonzero().flatten()
        raise AssertionError("%d storage element(s) outside the view were written; first at %s: %s (was %s)"
                             % (at.numel(), at[:8].tolist(), storage[at[:8]].tolist(),
                                clone[at[:8]].tolist()))
