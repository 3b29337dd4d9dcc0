"""tests/strided_views.py on CPU tensors: the mask is the complement of the view, the stride and
offset facts each geometry promises hold, the margins are there."""
import numpy as np
import pytest
import torch

from strided_views import (GEOM_NAMES, assert_outside_untouched, layout, make_slabs, make_view)

SHAPES = [(1, 5, 2, 7, 13), (2, 3, 3, 19, 4), (1, 6, 2, 23, 3), (2, 7, 2, 5, 16), (1, 1, 1, 1, 1)]


def _all(geom, shape):
    return make_view(shape, geom, seed=hash((geom, shape)) % 1000, device="cpu")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("geom", GEOM_NAMES)
def test_mask_is_the_complement_of_the_view(geom, shape):
    storage, view, clone, mask = _all(geom, shape)
    assert storage.dim() == 1 and tuple(view.shape) == shape and view.stride(4) == 1
    assert mask.dtype == torch.bool and mask.shape == storage.shape
    assert int((~mask).sum()) == int(np.prod(shape))            # no element of the view twice
    probe = torch.zeros_like(storage)
    probe.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(1.0)
    assert torch.equal(probe == 0, mask)                        # found without index arithmetic
    assert view.untyped_storage().data_ptr() == storage.untyped_storage().data_ptr()
    assert torch.equal(storage, clone) and clone.data_ptr() != storage.data_ptr()


@pytest.mark.parametrize("geom", GEOM_NAMES)
def test_fill_pattern_is_distinct_finite_and_nonzero(geom):
    storage, _, _, _ = _all(geom, SHAPES[0])
    v = storage.numpy()
    assert np.isfinite(v).all() and (v != 0).all()
    assert np.unique(np.abs(v)).size == v.size                  # no value twice, whatever the sign
    assert (v < 0).any() and (v > 0).any()
    other, _, _, _ = make_view(SHAPES[0], geom, seed=12345, device="cpu")
    assert not torch.equal(other, storage)                      # the seed matters


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("geom", GEOM_NAMES)
def test_margins(geom, shape):
    """one full plane + 4 floats of watched storage in front of and behind the buffer that holds
    the view: a store that is off by a row, a plane or a 16-byte piece stays in the allocation"""
    storage, view, _, mask = _all(geom, shape)
    L = layout(shape, geom)
    inside = (~mask).nonzero().flatten()
    first, last = int(inside[0]), int(inside[-1])
    assert first == view.storage_offset() == L["offset"]
    assert L["plane"] == view.stride(2) >= shape[3] * shape[4] and L["margin"] >= L["plane"] + 4
    assert first >= L["margin"] and storage.numel() - 1 - last >= L["margin"]
    assert bool(mask[:first].all()) and bool(mask[last + 1:].all())
    assert storage.data_ptr() % 16 == 0                         # offsets below count from a 16-byte boundary


def _dense(shape):
    N, C, D, H, W = shape
    return (C * D * H * W, D * H * W, H * W, W, 1)


@pytest.mark.parametrize("shape", SHAPES[:4], ids=lambda s: "x".join(map(str, s)))
def test_stride_and_offset_facts(shape):
    N, C, D, H, W = shape
    v = {g: _all(g, shape)[1] for g in GEOM_NAMES}
    off = {g: v[g].storage_offset() for g in GEOM_NAMES}
    assert v["dense"].stride() == _dense(shape) and off["dense"] % 4 == 0
    assert v["dense"].is_contiguous()
    # frame (1,1,1): rows two floats longer, first element at an odd float offset
    sn, sc, sd, sh, sw = v["frame111"].stride()
    assert sh == W + 2 and sd == (H + 2) * sh and sc == (D + 2) * sd and sn == C * sc
    assert off["frame111"] % 2 == 1
    # frame (0,2,2)
    sn, sc, sd, sh, sw = v["frame022"].stride()
    assert sh == W + 4 and sd == (H + 4) * sh and sc == D * sd and sn == C * sc
    assert off["frame022"] % 4 == 2
    # channels [2:2+C] of C + 3, spatially dense
    sn, sc, sd, sh, sw = v["cslice"].stride()
    assert (sc, sd, sh) == (D * H * W, H * W, W) and sn == (C + 3) * sc
    L = layout(shape, "cslice")
    assert off["cslice"] - L["lead"] == 2 * sc                  # two channels in front, one behind
    # channel slice + frame (1,1,3): no stride is the dense one
    sn, sc, sd, sh, sw = v["cslice_frame"].stride()
    assert sh == W + 6 and sd == (H + 2) * sh and sc == (D + 2) * sd and sn == (C + 3) * sc
    assert all(a != b for a, b in zip((sn, sc, sd, sh), _dense(shape)[:4]))
    # dense rows, strided planes
    sn, sc, sd, sh, sw = v["planes"].stride()
    assert sh == W and sd > H * W and sc == (D + 4) * sd and sn == C * sc
    # dense strides one float off: the first row base is misaligned, and EVERY row base is
    # when rows are whole 16-byte pieces (W % 4 == 0); other widths walk through all phases
    assert v["odd_base"].stride() == _dense(shape) and off["odd_base"] % 4 == 1
    rows = off["odd_base"] + np.arange(N * C * D * H) * W
    if W % 4 == 0:
        assert (rows % 4 != 0).all()
    else:
        assert set(rows % 4) == {0, 1, 2, 3}
    # every geometry but the control differs from it
    for g in GEOM_NAMES[1:]:
        assert v[g].stride() != v["dense"].stride() or off[g] % 4 != 0, g


def test_slabs_are_views_of_one_storage():
    shape = (1, 5, 2, 7, 13)
    storage, slabs, clone, mask = make_slabs(8, shape, "frame111", 3, device="cpu")
    assert tuple(slabs.shape) == (8,) + shape
    assert slabs.stride()[1:] == slabs[0].stride() and slabs.stride(0) == shape[0] * slabs.stride(1)
    assert slabs[0].stride(3) == shape[4] + 2 and slabs[0].storage_offset() % 2 == 1
    assert int((~mask).sum()) == 8 * int(np.prod(shape))
    slabs[3].fill_(0.0)
    assert float(storage[~mask].abs().min()) == 0.0             # the slab IS storage memory
    assert_outside_untouched(storage, clone, mask)


def test_assert_outside_untouched_sees_one_bit():
    storage, view, clone, mask = _all("cslice", (1, 4, 2, 5, 4))
    view.fill_(float("nan"))                                    # inside: anything goes
    assert_outside_untouched(storage, clone, mask)
    at = view.storage_offset() + 4 * view.stride(1)             # first float of the next channel
    assert bool(mask[at]) and not bool(mask[at - 1])
    for stray in (0.0, float("nan"), -float(storage[at])):      # a zero, a NaN, a flipped sign bit
        storage[at] = stray
        with pytest.raises(AssertionError, match="outside the view"):
            assert_outside_untouched(storage, clone, mask)
        storage[at] = clone[at]
    assert_outside_untouched(storage, clone, mask)
