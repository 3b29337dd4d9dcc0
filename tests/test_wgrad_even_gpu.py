"""GPU: the weight-gradient GEMM with EVEN position ranges ("MT,NT,9,B,G" / "MT,NT,8,B,G", B >= 1,
csrc/conv_pw_wgrad.hip pw_wgrad_ev_kernel, ranges from csrc/wgrad_even.hpp) against the CPU
oracle -- the oracle, the padded-gradient helper and the bound TOL of
test_ops_gpu.test_conv3d_wgrad_as_position_split_gemm, on three of its problems."""
import numpy as np
import pytest
import torch

from oracle import e2_oracle as O
from test_ops_gpu import TOL, dev, relerr, _plan_style_padded

pytestmark = pytest.mark.gpu

N = 2
PROBLEMS = [(40, 200, (1, 3, 3), (3, 11, 23)),      # 13 x 2: 12 tiles
            (33, 150, (2, 4, 4), (3, 14, 17)),
            (9, 100, (2, 3, 3), (4, 12, 21))]
# G = 1, 5: several tiles per work-group; 12: one tile each (13 x 2, first problem); 31, 256: tile
# boundaries inside a range, segments whose unit counts are no multiples of 4; 1000: more
# work-groups than (tile, unit) pairs
FORCED = ["%s,9,1,%d" % (t, g) for t in ("13,2", "7,2") for g in (1, 5, 12, 31, 256, 1000)] + ["2,4,9,1,31"]
# ... and the band-major order ("MT,NT,9,B,G", B > 1 bands of positions): ranges that cross tiles
# inside a band and bands; a grid of a multiple of 8 work-groups (the XCD-grouped order) and not;
# as many bands as the second problem has units (bands of one round of the four waves then)
FORCED += ["13,2,9,4,31", "13,2,9,3,256", "7,2,9,5,40", "7,2,9,24,37", "2,4,9,2,1000"]

_cache = {}


def problem(ci, co, k, sp):
    """inputs and the oracle's dW of one problem: computed once, shared by its cases, never written"""
    key = (ci, co, k, sp)
    if key not in _cache:
        rng = np.random.RandomState(ci + co)
        x = rng.rand(N, ci, *sp).astype(np.float32)
        wshape = (co, ci) + tuple(k)
        osp = tuple(s - kk + 1 for s, kk in zip(sp, k))
        dy = rng.randn(N, co, *osp).astype(np.float32)
        _cache[key] = (x, dy, O.conv3d_wgrad(dy, x, wshape))
    return _cache[key]


@pytest.mark.parametrize("force", FORCED)
@pytest.mark.parametrize("ci,co,k,sp", PROBLEMS)
def test_wgrad_with_taps_even_ranges(ctx, force, ci, co, k, sp):
    x, dy, dw_ref = problem(ci, co, k, sp)
    dyp = _plan_style_padded(dy, k)
    dw = torch.full(dw_ref.shape, float("nan"), device="cuda")
    # x followed by 32 finite floats (e2_set_input_slack): huge, they meet dy's zero border only
    xflat = torch.full((x.size + 32,), 1e30, device="cuda")
    xd = xflat[:x.size].view(x.shape)
    xd.copy_(dev(x))
    ctx.set_tiling("wgrad", force)
    ctx.set_input_slack(128)
    try:
        ctx.conv3d_wgrad_pad(xd, dyp, dw)
        assert ctx.last_launch() == ("wgrad_ks", force, "forced")
        assert relerr(dw, dw_ref) < TOL
        ctx.conv3d_wgrad_pad(xd, dyp, dw, accumulate=True)
        assert ctx.last_launch() == ("wgrad_ks", force, "forced")
        assert relerr(dw, 2 * dw_ref) < TOL
    finally:
        ctx.set_input_slack(0)
        ctx.set_tiling("wgrad", None)


@pytest.mark.parametrize("force", ["7,2,8,1,3", "7,2,8,1,37", "7,2,8,3,16"])
def test_pointwise_wgrad_even_ranges(ctx, force):
    """the 1x1x1 form: K = 273 positions per sample, K % 32 = 17 -- the masked last step runs in
    exactly one segment per tile (3 tiles of 16 units; G = 37: ranges of one or two units)"""
    Ci, Co, sp = 70, 100, (3, 7, 13)
    rng = np.random.RandomState(Ci + Co)
    x = rng.rand(N, Ci, *sp).astype(np.float32)
    dy = rng.randn(N, Co, *sp).astype(np.float32)
    ref = O.conv3d_wgrad(dy, x, (Co, Ci, 1, 1, 1))
    flat = torch.zeros(dy.size + 32, device="cuda")
    dyp = flat[:dy.size].view(dy.shape)
    dyp.copy_(dev(dy))
    dw = torch.full(ref.shape, float("nan"), device="cuda")
    ctx.set_tiling("wgrad", force)
    try:
        ctx.conv3d_wgrad_pad(dev(x), dyp, dw)
        assert ctx.last_launch() == ("pw_wgrad_ks", force, "forced")
        assert relerr(dw, ref) < TOL
        ctx.conv3d_wgrad_pad(dev(x), dyp, dw, accumulate=True)
        assert ctx.last_launch() == ("pw_wgrad_ks", force, "forced")
        assert relerr(dw, 2 * ref) < TOL
    finally:
        ctx.set_tiling("wgrad", None)


def _single_producer(tile, form, rows, cols):
    """the three tilings that give every tile ONE producer: the position split with S = 1, even
    ranges with one work-group walking every tile, even ranges with one work-group per tile"""
    mt, nt = (int(v) for v in tile.split(","))
    tiles = -(-rows // (16 * mt)) * -(-cols // (16 * nt))
    return ["%s,%d,0,1" % (tile, form), "%s,%d,1,1" % (tile, form), "%s,%d,1,%d" % (tile, form, tiles)]


def _assert_same_bits(ctx, forces, launch, run, ref):
    """pw_wgrad_ks_kernel and pw_wgrad_ev_kernel are two hand-kept copies of one tile body
    (DESIGN.md finding 62); this pins them to each other: with one producer per tile a wave gets
    the same units in the same order and the sums are added to a zeroed dw, so the results are
    EQUAL, first write and accumulate -- no tolerance"""
    got = []
    try:
        for force in forces:
            ctx.set_tiling("wgrad", force)
            dw = torch.full(ref.shape, float("nan"), device="cuda")
            run(dw, False)
            assert ctx.last_launch() == (launch, force, "forced")
            first = dw.clone()
            run(dw, True)
            assert ctx.last_launch() == (launch, force, "forced")
            got.append((first, dw))
    finally:
        ctx.set_tiling("wgrad", None)
    assert relerr(got[0][0], ref) < TOL and relerr(got[0][1], 2 * ref) < TOL
    for force, (first, second) in zip(forces[1:], got[1:]):
        assert torch.equal(first, got[0][0]), force
        assert torch.equal(second, got[0][1]), force + " (accumulate)"


@pytest.mark.parametrize("form", [9, 19])
@pytest.mark.parametrize("tile", ["7,2", "13,2", "2,4"])
def test_split_and_even_kernels_same_bits_with_taps(ctx, tile, form):
    """both unit loops (f32 and six products), 6 / 6 / 12 tiles"""
    ci, co, k, sp = PROBLEMS[2]
    x, dy, dw_ref = problem(ci, co, k, sp)
    dyp = _plan_style_padded(dy, k)
    xflat = torch.full((x.size + 32,), 1e30, device="cuda")
    xd = xflat[:x.size].view(x.shape)
    xd.copy_(dev(x))
    ctx.set_input_slack(128)
    try:
        _assert_same_bits(ctx, _single_producer(tile, form, co, ci * int(np.prod(k))), "wgrad_ks",
                          lambda dw, acc: ctx.conv3d_wgrad_pad(xd, dyp, dw, accumulate=acc), dw_ref)
    finally:
        ctx.set_input_slack(0)


@pytest.mark.parametrize("form", [8, 18])
def test_split_and_even_kernels_same_bits_pointwise(ctx, form):
    """the 1x1x1 form of test_pointwise_wgrad_even_ranges: K % 32 = 17, so the masked step runs,
    in the work-group of the last range there and in the segment with the last unit here; 3 tiles"""
    Ci, Co, sp = 70, 100, (3, 7, 13)
    rng = np.random.RandomState(Ci + Co)
    x = rng.rand(N, Ci, *sp).astype(np.float32)
    dy = rng.randn(N, Co, *sp).astype(np.float32)
    ref = O.conv3d_wgrad(dy, x, (Co, Ci, 1, 1, 1))
    flat = torch.zeros(dy.size + 32, device="cuda")
    dyp = flat[:dy.size].view(dy.shape)
    dyp.copy_(dev(dy))
    xd = dev(x)
    _assert_same_bits(ctx, _single_producer("7,2", form, Co, Ci), "pw_wgrad_ks",
                      lambda dw, acc: ctx.conv3d_wgrad_pad(xd, dyp, dw, accumulate=acc), ref)


@pytest.mark.parametrize("force", ["7,2,9,1,0", "7,2,9,1,65537", "7,2,9,100000,37"])
def test_even_ranges_out_of_range_are_refused(ctx, force):
    """e2_last_launch reports the string that ran: a work-group count outside 1 .. 65536 or more
    bands than units is an error, never clamped"""
    from elektronn2_amd.backend import E2Error
    ci, co, k, sp = PROBLEMS[2]
    x, dy, dw_ref = problem(ci, co, k, sp)
    dyp = _plan_style_padded(dy, k)
    dw = torch.zeros(dw_ref.shape, device="cuda")
    xflat = torch.zeros(x.size + 32, device="cuda")
    xd = xflat[:x.size].view(x.shape)
    xd.copy_(dev(x))
    ctx.set_tiling("wgrad", force)
    ctx.set_input_slack(128)
    try:
        with pytest.raises(E2Error, match="even position ranges"):
            ctx.conv3d_wgrad_pad(xd, dyp, dw)
    finally:
        ctx.set_input_slack(0)
        ctx.set_tiling("wgrad", None)
