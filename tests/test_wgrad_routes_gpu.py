"""GPU: which kernel a weight-gradient string "MT,NT,WK,BP,PS" runs (csrc/conv_host.hpp
e2_wgrad_route, decoded once in csrc/conv_wgrad.hip e2i_wgrad_conv) -- the LDS-staged and the direct
kernel through both entry points, by the family name e2_last_launch reports, with the result held
to the CPU oracle under test_ops_gpu's TOL; and the strings the decode refuses.  The K-contiguous
GEMMs (WK 7 / 8 / 9) are held by name in test_ops_gpu.py and test_wgrad_even_gpu.py.

One small problem: N = 1, 3 -> 20 channels, kernel (1, 3, 3), output (4, 9, 11).  The padded
gradient lies at the input's row pitch 13 (the launch plan's layout, NaN in its slack), so a plane
spans 8 * 13 + 11 = 115 positions: one 128-tile of the direct kernel per plane, two 64-tiles of the
LDS-staged one.  Cin * T = 27 columns (two 16-blocks, one N tile), 20 rows (two M tiles at MT = 1):
with PS = 4 a launch has 2 * 4 * 1 = 8 work-groups, a whole round of the XCD-grouped order.

Every expectation here was recorded from the library as it was BEFORE the route became a value of
its own (the same test, run against a build of that commit): what it pins is that behaviour."""
import numpy as np
import pytest
import torch

from oracle import e2_oracle as O
from test_ops_gpu import TOL, dev, relerr, _plan_style_padded

pytestmark = pytest.mark.gpu

K = (1, 3, 3)
W_SHAPE = (20, 3) + K
_cache = {}


def problem():
    """inputs and the oracle's dW: computed once, shared by every case, never written"""
    if not _cache:
        rng = np.random.RandomState(23)
        x = rng.rand(1, 3, 4, 11, 13).astype(np.float32)
        dy = rng.randn(1, 20, 4, 9, 11).astype(np.float32)
        _cache['p'] = (x, dy, O.conv3d_wgrad(dy, x, W_SHAPE))
    return _cache['p']


def run_twice(ctx, call, dw_ref, want):
    """overwrite, then accumulate: dw, 2 dw and what e2_last_launch says after each"""
    dw = torch.full(W_SHAPE, float("nan"), device="cuda")
    call(dw, False)
    assert ctx.last_launch() == want
    assert relerr(dw, dw_ref) < TOL
    call(dw, True)
    assert ctx.last_launch() == want
    assert relerr(dw, 2 * dw_ref) < TOL


PADDED = [("1,1,1,128,4", "wgrad_direct"), ("1,2,14,128,4", "wgrad_direct"),
          ("1,1,101,128,4", "wgrad_direct"), ("1,2,114,256,4", "wgrad_direct"),
          ("1,1,0,64,4", "wgrad_lds"), ("1,1,1,64,4", "wgrad_lds"), ("1,1,4,64,4", "wgrad_lds")]


@pytest.mark.parametrize("force,family", PADDED)
def test_padded_entry_runs_the_family_of_the_route(ctx, force, family):
    x, dy, dw_ref = problem()
    xd, dyp = dev(x), _plan_style_padded(dy, K)
    ctx.set_tiling("wgrad", force)
    try:
        run_twice(ctx, lambda dw, acc: ctx.conv3d_wgrad_pad(xd, dyp, dw, accumulate=acc), dw_ref,
                  (family, force, "forced"))
    finally:
        ctx.set_tiling("wgrad", None)


def test_unpadded_entry_reads_wk_1_bp_128_as_the_lds_kernel(ctx):
    """the string that names the direct kernel to the padded entry point"""
    x, dy, dw_ref = problem()
    xd, dyd = dev(x), dev(dy)
    force = "1,1,1,128,4"
    ctx.set_tiling("wgrad", force)
    try:
        run_twice(ctx, lambda dw, acc: ctx.conv3d_wgrad(xd, dyd, dw, accumulate=acc), dw_ref,
                  ("wgrad_lds", force, "forced"))
    finally:
        ctx.set_tiling("wgrad", None)


@pytest.mark.parametrize("padded,force", [(True, "1,1,14,64,4"), (True, "1,1,55,128,1"),
                                          (False, "1,2,14,128,4")])
def test_refused_strings(ctx, padded, force):
    """an E2Error before anything is launched: dw keeps its NaN fill.  e2_last_launch was noted
    before the refusal -- the LDS-staged family, "forced" -- and no fallback is counted."""
    from elektronn2_amd.backend import E2Error
    x, dy, _ = problem()
    xd = dev(x)
    dw = torch.full(W_SHAPE, float("nan"), device="cuda")
    fb0 = ctx.tiling_fallbacks()
    ctx.set_tiling("wgrad", force)
    try:
        with pytest.raises(E2Error, match="wgrad: "):
            if padded:
                ctx.conv3d_wgrad_pad(xd, _plan_style_padded(dy, K), dw)
            else:
                ctx.conv3d_wgrad(xd, dev(dy), dw)
        assert ctx.last_launch() == ("wgrad_lds", force, "forced")
        assert ctx.tiling_fallbacks() == fb0
        assert bool(torch.isnan(dw).all())
    finally:
        ctx.set_tiling("wgrad", None)


def test_the_cost_models_choice_for_the_padded_call(ctx):
    """no string set.  27 columns are two 16-blocks, so choose_wcfg skips its direct-kernel loop and
    prices the LDS-staged kernel; what e2_last_launch names is the kernel the dispatch then runs.
    Recorded: ('wgrad_lds', '1,1,1,64,8', 'model') on 256 CUs -- BP 64, so the kernel that was
    priced is the one that ran (a choice of BP 128 would have run the direct kernel);
    the split count follows the CU count and is not held."""
    x, dy, dw_ref = problem()
    xd, dyp = dev(x), _plan_style_padded(dy, K)
    dw = torch.full(W_SHAPE, float("nan"), device="cuda")
    ctx.conv3d_wgrad_pad(xd, dyp, dw)
    fam, til, src = ctx.last_launch()
    assert relerr(dw, dw_ref) < TOL
    assert (fam, src) == ("wgrad_lds", "model"), (fam, til, src)
