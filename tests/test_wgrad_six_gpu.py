"""GPU: the weight-gradient GEMMs whose f32 products are made of six bf16 MFMA products
("MT,NT,19,B,G" / "MT,NT,18,B,G", csrc/conv_pw_wgrad.hip pg_six_units; DESIGN.md finding 60) --
against the float64 oracle on the problems and with the bound TOL of test_wgrad_even_gpu, against
the f32 form on the same inputs, and product by product."""
import numpy as np
import pytest
import torch

from oracle import e2_oracle as O
from test_ops_gpu import TOL, dev, relerr, _plan_style_padded

pytestmark = pytest.mark.gpu

N = 2
PROBLEMS = [(40, 200, (1, 3, 3), (3, 11, 23)),
            (33, 150, (2, 4, 4), (3, 14, 17)),
            (9, 100, (2, 3, 3), (4, 12, 21))]
# even ranges, one band: several tiles per work-group, one each, boundaries inside a range, more
# work-groups than pairs; bands; the position-split grid
FORCED = ["13,2,19,1,%d" % g for g in (1, 12, 31, 1000)] + \
         ["7,2,19,1,5", "2,4,19,1,31", "13,2,19,4,31", "7,2,19,0,3", "3,4,19,0,3"]
PW = (70, 100, (3, 7, 13))                           # Ci, Co, spatial: K = 273, K % 32 = 17

_cache = {}


def problem(ci, co, k, sp):
    """inputs and the oracle's dW of one problem: computed once, shared by its cases, never written"""
    key = (ci, co, k, sp)
    if key not in _cache:
        rng = np.random.RandomState(ci + co)
        x = rng.rand(N, ci, *sp).astype(np.float32)
        osp = tuple(s - kk + 1 for s, kk in zip(sp, k))
        dy = rng.randn(N, co, *osp).astype(np.float32)
        _cache[key] = (x, dy, O.conv3d_wgrad(dy, x, (co, ci) + tuple(k)))
    return _cache[key]


def taps_inputs(ci, co, k, sp):
    """device operands as the launch plan lays them out; 1e30 in the 32 floats behind x: they meet
    dy's zero border only, and split into finite pieces"""
    x, dy, ref = problem(ci, co, k, sp)
    dyp = _plan_style_padded(dy, k)
    xflat = torch.full((x.size + 32,), 1e30, device="cuda")
    xd = xflat[:x.size].view(x.shape)
    xd.copy_(dev(x))
    return xd, dyp, ref


def pw_inputs():
    ci, co, sp = PW
    x, dy, ref = problem(ci, co, (1, 1, 1), sp)
    flat = torch.zeros(dy.size + 32, device="cuda")
    dyp = flat[:dy.size].view(dy.shape)
    dyp.copy_(dev(dy))
    return dev(x), dyp, ref


@pytest.mark.parametrize("force", FORCED)
@pytest.mark.parametrize("ci,co,k,sp", PROBLEMS)
def test_six_product_wgrad_with_taps(ctx, force, ci, co, k, sp):
    xd, dyp, ref = taps_inputs(ci, co, k, sp)
    dw = torch.full(ref.shape, float("nan"), device="cuda")
    before = ctx.tiling_fallbacks()
    ctx.set_tiling("wgrad", force)
    ctx.set_input_slack(128)
    try:
        ctx.conv3d_wgrad_pad(xd, dyp, dw)
        assert ctx.last_launch() == ("wgrad_ks", force, "forced")
        e1 = relerr(dw, ref)
        ctx.conv3d_wgrad_pad(xd, dyp, dw, accumulate=True)
        assert ctx.last_launch() == ("wgrad_ks", force, "forced")
        e2 = relerr(dw, 2 * ref)
        print("%s on %s: %.2e, accumulated %.2e" % (force, (ci, co, k, sp), e1, e2))
        assert e1 < TOL
        assert e2 < TOL
        assert ctx.tiling_fallbacks() == before
    finally:
        ctx.set_input_slack(0)
        ctx.set_tiling("wgrad", None)


@pytest.mark.parametrize("force", ["7,2,18,1,3", "7,2,18,1,37", "7,2,18,0,3"])
def test_six_product_pointwise_wgrad(ctx, force):
    """the 1x1x1 form: K % 32 = 17, the masked last step (f32 MFMAs) next to six-product units"""
    xd, dyp, ref = pw_inputs()
    dw = torch.full(ref.shape, float("nan"), device="cuda")
    before = ctx.tiling_fallbacks()
    ctx.set_tiling("wgrad", force)
    try:
        ctx.conv3d_wgrad_pad(xd, dyp, dw)
        assert ctx.last_launch() == ("pw_wgrad_ks", force, "forced")
        e1 = relerr(dw, ref)
        ctx.conv3d_wgrad_pad(xd, dyp, dw, accumulate=True)
        assert ctx.last_launch() == ("pw_wgrad_ks", force, "forced")
        e2 = relerr(dw, 2 * ref)
        print("%s: %.2e, accumulated %.2e" % (force, e1, e2))
        assert e1 < TOL
        assert e2 < TOL
        assert ctx.tiling_fallbacks() == before
    finally:
        ctx.set_tiling("wgrad", None)


def _run(ctx, force, xd, dyp, shape, slack):
    dw = torch.full(shape, float("nan"), device="cuda")
    ctx.set_tiling("wgrad", force)
    if slack:
        ctx.set_input_slack(128)
    try:
        ctx.conv3d_wgrad_pad(xd, dyp, dw)
        assert ctx.last_launch()[1:] == (force, "forced")
    finally:
        ctx.set_input_slack(0)
        ctx.set_tiling("wgrad", None)
    return dw


@pytest.mark.parametrize("f32,six,taps", [("13,2,9,1,31", "13,2,19,1,31", True), ("7,2,9,0,3", "7,2,19,0,3", True),
                                          ("7,2,8,1,3", "7,2,18,1,3", False), ("7,2,8,0,3", "7,2,18,0,3", False)])
def test_six_products_are_of_the_f32_forms_class(ctx, f32, six, taps):
    """same inputs, same tile, same ranges: the six-product error against float64 is at most 3 x
    the f32 form's (finding 50 measured 1.7 x in a micro-benchmark; a dropped or mis-paired piece
    product costs 2^-16 per term, a hundred times that)"""
    xd, dyp, ref = taps_inputs(*PROBLEMS[0]) if taps else pw_inputs()
    e_f32 = relerr(_run(ctx, f32, xd, dyp, ref.shape, taps), ref)
    e_six = relerr(_run(ctx, six, xd, dyp, ref.shape, taps), ref)
    print("%s %.3e | %s %.3e | ratio %.2f" % (f32, e_f32, six, e_six, e_six / e_f32))
    assert e_six <= 3 * e_f32


def _full_mantissa(rng, shape):
    """f32 values with all 24 mantissa bits in use (the last one set), random signs, exponents
    over seven binades"""
    m = (rng.randint(0, 1 << 22, shape).astype(np.int64) << 1 | 1) + (1 << 23)
    v = np.ldexp(m.astype(np.float64), rng.randint(-26, -19, shape)) * rng.choice([-1.0, 1.0], shape)
    f = v.astype(np.float32)
    assert np.all(f.astype(np.float64) == v)
    return f


@pytest.mark.parametrize("force", ["7,2,18,1,3", "7,2,18,0,1", "13,2,18,1,5"])
def test_one_product_per_output(ctx, force):
    """dy[m] is non-zero at ONE position k_m, so dW[m][n] = dy[m][k_m] * x[n][k_m], one product: a
    wrong pairing of the pieces, which a long random sum hides under TOL, shows here.  Bound
    2^-21 |a b|: the three dropped products are below 2^-23 |a b| together, five f32 additions
    of exact piece products add at most 5 * 2^-24 |a b|.  (A missing mid * mid gives 2^-16.)"""
    Co, Ci, sp = 100, 70, (1, 8, 8)                  # 64 positions: two units, no masked step
    rng = np.random.RandomState(7)
    x = _full_mantissa(rng, (1, Ci) + sp)
    dy = np.zeros((1, Co) + sp, np.float32)
    km = rng.randint(0, 64, Co)
    dyf = dy.reshape(Co, 64)
    dyf[np.arange(Co), km] = _full_mantissa(rng, (Co,))
    a = dyf[np.arange(Co), km].astype(np.float64)[:, None]
    b = x.reshape(Ci, 64).astype(np.float64)[:, km].T          # [Co][Ci]
    want = a * b
    flat = torch.zeros(dy.size + 32, device="cuda")
    dyp = flat[:dy.size].view(dy.shape)
    dyp.copy_(dev(dy))
    dw = _run(ctx, force, dev(x), dyp, (Co, Ci, 1, 1, 1), False)
    got = dw.cpu().numpy().astype(np.float64).reshape(Co, Ci)
    worst = float((np.abs(got - want) / np.abs(want)).max())
    print("%s: worst |got - a b| / |a b| = 2^%.2f" % (force, np.log2(max(worst, 1e-300))))
    assert np.all(np.abs(got - want) <= 2.0 ** -21 * np.abs(want))


@pytest.mark.parametrize("force,what", [("7,2,19,1,0", "even position ranges"), ("7,2,19,1,65537", "even position ranges"),
                                        ("7,2,19,100000,37", "even position ranges")])
def test_six_product_ranges_out_of_range_are_refused(ctx, force, what):
    from elektronn2_amd.backend import E2Error
    xd, dyp, ref = taps_inputs(*PROBLEMS[2])
    dw = torch.zeros(ref.shape, device="cuda")
    ctx.set_tiling("wgrad", force)
    ctx.set_input_slack(128)
    try:
        with pytest.raises(E2Error, match=what):
            ctx.conv3d_wgrad_pad(xd, dyp, dw)
    finally:
        ctx.set_input_slack(0)
        ctx.set_tiling("wgrad", None)


def test_six_product_pointwise_ranges_out_of_range_are_refused(ctx):
    from elektronn2_amd.backend import E2Error
    xd, dyp, ref = pw_inputs()
    dw = torch.zeros(ref.shape, device="cuda")
    for force in ("7,2,18,1,0", "7,2,18,100000,37"):
        ctx.set_tiling("wgrad", force)
        try:
            with pytest.raises(E2Error, match="even position ranges"):
                ctx.conv3d_wgrad_pad(xd, dyp, dw)
        finally:
            ctx.set_tiling("wgrad", None)


@pytest.mark.parametrize("force,taps", [("7,2,19,1,5", True), ("7,2,19,0,3", True), ("7,2,18,1,3", False)])
def test_six_products_are_refused_in_bf16_mode(ctx, force, taps):
    """an error of the launcher, in the words of the limit of the form it extends -- not a fallback"""
    from elektronn2_amd.backend import E2Error
    xd, dyp, ref = taps_inputs(*PROBLEMS[2]) if taps else pw_inputs()
    dw = torch.zeros(ref.shape, device="cuda")
    before = ctx.tiling_fallbacks()
    ctx.set_mfma_dtype('bf16')
    ctx.set_tiling("wgrad", force)
    ctx.set_input_slack(128)
    try:
        with pytest.raises(E2Error, match="an f32 kernel, not offered in bf16 mode"):
            ctx.conv3d_wgrad_pad(xd, dyp, dw)
        assert ctx.tiling_fallbacks() == before
    finally:
        ctx.set_input_slack(0)
        ctx.set_tiling("wgrad", None)
        ctx.set_mfma_dtype('f32')
