"""GEMM and pooling outputs written into strided views, per forced tiling.

The training plan's outputs are not dense: with pad_inplace a node's output is the interior of
the zero-framed image of its 'same' / 'full' consumers ("the frame is zero from here on (nothing
ever writes it)", plan.py), UpConv / Concat outputs are channel slices of wider buffers, the
pooling backward writes the interior of a padded gradient buffer.  The kernels have store code
of their own for these cases (wide epilogue with osY != Wo, narrow / atomic / scatter epilogue,
igemm_zero_output through e2i_fill_view, the pointwise GEMM's row offsets, pw_store4 / pw_storeN
on 4-byte-aligned vectors).  Every case here launches into a view inside watched storage
(tests/strided_views.py) and checks

  * the view against the float64 oracle: 2e-5 of the reference's max magnitude (TOL of
    test_ops_gpu.py, the bound of the exact-f32 MFMA path), or the tighter bound test_ops_gpu.py
    already holds the op to (pooling passes: 1e-7, max-pool forward: exact),
  * that no NaN is left in the view (it is NaN before the launch),
  * that no bit of the storage outside the view changed,
  * without atomics (split count 1, the slab "parts" form): bit equality with the same launch
    into a dense tensor -- the same GEMM in the same order, only the store differs,
  * that e2_last_launch names the kernel family the case is meant to exercise.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import e2_oracle as O
from strided_views import GEOM_NAMES, assert_outside_untouched, make_slabs, make_view

pytestmark = pytest.mark.gpu
TOL = 2e-5
NAN = float("nan")
F32 = np.float32


def dev(a):
    return torch.tensor(np.asarray(a, F32), device="cuda")


def relerr(got, ref):
    got = got.detach().cpu().numpy().astype(np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)          # shared between cases: stays what it is
    return arrays


def nan_view(shape, geom, seed):
    """(storage, view, clone, mask) with the view itself set to NaN"""
    store, view, clone, mask = make_view(tuple(int(v) for v in shape), geom, seed)
    view.fill_(NAN)
    return store, view, clone, mask


def check(watched, ref, tol, dense=None, what=""):
    """value / NaN / surroundings / bit-equality checks of one launch; tol None: exact"""
    store, view, clone, mask = watched
    e = relerr(view, ref)
    print(what, "relerr %.3g" % e)
    assert not bool(torch.isnan(view).any()), what
    assert (e == 0.0) if tol is None else (e < tol), (what, e)
    assert_outside_untouched(store, clone, mask)
    if dense is not None:
        assert same_bits(view, dense), what


def batch_of(geom):
    return 2 if geom == "cslice_frame" else 1


def crop_of(*keys):
    """half of the conv cases read x as the interior crop [:, :, 1:-1, 2:-3, 3:-2] of a larger
    tensor (isY > W: the LDS-DMA span loads depend on it) -- a fixed function of the case"""
    return sum(sum(map(ord, str(k))) for k in keys) % 2 == 1


def as_input(a, crop, border=(0, 0, 0)):
    """device tensor of ``a`` inside a zero border (the padded gradient buffer of a data
    gradient); crop: all of that the interior of a larger tensor of finite junk"""
    N, C = a.shape[:2]
    sp = [a.shape[2 + i] + 2 * border[i] for i in range(3)]
    if crop:
        big = torch.full((N, C, sp[0] + 2, sp[1] + 5, sp[2] + 5), 7.5, device="cuda")
        buf = big[:, :, 1:-1, 2:-3, 3:-2]
        assert buf.stride(3) > sp[2]
    else:
        buf = torch.empty((N, C) + tuple(sp), device="cuda")
    buf.fill_(0.0)
    b = border
    buf[:, :, b[0]:b[0] + a.shape[2], b[1]:b[1] + a.shape[3], b[2]:b[2] + a.shape[4]] = dev(a)
    return buf


# ---- a. conv forward and data gradient ------------------------------------------------------------
# output width -> height: H * W is no multiple of 64 (a tail tile) and > 64 (two tiles at NT = 1).
# 13: pieces of 4 straddle row ends at every phase; 4: the boundary of Wo >= 4; 3: the narrow form
# for strided rows; 16: no straddle
OUT_HW = {13: 7, 4: 19, 3: 23, 16: 5}
WIDTHS = tuple(OUT_HW)


@functools.lru_cache(maxsize=None)
def conv_problem(op, N, W, k, ci, co):
    """(input, weights, float64 reference) of one forward ('fwd': output (N, co, 2, H, W)) or data
    gradient ('dgrad': dx (N, ci, kd + 1, H, W)); computed once, shared, read-only"""
    rng = np.random.RandomState(1000 + 7 * W + 31 * N + 101 * k[2] + k[0] + (op == "dgrad") + ci)
    H = OUT_HW[W]
    w = (rng.randn(co, ci, *k) / np.sqrt(ci * np.prod(k))).astype(F32)
    if op == "fwd":
        x = rng.rand(N, ci, 2 + k[0] - 1, H + k[1] - 1, W + k[2] - 1).astype(F32)
        return frozen(x, w, O.conv3d_fwd(x, w))
    dxs = (N, ci, k[0] + 1, H, W)
    dy = rng.randn(N, co, 2, H - k[1] + 1, W - k[2] + 1).astype(F32)
    return frozen(dy, w, O.conv3d_dgrad(dy, w, dxs))


def expected_tiling(force):
    return force + ",32,0" if force.startswith("1,") and force.count(",") == 2 else force


def run_conv(ctx, op, geom, W, k, ci, co, force, family, atomic):
    """one conv launch (packing inside) into a ``geom`` view + the dense twin when no atomics run"""
    N = batch_of(geom)
    inp, w, ref = conv_problem(op, N, W, k, ci, co)
    crop = crop_of(op, geom, W, k, force)
    src = as_input(inp, crop, (0, 0, 0) if op == "fwd" else tuple(kk - 1 for kk in k))
    wd = dev(w)
    call = ctx.conv3d_fwd if op == "fwd" else ctx.conv3d_dgrad
    watched = nan_view(ref.shape, geom, seed=W + len(geom))
    dense = None
    ctx.set_tiling("igemm", force)
    try:
        call(src, wd, watched[1])
        ll = ctx.last_launch()
        if atomic is None:                      # the library's tiling: "MT,NT,CC,SK" says
            atomic = int(ll[1].split(",")[3]) > 1
        if not atomic:
            dense = torch.full(ref.shape, NAN, device="cuda")
            call(src, wd, dense)
    finally:
        ctx.set_tiling("igemm", None)
    what = "%s %s W=%d k=%s crop=%d %s -> %s" % (op, geom, W, k, crop, force, " ".join(ll))
    if force:
        assert ll == (family, expected_tiling(force), "forced"), what
    else:
        assert ll[0] == family and ll[2] == "model", what
    check(watched, ref, TOL, dense, what)


# tiling strings test_ops_gpu.py runs on ci = 22 (20), co = 24, k = (3, 2, 3): known to fit.
# (string, family e2_last_launch must name, atomics?)
IGEMM_FORMS = [
    ("2,1,8,1", "igemm", False),                 # 16x16x4, wide epilogue, NT = 1
    ("2,2,8,1", "igemm", False),                 # NT = 2
    ("2,4,16,1", "igemm", False),                # NT = 4
    ("2,1,8,4", "igemm", True),                  # split-K: atomics + igemm_zero_output
    ("2,4,16,3", "igemm", True),
    ("4,5,1,8,1,1,4,1", "igemm4", False),        # 4x4x1, plain
    ("4,5,1,8,4,1,4,1", "igemm4", True),         # 4x4x1, split
]


@pytest.mark.parametrize("force,family,atomic", IGEMM_FORMS, ids=[f[0] for f in IGEMM_FORMS])
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("geom", GEOM_NAMES)
def test_conv_fwd_and_dgrad_into_views(ctx, geom, W, force, family, atomic):
    """ci = 22, co = 24 (tile rows past Cout), k = (3, 2, 3): forward into the view, and the data
    gradient with the view as dx (the interior of the previous layer's padded gradient buffer)"""
    for op in ("fwd", "dgrad"):
        run_conv(ctx, op, geom, W, (3, 2, 3), 22, 24, force, family, atomic)


@pytest.mark.parametrize("W", (13, 16))
@pytest.mark.parametrize("kw", (1, 4, 5))
@pytest.mark.parametrize("geom", ("frame111", "cslice_frame", "odd_base"))
def test_conv_tap_widths_into_views(ctx, geom, kw, W):
    """the other specialised tap widths (3 is the case above) in the no-split 16x16x4 family"""
    for op in ("fwd", "dgrad"):
        run_conv(ctx, op, geom, W, (2, 2, kw), 22, 24, "2,2,8,1", "igemm", False)


PW_FORMS = [("1,4,1", "pw_gemm", False), ("1,7,2,64,0", "pw_gemm", False),
            ("7,2,32,1", "igemm", False), ("4,13,1,16,1,2,4,1", "igemm4", False)]


@pytest.mark.parametrize("force,family,atomic", PW_FORMS, ids=[f[0] for f in PW_FORMS])
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("geom", GEOM_NAMES)
def test_pointwise_conv_into_views(ctx, geom, W, force, family, atomic):
    """1x1x1 kernel, Ci = 70, Co = 100: the pointwise GEMM ("1,MT,NT" / "1,MT,NT,KC,0": row
    offsets per lane) and the two implicit-GEMM kernels on the same problem"""
    for op in ("fwd", "dgrad"):
        run_conv(ctx, op, geom, W, (1, 1, 1), 70, 100, force, family, atomic)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("geom", GEOM_NAMES)
def test_generic_tap_width_into_views(ctx, geom, W):
    """kw = 2 has no specialised instance: the generic kernel (narrow epilogue) with the
    library's own tiling"""
    for op in ("fwd", "dgrad"):
        run_conv(ctx, op, geom, W, (2, 2, 2), 22, 24, None, "igemm_generic", None)


# ---- b. split-K zero fill ---------------------------------------------------------------------
@pytest.mark.parametrize("force,family", [("2,1,8,4", "igemm"), ("4,5,1,8,4,1,4,1", "igemm4")])
@pytest.mark.parametrize("geom,N", [("frame111", 1), ("cslice", 2), ("cslice_frame", 2),
                                    ("cslice", 1), ("dense", 1)])
def test_split_k_clears_the_view_and_nothing_else(ctx, geom, N, force, family):
    """atomics accumulate onto the output, so the library clears it first: the view (NaN before
    the launch) and nothing around it.  A strided view is cleared through e2i_fill_view, which
    records no flat fill and does not read e2_set_skip_zero_fill; a view that is one flat run
    (dense; the channel slice of ONE sample) is noted for the caller and left to it under the
    flag"""
    W, k = 13, (3, 2, 3)
    x, w, ref = conv_problem("fwd", N, W, k, 22, 24)
    xd, wd = dev(x), dev(w)
    flat = geom == "dense" or (geom == "cslice" and N == 1)
    ctx.set_tiling("igemm", force)
    try:
        for skip in (False, True):
            watched = nan_view(ref.shape, geom, seed=5 + skip)
            ctx.set_skip_zero_fill(skip)
            ctx.conv3d_fwd(xd, wd, watched[1])
            ptr, n = ctx.conv_last_zero_fill()
            assert ctx.last_launch() == (family, force, "forced")
            what = "%s N=%d %s skip=%d" % (geom, N, force, skip)
            if flat:
                assert (ptr, n) == (watched[1].data_ptr(), watched[1].numel()), what
                if skip:                       # the caller's fill: NaN + sums stays NaN
                    assert bool(torch.isnan(watched[1]).all()), what
                    assert_outside_untouched(watched[0], watched[2], watched[3])
                    continue
            else:
                assert n == 0, what
            check(watched, ref, TOL, None, what)
    finally:
        ctx.set_skip_zero_fill(False)
        ctx.set_tiling("igemm", None)


# ---- c. slab form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", [(1, 2, 2), (2, 2, 2), (1, 1, 1)])
@pytest.mark.parametrize("force,family", [("2,1,8,4", "igemm"), ("2,4,16,3", "igemm"), ("2,2,8,1", "igemm"),
                                          ("4,5,1,8,4,1,4,1", "igemm4")])
def test_partial_sum_slabs_as_framed_views(ctx, force, family, pool):
    """split-K without atomics: 8 slabs, each the interior of a (1,1,1) frame, all in one watched
    storage.  The conv writes slabs [:n] (their sum is the oracle's result, bit-equal to the
    launch into dense slabs) and nothing else; the pooling pass adds the strided slabs up into
    a strided out; the data gradient's slabs go through bias_act_bwd_out_parts into a strided
    dy"""
    W, k, ci, co = 13, (3, 2, 3), 22, 24
    x, w, y_ref = conv_problem("fwd", 1, W, k, ci, co)
    rng = np.random.RandomState(3)
    b = (rng.randn(co) / 4).astype(F32)
    out_ref = O.bias_act_fwd(O.maxpool3d_fwd(y_ref, pool), b, 'relu')
    ws = torch.empty(ctx.conv_ws_bytes(co, ci, k) // 4 + 64, device="cuda")
    ctx.conv3d_pack(dev(w), 0, ws)
    store, slabs, clone, mask = make_slabs(8, y_ref.shape, "frame111", seed=8)
    slabs.fill_(NAN)
    dense = torch.full((8,) + y_ref.shape, NAN, device="cuda")
    xd = dev(x)
    ctx.set_tiling("igemm", force)
    try:
        n = ctx.conv3d_fwd_packed_parts(xd, ws, co, k, slabs)
        assert ctx.last_launch() == (family, force, "forced")
        assert ctx.conv3d_fwd_packed_parts(xd, ws, co, k, dense) == n
    finally:
        ctx.set_tiling("igemm", None)
    want = min(int(force.split(",")[4 if force.startswith("4,") else 3]), 8)
    assert (1 <= n <= want) if force.startswith("4,") else (n == want), (n, want)
    assert bool(torch.isnan(slabs[n:]).all()) and not bool(torch.isnan(slabs[:n]).any())
    assert_outside_untouched(store, clone, mask)
    assert same_bits(slabs[:n], dense[:n])
    assert relerr(slabs[:n].double().sum(0), y_ref) < TOL
    for geom in ("frame111", "cslice_frame"):
        part = slabs.clone()                    # (the pass leaves the sum in slab 0)
        pstore = store.clone()
        parts = pstore.as_strided(slabs.shape, slabs.stride(), slabs.storage_offset())
        out = nan_view(out_ref.shape, geom, seed=9)
        ctx.pool_bias_act_fwd_parts(parts, n, dev(b), pool, 'relu', out[1])
        check(out, out_ref, TOL, None, "pool_bias_act_fwd_parts %s %s" % (pool, geom))
        # the sum is left in slab 0 wherever a pooling window reads (floor semantics: W = 13 and
        # H = 7 leave a column and a row no window reaches -- those keep the first partial sum,
        # and the backward never reads them); the other slabs are only read
        d, h, w_ = (y_ref.shape[2 + i] // pool[i] * pool[i] for i in range(3))
        assert relerr(parts[0][:, :, :d, :h, :w_], y_ref[:, :, :d, :h, :w_]) < TOL
        rest = parts[0].clone()
        rest[:, :, :d, :h, :w_] = part[0][:, :, :d, :h, :w_]
        assert same_bits(rest, part[0]) and same_bits(parts[1:], part[1:])
        assert_outside_untouched(pstore, clone, mask)

    # the data gradient as slabs
    dy, w2, dx_ref = conv_problem("dgrad", 1, W, k, ci, co)
    ctx.conv3d_pack(dev(w2), 1, ws)
    dyp = as_input(dy, False, tuple(kk - 1 for kk in k))
    gstore, gp, gclone, gmask = make_slabs(8, dx_ref.shape, "frame111", seed=10)
    gp.fill_(NAN)
    gdense = torch.full((8,) + dx_ref.shape, NAN, device="cuda")
    ctx.set_tiling("igemm", force)
    try:
        gn = ctx.conv3d_dgrad_packed_parts(dyp, ws, ci, k, gp)
        assert ctx.last_launch() == (family, force, "forced")
        assert ctx.conv3d_dgrad_packed_parts(dyp, ws, ci, k, gdense) == gn
    finally:
        ctx.set_tiling("igemm", None)
    assert 1 <= gn <= want
    assert bool(torch.isnan(gp[gn:]).all()) and not bool(torch.isnan(gp[:gn]).any())
    assert_outside_untouched(gstore, gclone, gmask)
    assert same_bits(gp[:gn], gdense[:gn])
    assert relerr(gp[:gn].double().sum(0), dx_ref) < TOL
    if pool == (1, 1, 1):     # a fused-epilogue producer: slopes from its stored output
        yprod = rng.randn(*dx_ref.shape).astype(F32)
        yprod[0, 0] = np.round(yprod[0, 0] * 2) / 2             # exact zeros of the pre-activation
        bp = (rng.randn(ci) / 4).astype(F32)
        bp[0] = 0.5
        dpre, _ = O.bias_act_bwd(dx_ref.astype(F32), yprod, bp, 'relu')
        outp = dev(O.bias_act_fwd(yprod, bp, 'relu'))
        outp[dev(yprod + bp.reshape(1, -1, 1, 1, 1)) < 0] = -0.0
        for geom in ("frame111", "cslice", "odd_base"):
            d2 = nan_view(dx_ref.shape, geom, seed=11)
            db2 = torch.zeros(ci, device="cuda")
            ctx.bias_act_bwd_out_parts(gp, gn, outp, 'relu', d2[1], db2)
            check(d2, dpre, TOL, None, "bias_act_bwd_out_parts " + geom)
        assert_outside_untouched(gstore, gclone, gmask)        # dout is only read


# ---- d. UpConv ----------------------------------------------------------------------------------
# (Ci, Co, pool, input spatial, act): the pools of test_ops_gpu.UPCONV_CASES, R = 8 and 6
UP_CASES = [(8, 6, (2, 2, 2), (3, 4, 5), 'relu'), (5, 7, (2, 1, 3), (2, 3, 4), 'lin')]
UP_FORMS = [(None, "igemm"), ("2,1,4,1", "igemm"), ("2,1,4,2", "igemm"),        # 16x16x4 scatter (+ atomics)
            ("4,16,1,16,1,2,2,1", "igemm4"), ("4,4,2,16,2,2,3,2", "igemm4"),
            ("1,4,1", "pw_gemm"), ("1,8,1,64,0", "pw_gemm")]


@functools.lru_cache(maxsize=None)
def up_problem(case, N):
    Ci, Co, pool, sp, act = UP_CASES[case]
    rng = np.random.RandomState(13 + case + N)
    x = rng.randn(N, Ci, *sp).astype(F32)
    w = (rng.randn(Co, Ci, *pool) / np.sqrt(Ci)).astype(F32)
    b = rng.randn(Co).astype(F32)
    pre = O.upconv3d_fwd(x, w, pool)
    y_ref = O.bias_act_fwd(pre, b, act)
    dout = rng.randn(*y_ref.shape).astype(F32)
    dpre, db_ref = O.bias_act_bwd(dout, pre, b, act)
    return frozen(x, w, b, y_ref, dout, O.upconv3d_dgrad(dpre, w, pool),
                  O.upconv3d_wgrad(dpre, x, pool), db_ref)


@pytest.mark.parametrize("force,family", UP_FORMS, ids=[str(f[0]) for f in UP_FORMS])
@pytest.mark.parametrize("geom", ("cslice_frame", "frame111"))
@pytest.mark.parametrize("case", range(len(UP_CASES)))
def test_upconv_into_views(ctx, case, geom, force, family):
    """the depth-to-space scatter into a framed output (plan._inplace_frame) and into a framed
    channel slice, all three kernel forms; the backward reads that y and a strided dout and
    writes dx into a frame; dw / dbias do not depend on the views"""
    Ci, Co, pool, sp, act = UP_CASES[case]
    N = batch_of(geom)
    x, w, b, y_ref, dout, dx_ref, dw_ref, db_ref = up_problem(case, N)
    xd, wd, bd = dev(x), dev(w), dev(b)
    nb = ctx.upconv_image_bytes(Co, Ci, pool) // 4 + 64
    wp_f, wp_d = torch.zeros(nb, device="cuda"), torch.zeros(nb, device="cuda")
    ctx.conv3d_pack_multi(*ctx.make_pack_jobs([(wd, wp_f, 2), (wd, wp_d, 3)]))
    ws = torch.empty(ctx.upconv_ws_bytes(Co, Ci, pool, x.shape) // 4 + 64, device="cuda")
    yw = nan_view(y_ref.shape, geom, seed=20 + case)
    gstore, gv, _, _ = make_view(y_ref.shape, geom, seed=21)
    gv.copy_(dev(dout))
    gclone = gstore.clone()
    dxw = nan_view(x.shape, "frame111", seed=22)
    dw = torch.full(w.shape, NAN, device="cuda")
    db = torch.full((Co,), NAN, device="cuda")
    ydense = None
    ctx.set_tiling("igemm", force)
    try:
        ctx.upconv3d_fwd_packed(xd, wp_f, bd, Co, pool, act, yw[1])
        ll = ctx.last_launch()
        atomic = False                          # K splits only where Cin spans several chunks of CC
        if ll[0] != "pw_gemm":
            at = 3 if ll[0] == "igemm4" else 2          # "4,MG,NT,CC,SK,..." / "MT,NT,CC,SK"
            cc, sk = (int(v) for v in ll[1].split(",")[at:at + 2])
            atomic = sk > 1 and Ci > cc
        if not atomic:
            ydense = torch.full(y_ref.shape, NAN, device="cuda")
            ctx.upconv3d_fwd_packed(xd, wp_f, bd, Co, pool, act, ydense)
        what = "upconv %d %s %s -> %s" % (case, geom, force, " ".join(ll))
        assert ll[0] == family and ll[2] == ("forced" if force else "model"), what
        if force:
            assert ll[1] == expected_tiling(force), what
        check(yw, y_ref, TOL, ydense, what)
        ctx.upconv3d_bwd_packed(xd, wp_d, yw[1], gv, pool, act, dxw[1], dw, db, ws)
    finally:
        ctx.set_tiling("igemm", None)
    check(dxw, dx_ref, TOL, None, what + " dx")
    assert same_bits(gstore, gclone) and relerr(yw[1], y_ref) < TOL          # read only
    assert_outside_untouched(yw[0], yw[2], yw[3])
    assert relerr(dw, dw_ref) < TOL and relerr(db, db_ref) < TOL


# ---- e. pooling / bias / activation passes ------------------------------------------------------
POOLS = [(1, 1, 1), (1, 2, 2), (2, 1, 1), (2, 2, 2), (3, 2, 1)]      # four fixed windows + a generic one


@functools.lru_cache(maxsize=None)
def pool_problem(pool, shape):
    rng = np.random.RandomState(11 + sum(pool))
    y = rng.randn(*shape).astype(F32)
    y[0, 0] = np.round(y[0, 0] * 2) / 2              # ties inside windows, exact zeros of the pre-activation
    b = rng.randn(shape[1]).astype(F32)
    b[0] = 0.5
    p_ref = O.maxpool3d_fwd(y, pool)
    out_ref = O.bias_act_fwd(p_ref, b, 'relu')
    dout = rng.randn(*out_ref.shape).astype(F32)
    dp, _ = O.bias_act_bwd(dout, p_ref.astype(F32), b, 'relu')
    base = rng.randn(*shape).astype(F32)
    return frozen(y, b, p_ref, out_ref, dout, O.maxpool3d_bwd(dp, y, pool),
                  O.maxpool3d_bwd(dout, y, pool), base)


def run_pool(ctx, pool, shape, geom):
    y, b, p_ref, out_ref, dout, dy_ref, dx_ref, base = pool_problem(pool, shape)
    yd, bd, gd = dev(y), dev(b), dev(dout)
    tag = "%s %s %s" % (pool, shape, geom)
    out = nan_view(out_ref.shape, geom, seed=30)
    dense = torch.full(out_ref.shape, NAN, device="cuda")
    ctx.pool_bias_act_fwd(yd, bd, pool, 'relu', out[1])
    ctx.pool_bias_act_fwd(yd, bd, pool, 'relu', dense)
    check(out, out_ref, 1e-7, dense, "pool_bias_act_fwd " + tag)

    dy = nan_view(shape, geom, seed=31)
    dense = torch.full(shape, NAN, device="cuda")
    db = torch.zeros(shape[1], device="cuda")
    ctx.pool_bias_act_bwd(gd, yd, bd, pool, 'relu', dy[1], db)
    ctx.pool_bias_act_bwd(gd, yd, bd, pool, 'relu', dense, torch.zeros_like(db))
    check(dy, dy_ref, 1e-7, dense, "pool_bias_act_bwd " + tag)

    mp = nan_view(out_ref.shape, geom, seed=32)
    ctx.maxpool3d_fwd(yd, pool, mp[1])
    check(mp, p_ref, None, None, "maxpool3d_fwd " + tag)

    dx = nan_view(shape, geom, seed=33)
    dense = torch.full(shape, NAN, device="cuda")
    ctx.maxpool3d_bwd(gd, yd, pool, dx[1])
    ctx.maxpool3d_bwd(gd, yd, pool, dense)
    check(dx, dx_ref, 1e-7, dense, "maxpool3d_bwd " + tag)

    store, view, _, mask = make_view(shape, geom, seed=34)
    view.copy_(dev(base))
    clone = store.clone()
    ctx.maxpool3d_bwd(gd, yd, pool, view, accumulate=True)
    check((store, view, clone, mask), base.astype(np.float64) + dx_ref, 1e-6, None,
          "maxpool3d_bwd accumulate " + tag)
    return dy[1], dx[1]


@pytest.mark.parametrize("geom", GEOM_NAMES)
@pytest.mark.parametrize("pool", POOLS, ids=lambda p: "x".join(map(str, p)))
def test_pooling_passes_into_views(ctx, pool, geom):
    """pool_bias_act_fwd -> out, pool_bias_act_bwd -> dy, maxpool3d_fwd / _bwd (also
    accumulate=True) -> views: batch 2, 5 channels, odd widths (pw_store4 / pw_storeN meet rows
    at every 4-byte alignment)"""
    run_pool(ctx, pool, (2, 5, 6 * pool[0], 4 * pool[1], 5 * pool[2]), geom)


@pytest.mark.parametrize("geom", ("frame111", "cslice_frame", "odd_base", "planes"))
@pytest.mark.parametrize("pool", [(2, 2, 2), (1, 2, 2), (3, 2, 1)], ids=lambda p: "x".join(map(str, p)))
def test_pooling_backward_with_extents_the_window_does_not_divide(ctx, pool, geom):
    """floor semantics: the backward first clears dy through e2i_fill_view -- the rows, columns
    and planes no window reaches are exact zeros, the surroundings of the view keep their bits"""
    shape = (batch_of(geom), 3, 5, 7, 9)
    for got in run_pool(ctx, pool, shape, geom):
        g = got.cpu().numpy()
        d, h, w = (shape[2 + i] // pool[i] * pool[i] for i in range(3))
        for rest in (g[:, :, d:], g[:, :, :, h:], g[..., w:]):
            assert np.array_equal(rest.view(np.int32), np.zeros(rest.shape, np.int32))   # +0.0
        assert (d, h, w) != tuple(shape[2:])


# ---- f. fused bias / act epilogue ---------------------------------------------------------------
@pytest.mark.parametrize("force,family", [(None, "igemm"), ("2,2,8,1", "igemm"), ("2,4,16,1", "igemm"),
                                          ("4,5,1,8,1,1,4,1", "igemm4")], ids=str)
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("geom", ("cslice", "planes", "frame111"))
def test_fused_bias_act_epilogue_into_views(ctx, geom, W, force, family):
    """conv3d_fwd_packed_act works into views with dense rows (a channel slice, strided planes)
    and refuses strided rows by name, before anything is written"""
    from elektronn2_amd.backend import E2Error
    k, ci, co = (3, 2, 3), 22, 24
    N = batch_of(geom)
    x, w, y_ref = conv_problem("fwd", N, W, k, ci, co)
    b = (np.random.RandomState(W).randn(co) / 4).astype(F32)
    pre = y_ref + b.reshape(1, -1, 1, 1, 1)
    xd = as_input(x, crop_of(geom, W, force))
    ws = torch.empty(ctx.conv_ws_bytes(co, ci, k) // 4 + 64, device="cuda")
    ctx.conv3d_pack(dev(w), 0, ws)
    watched = nan_view(y_ref.shape, geom, seed=40 + W)
    dense = torch.full(y_ref.shape, NAN, device="cuda")
    ctx.set_tiling("igemm", force)
    try:
        if geom == "frame111":
            before = watched[0].clone()
            with pytest.raises(E2Error, match="dense output rows"):
                ctx.conv3d_fwd_packed_act(xd, ws, co, k, dev(b), 'relu', watched[1])
            torch.cuda.synchronize()
            assert same_bits(watched[0], before)
            return
        ctx.conv3d_fwd_packed_act(xd, ws, co, k, dev(b), 'relu', watched[1])
        ll = ctx.last_launch()
        ctx.conv3d_fwd_packed_act(xd, ws, co, k, dev(b), 'relu', dense)
    finally:
        ctx.set_tiling("igemm", None)
    what = "fused act %s W=%d %s -> %s" % (geom, W, force, " ".join(ll))
    assert ll[0] == family and (ll[1:] == (force, "forced") if force else ll[2] == "model"), what
    check(watched, np.maximum(pre, 0), TOL, dense, what)
    neg = torch.signbit(watched[1]).cpu().numpy()           # -0.0 marks a NEGATIVE pre-activation
    assert neg[pre < -1e-6].all() and not neg[pre > 1e-6].any()


# ---- g. first layer ---------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ("cslice", "odd_base", "frame111"))
def test_first_layer_into_views(ctx, geom):
    """conv1_pool_act_fwd (one input channel, conv + pool + bias + relu in one kernel) with the
    smallest case of test_fused_first_layer: its stores take any strides"""
    k, sp, pool = (1, 4, 4), (1, 19, 11), (1, 2, 2)
    rng = np.random.RandomState(21)
    x = rng.rand(2, 1, *sp).astype(F32)
    w = (rng.randn(20, 1, *k) / 3).astype(F32)
    b = (rng.randn(20) / 4).astype(F32)
    out_ref, _ = O.conv_node_fwd(x, w, b, pool, 'relu')
    watched = nan_view(out_ref.shape, geom, seed=50)
    dense = torch.full(out_ref.shape, NAN, device="cuda")
    ctx.conv1_pool_act_fwd(dev(x), dev(w), dev(b), pool, 'relu', watched[1])
    ctx.conv1_pool_act_fwd(dev(x), dev(w), dev(b), pool, 'relu', dense)
    check(watched, out_ref, TOL, dense, "conv1_pool_act_fwd " + geom)
