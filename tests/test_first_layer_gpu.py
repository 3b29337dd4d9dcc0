"""The fused first layer (csrc/conv_first.hip, csrc/conv_first_mfma.hip) against the float64 oracle,
EXACTLY, for every kernel instance: three geometries x MG = 5 / MG = 8 / the VALU fallback.

Inputs on a binary grid (tests/first_layer_cases.py) make every float32 sum exact in any order, so
out, dW and dbias are compared for equality -- no tolerance -- and the pooling window's ties and a
pre-activation of exactly zero really happen (test_first_layer_host.py pins both, and shows that
each wrong variant of a promise fails the very comparison used here).

  * test_exact: the 162 cases of the table (geometry x Cout 1, 3, 17, 20 / 21, 29, 32 / 33, 40 x
    pooled shape A, B, C x relu, lin; N = 2, D = 3).  Forward into NaN; backward onto prefilled
    dW = 3, dbias = -5 with a NaN-filled workspace of EXACTLY conv1_bwd_ws_bytes bytes inside
    watched storage (a NaN in dW: a slot read that nobody wrote; a changed bit outside: the size
    function is short); a second launch on the same workspace gives prefill + 2 * reference.
    These entry points do not report to e2_last_launch, so the kernel family a case runs is
    asserted from Cout alone (first_layer_cases.form: <= 20 MG = 5, <= 32 MG = 8, else VALU) --
    through the workspace size, which is the only thing the library tells about it.
  * test_exact_views: x the interior crop of a tensor that is NaN around it, dout a
    channel-sliced framed view with NaN around it, out into two kinds of view inside watched
    storage, bit-identical to the dense launch.
  * test_exact_persistent: more tiles than the persistent grid, and no multiple of it -- the
    second trip of the tile loop, dW / dbias carried across tiles, one slot per work-group.
  * test_general_floats: rand / randn inputs held to test_fused_first_layer's bound.
  * test_refusals_*: an activation other than relu / lin, a wrong output shape, a short workspace
    and a bf16 image for a VALU channel count are errors that leave the outputs' bits alone.
  * test_first_layer_in_a_net: three hand-built nets whose first node runs the 'first' route,
    loss and every gradient against the oracle.

Measured on an MI355X (256 CUs): 192 cases, 8 s of wall time for the file (the longest case, the
2080-tile VALU one, 2.7 s, most of it the oracle); every exact case exact; general floats at worst
0.0154 of the bound for out (k6p2, Cout 17), 0.0082 for dW (k3p1, Cout 17), 0.0075 for dbias (k6p2,
Cout 40).  No kernel was found wrong.
"""
import numpy as np
import pytest
import torch

import first_layer_cases as FL
from oracle import e2_oracle as O
from strided_views import assert_outside_untouched, make_view

pytestmark = pytest.mark.gpu
TOL = 2e-5               # test_ops_gpu.TOL, the bound test_fused_first_layer holds this layer to
TOL_MODEL = 1e-4         # test_model_gpu.TOL
NAN = float("nan")
F32 = np.float32


def dev(a):
    return torch.tensor(np.asarray(a, F32), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def relerr(got, ref):
    got = host(got).astype(np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def nan_view(shape, geom, seed):
    store, view, clone, mask = make_view(tuple(int(v) for v in shape), geom, seed)
    view.fill_(NAN)
    return store, view, clone, mask


def in_nan(a, geom, seed):
    """``a`` as a view of kind ``geom`` inside storage that is NaN everywhere else"""
    store, view, _, _ = make_view(a.shape, geom, seed)
    store.fill_(NAN)
    view.copy_(dev(a))
    return view


def cropped_in_nan(a):
    """``a`` as the interior crop [:, :, 1:-1, 2:-3, 3:-2] of a larger tensor of NaN"""
    N, C, D, H, W = a.shape
    big = torch.full((N, C, D + 2, H + 5, W + 5), NAN, device="cuda")
    buf = big[:, :, 1:-1, 2:-3, 3:-2]
    buf.copy_(dev(a))
    assert buf.stride(3) > W and bool(torch.isnan(big).any())
    return buf


def watched_workspace(ctx, ref, seed):
    """a NaN-filled workspace of exactly the bytes the size function asks for, inside watched
    storage; the size is the formula of the form Cout selects"""
    N, cout, D, Ho, Wo = ref["dout"].shape
    nbytes = ctx.conv1_bwd_ws_bytes(ref["dout"].shape, ref["k"])
    assert nbytes == 4 * FL.ws_floats(ref["geometry"], cout, N, D, Ho, Wo), (FL.form(cout), nbytes)
    watched = nan_view((1, 1, 1, 1, nbytes // 4), "dense", seed)
    ws = watched[1].reshape(-1)
    assert ws.data_ptr() == watched[1].data_ptr() and ws.numel() * 4 == nbytes
    return watched, ws


def run_exact(ctx, ref, x=None, dout=None, seed=1):
    """forward into NaN, backward onto the prefill with a watched NaN workspace, twice"""
    x = dev(ref["x"]) if x is None else x
    dout = dev(ref["dout"]) if dout is None else dout
    w, b = dev(ref["w"]), dev(ref["b"])
    pool, act = ref["pool"], ref["act"]
    out = torch.full(ref["out"].shape, NAN, device="cuda")
    ctx.conv1_pool_act_fwd(x, w, b, pool, act, out)
    dw = torch.full(ref["w"].shape, FL.PREFILL[0], device="cuda")
    db = torch.full(ref["b"].shape, FL.PREFILL[1], device="cuda")
    watched, ws = watched_workspace(ctx, ref, seed)
    ctx.conv1_pool_act_bwd(x, w, b, dout, pool, act, dw, db, ws=ws)
    FL.check_exact(host(out), host(dw), host(db), ref, FL.PREFILL)
    assert_outside_untouched(watched[0], watched[2], watched[3])
    ctx.conv1_pool_act_bwd(x, w, b, dout, pool, act, dw, db, ws=ws)
    FL.check_exact(None, host(dw), host(db), ref, FL.PREFILL, launches=2)
    assert_outside_untouched(watched[0], watched[2], watched[3])
    return out


@pytest.mark.parametrize("case", FL.TABLE, ids=FL.case_id)
def test_exact(ctx, case):
    ref = FL.table_case(case)
    assert ctx.conv1_supported(1, ref["k"], ref["pool"])
    run_exact(ctx, ref, seed=FL.seed_of(*case) % 1000)


VIEW_CASES = tuple((g, c) for g in FL.GEOMETRIES for c in (20, 29, 40))


@pytest.mark.parametrize("geometry,cout", VIEW_CASES, ids=["%s-c%d" % v for v in VIEW_CASES])
def test_exact_views(ctx, geometry, cout):
    """one channel count per form, shape B, relu: what plan.grad[self], the framed input image and
    the framed / channel-sliced outputs of the training plan look like"""
    ref = FL.table_case((geometry, cout, "B", "relu"))
    x, dout = cropped_in_nan(ref["x"]), in_nan(ref["dout"], "cslice_frame", 11)
    dense = run_exact(ctx, ref, x=x, dout=dout, seed=12)
    plain = torch.full(ref["out"].shape, NAN, device="cuda")
    w, b = dev(ref["w"]), dev(ref["b"])
    ctx.conv1_pool_act_fwd(dev(ref["x"]), w, b, ref["pool"], "relu", plain)
    assert same_bits(dense, plain)
    for n, geom in enumerate(("cslice_frame", "frame111")):
        store, view, clone, mask = nan_view(ref["out"].shape, geom, 13 + n)
        ctx.conv1_pool_act_fwd(x, w, b, ref["pool"], "relu", view)
        FL.check_exact(host(view), None, None, ref, None)
        assert_outside_untouched(store, clone, mask)
        assert same_bits(view, plain), geom


@pytest.mark.parametrize("name", sorted(FL.LONG))
def test_exact_persistent(ctx, name):
    """more tiles than the persistent grid (MFMA forward and backward: min(tiles, 3 * CUs, 1024);
    VALU forward: min(tiles, 8 * CUs)) and not a multiple of it: some work-groups take a second
    tile and some do not.  D grows until the CU count of this device gives both."""
    g, cout, act, N, D, (Ho, Wo) = FL.LONG[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for D in range(D, D + 64):
        ntiles, grid_of = FL.tiles(g, cout, N, D, Ho, Wo)
        grid = grid_of(cus)
        if ntiles > grid and ntiles % grid != 0:
            break
    print(name, "D", D, "tiles", ntiles, "grid", grid, FL.form(cout))
    assert ntiles > grid and ntiles % grid != 0, (cus, ntiles, grid)
    ref = FL.long_case(name, D)
    assert ref["exact_bound"] < 2 ** 24, ref["exact_bound"]
    run_exact(ctx, ref, seed=3)


FLOAT_CASES = tuple((g, c) for g in FL.GEOMETRIES for c in (17, 29, 40))


@pytest.mark.parametrize("geometry,cout", FLOAT_CASES, ids=["%s-c%d" % v for v in FLOAT_CASES])
def test_general_floats(ctx, geometry, cout):
    """values that are not special: the inputs and the bounds of test_fused_first_layer"""
    k, pool = FL.GEOMETRIES[geometry]
    Ho, Wo = FL.pooled_hw(geometry, "B")
    rng = np.random.RandomState(21)
    x = rng.rand(FL.N_SMALL, 1, FL.D_SMALL, Ho * pool[1] + k[1] - 1, Wo * pool[2] + k[2] - 1).astype(F32)
    w = (rng.randn(cout, 1, *k) / 3).astype(F32)
    b = (rng.randn(cout) / 4).astype(F32)
    out_ref, cache = O.conv_node_fwd(x, w, b, pool, 'relu')
    out = torch.full(out_ref.shape, NAN, device="cuda")
    ctx.conv1_pool_act_fwd(dev(x), dev(w), dev(b), pool, 'relu', out)
    dout = rng.randn(*out_ref.shape).astype(F32)
    _, dw_ref, db_ref = O.conv_node_bwd(dout, x, w, b, cache, pool, 'relu', need_dx=False)
    dw = torch.zeros(w.shape, device="cuda"); db = torch.zeros(cout, device="cuda")
    ctx.conv1_pool_act_bwd(dev(x), dev(w), dev(b), dev(dout), pool, 'relu', dw, db)
    errs = dict(out=relerr(out, out_ref), dw=relerr(dw, dw_ref), db=relerr(db, db_ref))
    print(geometry, cout, {n: "%.3g of the bound" % (e / TOL) for n, e in errs.items()})
    for n, e in errs.items():
        assert e < TOL, (n, e)


# ---- refusals -----------------------------------------------------------------------------------------
def pattern(shape, seed):
    """distinct finite floats: a store of any value changes bits"""
    n = int(np.prod(shape))
    vals = (np.random.RandomState(seed).permutation(n) + 1).astype(F32) / F32(64)
    return dev(vals.reshape(shape))


def refusal_case(cout):
    ref = FL.table_case(("k4p2", cout, "B", "relu"))
    return ref, dev(ref["x"]), dev(ref["w"]), dev(ref["b"]), dev(ref["dout"])


def refused(call, what, *kept):
    from elektronn2_amd.backend import E2Error
    before = [t.clone() for t in kept]
    with pytest.raises(E2Error, match=what):
        call()
    torch.cuda.synchronize()
    for t, t0 in zip(kept, before):
        assert same_bits(t, t0)


@pytest.mark.parametrize("cout", (20, 40))
def test_refusals_act(ctx, cout):
    """only relu and lin are computed here: the other E2_ACT_* values are an error, not 'lin'"""
    ref, x, w, b, dout = refusal_case(cout)
    out = pattern(ref["out"].shape, 1)
    dw, db = pattern(ref["w"].shape, 2), pattern(ref["b"].shape, 3)
    for act in ("tanh", "soft+"):
        refused(lambda: ctx.conv1_pool_act_fwd(x, w, b, ref["pool"], act, out), "bad act", out)
        refused(lambda: ctx.conv1_pool_act_bwd(x, w, b, dout, ref["pool"], act, dw, db), "bad act", dw, db)
    ctx.conv1_pool_act_fwd(x, w, b, ref["pool"], "lin", out)         # the neighbouring values pass
    ctx.conv1_pool_act_bwd(x, w, b, dout, ref["pool"], "relu", dw, db)


@pytest.mark.parametrize("cout", (20, 40))
def test_refusals_shape_and_workspace(ctx, cout):
    ref, x, w, b, dout = refusal_case(cout)
    N, _, D, Ho, Wo = ref["out"].shape
    for shape in ((N, cout, D, Ho + 1, Wo), (N, cout, D, Ho, Wo - 1), (N, cout + 1, D, Ho, Wo)):
        out = pattern(shape, 4)
        refused(lambda: ctx.conv1_pool_act_fwd(x, w, b, ref["pool"], "relu", out), "pooled output", out)
    dw, db = pattern(ref["w"].shape, 5), pattern(ref["b"].shape, 6)
    gbad = pattern((N, cout, D, Ho + 1, Wo), 7)
    refused(lambda: ctx.conv1_pool_act_bwd(x, w, b, gbad, ref["pool"], "relu", dw, db), "pooled output", dw, db)
    nfl = ctx.conv1_bwd_ws_bytes(ref["dout"].shape, ref["k"]) // 4
    short = pattern((nfl - 1,), 8)
    refused(lambda: ctx.conv1_pool_act_bwd(x, w, b, dout, ref["pool"], "relu", dw, db, ws=short),
            "workspace too small", dw, db, short)


def test_refusals_bf16_image_of_a_valu_channel_count(ctx):
    """the channels-last bf16 copy is written by the matrix-core form alone (Cout <= 32)"""
    ref, x, w, b, _ = refusal_case(33)
    N, cout, D, Ho, Wo = ref["out"].shape
    kg = (cout + 15) // 16 * 2
    out = pattern(ref["out"].shape, 9)
    nxt = torch.full((N * D * kg * Ho * Wo * 16 + 512,), 0x5a, dtype=torch.uint8, device="cuda")
    before = nxt.clone()
    refused(lambda: ctx.conv1_pool_act_fwd_bf16(x, w, b, ref["pool"], "relu", out, nxt, kg),
            "33 output channels", out)
    assert torch.equal(nxt, before)


# ---- in a net ----------------------------------------------------------------------------------------
NETS = [(12, (1, 4, 4), (1, 2, 2), (3, 31, 31)),
        (24, (1, 6, 6), (1, 2, 2), (3, 31, 31)),
        (40, (1, 3, 3), None, (3, 30, 30))]


@pytest.mark.parametrize("n_f,k,pool,sp", NETS, ids=["k4p2-c12", "k6p2-c24", "k3p1-c40"])
def test_first_layer_in_a_net(n_f, k, pool, sp):
    """MG = 5, MG = 8 and the VALU form as the first node of a net: the plan's framed / strided
    buffers, its workspace, its zeroed gradient slots"""
    from elektronn2_amd import neuromancer as nm
    from test_model_gpu import rel
    from test_tuning_keys_gpu import finish, route
    nm.model_manager.reset()
    np.random.seed(7)
    inp = nm.Input((1, 1) + sp, 'b,f,z,x,y', name='raw')
    c0 = nm.Conv(inp, n_f, k, pool_shape=pool)
    c1 = nm.Conv(c0, 8, (1, 3, 3))
    model, x, t = finish(inp, c1)
    convs = [n for n in model.nodes.values() if type(n) is nm.Conv]
    assert convs[:2] == [c0, c1] and len(convs) == 3
    spec = [(n_f, k, pool or (1, 1, 1), 'relu'), (8, (1, 3, 3), (1, 1, 1), 'relu'),
            (2, (1, 1, 1), (1, 1, 1), 'lin')]
    params = [(n.w.get_value(), n.b.get_value()) for n in convs]
    loss_ref, grads_ref, _ = O.net_loss_and_grads(spec, params, x, t)
    g = model.gradients(x, t)
    plan = model._grad_func.func
    assert route(c0, plan) == 'first' and FL.form(n_f) == {12: "mfma5", 24: "mfma8", 40: "valu"}[n_f]
    assert abs(float(model.loss(x, t)) - loss_ref) / abs(loss_ref) < TOL_MODEL
    names = list(model.loss_node.all_trainable_params.keys())
    assert len(g) == len(names) == 6
    for n, (dw_ref, db_ref) in zip(convs, grads_ref):
        assert rel(g[names.index(n.name + '_w')], dw_ref) < TOL_MODEL, n.name
        assert rel(g[names.index(n.name + '_b')], db_ref) < TOL_MODEL, n.name
