"""csrc/dense_gemm.hip through backend.Context against float64 NumPy, and through the plan (option
``dense_gemm``).  The op bound is derived, not measured: an f32 dot product of length K in ANY
summation order, plus the final add, misses the exact value by at most
(K + 2) 2^-24 (|A| @ |B|) + 2^-24 |base| per element (right-hand side in float64)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_batchnorm_host import (NETS, SGD, TOL_GRAD, TOL_OUT, BnRef, args_of, dense_case, dense_refs,
                                 feed_for, rel)
from test_dense_gemm_host import net_a

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
OPS = ('fwd', 'dgrad', 'wgrad')
SHAPES = [(1, 3, 1), (16, 16, 16), (64, 64, 64), (17, 33, 65), (20, 576, 200), (130, 70, 9), (5, 1030, 19)]
NAN = float("nan")


def dev(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")


def launch(ctx, op, x, w, dy, out, acc, splits, ws=None):
    if op == 'fwd':
        ctx.dense_gemm_fwd(x, w, out, splits=splits, ws=ws)
    elif op == 'dgrad':
        ctx.dense_gemm_dgrad(dy, w, out, accumulate=acc, splits=splits, ws=ws)
    else:
        ctx.dense_gemm_wgrad(x, dy, out, accumulate=acc, splits=splits, ws=ws)
    torch.cuda.synchronize()


def within_bound(got, ref, acc, what):
    a, b, base, prod = ref
    a, b, base = (np.asarray(v, np.float64) for v in (a, b, base if acc else 0.0))
    bound = (a.shape[1] + 2) * U * (np.abs(a) @ np.abs(b)) + U * np.abs(base)
    err = np.abs(got.astype(np.float64) - (prod + base))
    print("%s: worst error / bound %.3f" % (what, float((err / bound).max())))
    assert np.isfinite(got).all() and (err <= bound).all(), (what, float((err / bound).max()))


CASES = [(op, shape, splits, acc) for op in OPS for shape in SHAPES for splits in (1, 4)
         for acc in ((False,) if op == 'fwd' else (False, True))]


@pytest.mark.parametrize("op,shape,splits,acc", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_ops_against_float64(ctx, op, shape, splits, acc):
    from elektronn2_amd import backend
    n, k, m = shape
    c, ref = dense_case(n, k, m), dense_refs(n, k, m)[op]
    rows, red = ref[3].shape[0], ref[0].shape[1]
    out = dev(ref[2]) if acc else torch.full(ref[3].shape, NAN, device="cuda")
    args = (ctx, op, dev(c['x']), dev(c['w']), dev(c['dy']), out, acc, splits)
    limit = -(-red // 4)                      # the header's: ceil(reduction length / 4)
    if splits > limit:
        with pytest.raises(backend.E2Error, match="allows at most %d" % limit):
            launch(*args)
        return
    choice = ctx.dense_gemm_choice(op, n, k, m, splits)
    assert choice['tile'] == ((16, 128) if rows <= 32 else (64, 64)) and choice['splits'] == splits
    launch(*args)
    within_bound(out.cpu().numpy(), ref, acc, (op, n, k, m, splits, acc))


def pitched(a, aligned, fill=None):
    """an (r, c) view of row pitch > c inside NaN-filled storage, holding ``a`` (or ``fill``)"""
    r, c = a.shape
    pitch = c + (4 if aligned else 3)
    st = torch.full(((r + 2) * pitch + 8,), NAN, device="cuda")
    v = st.as_strided((r, c), (pitch, 1), pitch + (4 if aligned else 1))
    v.copy_(dev(a) if fill is None else torch.full_like(v, fill))
    return st, v


@pytest.mark.parametrize("aligned", [False, True], ids=["odd", "aligned"])
@pytest.mark.parametrize("op", OPS)
def test_pitched_views(ctx, op, aligned):
    n, k, m = 18, 36, 68
    c, ref = dense_case(n, k, m), dense_refs(n, k, m)[op]
    (_, x), (_, dy) = pitched(c['x'], aligned), pitched(c['dy'], aligned)
    if op == 'wgrad':
        out = torch.full((k, m), NAN, device="cuda")
        launch(ctx, op, x, dev(c['w']), dy, out, False, 0)
    else:
        st, out = pitched(ref[3], aligned, fill=7.0)
        before = st.clone()
        launch(ctx, op, x, dev(c['w']), dy, out, False, 0)
        inside = torch.zeros_like(st, dtype=torch.bool)
        inside.as_strided(out.shape, out.stride(), out.storage_offset()).fill_(True)
        assert torch.equal(st.view(torch.int32)[~inside], before.view(torch.int32)[~inside])
    within_bound(out.cpu().numpy(), ref, False, (op, aligned))


@pytest.mark.parametrize("op", OPS)
def test_split_k_is_reproducible(ctx, op):
    n, k, m = 20, 576, 200
    c, ref = dense_case(n, k, m), dense_refs(n, k, m)[op]
    outs = [torch.full(ref[3].shape, NAN, device="cuda") for _ in range(2)]
    for o in outs:
        launch(ctx, op, dev(c['x']), dev(c['w']), dev(c['dy']), o, False, 4)
    assert torch.equal(outs[0], outs[1]) and not torch.isnan(outs[0]).any()


def test_refusals(ctx):
    from elektronn2_amd import backend
    lib = backend.lib()
    n, k, m = 20, 576, 200
    t, ws = torch.zeros(k * m, device="cuda"), torch.zeros(4 * k * m, device="cuda")
    p, wp = C.c_void_p(t.data_ptr()), C.c_void_p(ws.data_ptr())
    calls = dict(
        e2_dense_gemm_fwd=(lambda a, ld, nb: lib.e2_dense_gemm_fwd(ctx.h, a, ld, p, p, m, n, k, m, 4, wp, nb),
                           k, 16 * n * m),
        e2_dense_gemm_dgrad=(lambda a, ld, nb: lib.e2_dense_gemm_dgrad(ctx.h, a, ld, p, p, k, n, k, m, 0, 4, wp, nb),
                             m, 16 * n * k),
        e2_dense_gemm_wgrad=(lambda a, ld, nb: lib.e2_dense_gemm_wgrad(ctx.h, a, ld, p, m, p, n, k, m, 1, 4, wp, nb),
                             k, 16 * k * m))
    for name, (call, row, need) in calls.items():
        for bad, text in (((None, row, need), "null"), ((p, row - 1, need), "pitch below the row length"),
                          ((p, row, need - 1), "need a workspace of")):
            with pytest.raises(backend.E2Error, match=text):
                backend._chk(call(*bad), name)
    assert not t.any() and not ws.any()


# ---- nets ------------------------------------------------------------------------------------------
OLD, NEW = ('dense_fwd', 'dense_dgrad', 'dense_wgrad'), ('dense_gemm_fwd', 'dense_gemm_dgrad', 'dense_gemm_wgrad')
# option, net, (data seed, classes, batch), routes.  A under 'auto': the hidden layer's forward (the input takes
# no gradient, its wgrad is below ITS threshold), the head below both.  C: two flatten=True heads on a Conv.
NET_CASES = [('auto', net_a, (7, 10, None), {NEW[0]} | set(OLD)), (False, net_a, (7, 10, None), set(OLD)),
             (True, NETS[2][1], (NETS[2][4], NETS[2][2], NETS[2][3]), set(NEW))]


@pytest.mark.parametrize("option,make,data,routes", NET_CASES, ids=["A-auto", "B-off", "C-forced"])
def test_two_sgd_steps_against_float64_on_the_expected_routes(monkeypatch, option, make, data, routes):
    """loss at TOL_OUT and every parameter at TOL_GRAD against the float64 step reference; the
    Context methods the plan called; net C's second dgrad into the trunk accumulates"""
    from elektronn2_amd import backend
    from elektronn2_amd.neuromancer import plan_options
    calls = []
    for name in OLD + NEW:
        def spy(self, *a, _orig=getattr(backend.Context, name), _name=name, **kw):
            calls.append((_name, bool(kw.get('accumulate', False))))
            return _orig(self, *a, **kw)
        monkeypatch.setattr(backend.Context, name, spy)
    with plan_options(dense_gemm=option):
        m = make()
        m.set_opt_meta_params('SGD', SGD)
        feed, ref = feed_for(m, *data), BnRef(m)
        for step in range(2):
            lref = ref.step(feed, 'SGD')
            loss = float(m.trainingstep(*args_of(m, feed), optimiser='SGD')[0])
            print("step %d: loss %.8f ref %.8f" % (step, loss, lref))
            assert abs(loss - lref) <= TOL_OUT * abs(lref), (step, loss, lref)
    for node in m.nodes.values():
        for key, p in node.params.items():
            if key in ('w', 'b', 'gamma'):
                e = rel(p.get_value(), ref.p(p).detach().numpy())
                assert e <= TOL_GRAD, (node.name, key, e)
    assert set(c[0] for c in calls) == routes, calls
    if option is True:
        assert [c[1] for c in calls if c[0] == NEW[1]][:2] == [False, True], calls


def test_graph_replay_equals_eager_bit_for_bit():
    """net A's gradients three times on the same parameters -- eager, captured, replayed: every weight
    gradient (all behind the hidden layer's split-K GEMM forward) has the same bits.  Bias gradients
    and the loss sum use float atomics in kernels of their own: a whole step never was reproducible."""
    m = net_a()
    args = args_of(m, feed_for(m, 7, 10))
    names = list(m.loss_node.all_trainable_params.keys())
    runs = [dict(zip(names, m.gradients(*args))) for _ in range(3)]
    assert m._grad_func.func.use_graph
    for name in ('hidden_w', 'head_w'):
        assert np.abs(runs[0][name]).max() > 0
        for later in runs[1:]:
            assert np.array_equal(runs[0][name].view(np.int32), later[name].view(np.int32)), name
