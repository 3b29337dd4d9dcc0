"""Pool modes 'average' / 'sum' with a stride of their own and 2-D Pool nodes on the GPU
(csrc/pool.hip: e2_pool3d_lin_fwd / e2_pool3d_lin_bwd; neural.py:1409-1559 and
computations.py:538-649 of the reference).

The reference of every number is the float64 restatement of tests/test_pool_modes_host.py
(``pool_ref``: torch.nn.functional.avg_pool3d, times the window size for 'sum', autograd for the
backward; ``PoolRef`` for whole graphs; pinned there against a NumPy sliding-window loop) -- never the
code under test.  Bounds are the project's own: ops 2e-5 of the reference's largest magnitude
(tests/test_ops_gpu.py:16); loss, prediction and every gradient 1e-4 (tests/test_model_gpu.py:17);
parameters after three Adam steps 5e-4 (DESIGN.md "Tolerances"); one route against another 1e-5
(losses) / 1e-4 (parameters).  Linear pooling takes no decisions: nothing is left out of any
comparison."""
import functools

import numpy as np
import pytest
import torch

from test_dropout_gpu import VIEWS
from test_pool_modes_host import (ADAM, INPUTS, NETS, WINDOWS, WINDOW_IDS, PoolRef, batch_for,
                                  net_chain, net_skip, out_extent, pool_ref, pool_ref_fwd_bwd)

pytestmark = pytest.mark.gpu
TOL = 2e-5
TOL_STEP = 1e-4
TOL_PARAM = 5e-4


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device='cuda')


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


# ---- A. the ops through the C ABI ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def op_case(shape, pool, stride, mode):
    """(x, dout, reference out, reference dx, mask of the elements no window covers): made once
    and shared by the view combinations"""
    rng = np.random.RandomState(abs(hash((shape, pool, stride))) % (2 ** 31))
    x = rng.randn(*shape).astype(np.float32)
    x.flat[::7] = -0.0                                   # (a sign bit a sum from +0 would lose)
    dout = rng.randn(*(shape[:2] + out_extent(shape[2:], pool, stride))).astype(np.float32)
    out, dx = pool_ref_fwd_bwd(x, dout, pool, stride, mode)
    cov = []
    for i, p, s in zip(shape[2:], pool, stride):
        o = (i - p) // s + 1
        cov.append(np.array([any(k * s <= j < k * s + p for k in range(o)) for j in range(i)]))
    covered = cov[0][:, None, None] & cov[1][None, :, None] & cov[2][None, None, :]
    uncovered = np.broadcast_to(~covered, shape)
    assert np.all(dx[uncovered] == 0)
    for a in (x, dout, out, dx):
        a.setflags(write=False)
    return x, dout, out, dx, uncovered


def _outside(make, shape):
    """mask over the storage of a view made by ``make``: True where the view does NOT lie"""
    store, view = make(shape)
    store.fill_(0); view.fill_(1)
    return store == 0


@pytest.mark.parametrize("dview", VIEWS, ids=["dst_" + v[0] for v in VIEWS])
@pytest.mark.parametrize("sview", VIEWS, ids=["src_" + v[0] for v in VIEWS])
@pytest.mark.parametrize("win", WINDOWS, ids=WINDOW_IDS)
@pytest.mark.parametrize("mode", ['avg', 'sum'])
def test_fwd_and_bwd_through_the_c_abi(ctx, mode, win, sview, dview):
    pool, stride = win
    done = 0
    for shape in INPUTS:
        if any(p > i for p, i in zip(pool, shape[2:])):
            continue
        done += 1
        x, dout, ref_out, ref_dx, uncovered = op_case(shape, pool, stride, mode)
        oshape = ref_out.shape
        what = (mode, win, shape)
        # ---- forward: x in a source view, out in a destination view
        sstore, sv = sview[1](shape)
        sstore.fill_(-77.0); sv.copy_(dev(x))
        sbefore = sstore.clone()
        dstore, dv = dview[1](oshape)
        dstore.fill_(-55.0)
        dbefore = dstore.clone()
        ctx.pool_lin_fwd(sv, pool, stride, mode, dv)
        got = dv.cpu().numpy()
        e = rel(got, ref_out)
        assert e < TOL, (what, e)
        assert torch.equal(sstore, sbefore), what
        outside = _outside(dview[1], oshape)
        assert torch.equal(dstore[outside], dbefore[outside]), what
        dstore2, dv2 = dview[1](oshape)
        dstore2.fill_(3.0)
        ctx.pool_lin_fwd(sv, pool, stride, mode, dv2)
        assert np.array_equal(bits(dv2.cpu().numpy()), bits(got)), what
        if mode == 'avg' and pool == (1, 1, 1) and stride == (1, 1, 1):
            assert np.array_equal(bits(got), bits(x)), what
        # ---- backward: dout in a source view, dx in a destination view
        gstore, gv = sview[1](oshape)
        gstore.fill_(-77.0); gv.copy_(dev(dout))
        gbefore = gstore.clone()
        xstore, xv = dview[1](shape)
        xstore.fill_(-55.0)
        xbefore = xstore.clone()
        ctx.pool_lin_bwd(gv, pool, stride, mode, xv)
        gdx = xv.cpu().numpy()
        e = rel(gdx, ref_dx)
        assert e < TOL, (what, e)
        assert np.all(bits(gdx)[uncovered] == 0), what               # +0, not -0, not left over
        assert torch.equal(gstore, gbefore), what
        outside = _outside(dview[1], shape)
        assert torch.equal(xstore[outside], xbefore[outside]), what
        xstore2, xv2 = dview[1](shape)
        xstore2.fill_(3.0)
        ctx.pool_lin_bwd(gv, pool, stride, mode, xv2)
        assert np.array_equal(bits(xv2.cpu().numpy()), bits(gdx)), what
        # ---- accumulate: dx = base + gradient; what no window covers keeps its bits
        rng = np.random.RandomState(3)
        base = rng.randn(*shape).astype(np.float32)
        base.flat[::5] = -0.0
        base.flat[1::11] = np.float32(1e-42)
        xv.copy_(dev(base))
        xbefore = xstore.clone()
        ctx.pool_lin_bwd(gv, pool, stride, mode, xv, accumulate=True)
        acc = xv.cpu().numpy()
        want = base.astype(np.float64) + ref_dx
        assert np.abs(acc - want).max() <= 1e-6 * max(np.abs(want).max(), 1e-30), what
        assert np.array_equal(bits(acc)[uncovered], bits(base)[uncovered]), what
        assert torch.equal(xstore[outside], xbefore[outside]), what
        assert torch.equal(gstore, gbefore), what
    assert done >= 1


def test_rejected_arguments_name_the_entry_point(ctx):
    from elektronn2_amd import backend
    x = torch.zeros((1, 2, 4, 6, 8), device='cuda')
    for name, call in (("e2_pool3d_lin_fwd", lambda p, s, m, small: ctx.pool_lin_fwd(x, p, s, m, small)),
                       ("e2_pool3d_lin_bwd", lambda p, s, m, small: ctx.pool_lin_bwd(small, p, s, m, x))):
        ok = torch.zeros((1, 2, 2, 3, 4), device='cuda')
        call((2, 2, 2), (2, 2, 2), 'avg', ok)
        for small in ((1, 2, 2, 3, 3), (1, 2, 3, 3, 4), (1, 3, 2, 3, 4), (2, 2, 2, 3, 4)):
            with pytest.raises(backend.E2Error, match=name):                 # sizes do not match
                call((2, 2, 2), (2, 2, 2), 'avg', torch.zeros(small, device='cuda'))
        one = torch.zeros((1, 2, 1, 1, 1), device='cuda')
        with pytest.raises(backend.E2Error, match=name):                     # p > in
            call((5, 2, 2), (1, 1, 1), 'avg', one)
        with pytest.raises(backend.E2Error, match=name):
            call((2, 2, 9), (1, 1, 1), 'sum', one)
        with pytest.raises(backend.E2Error, match=name):                     # s < 1
            call((2, 2, 2), (2, 0, 2), 'avg', ok)
        with pytest.raises(backend.E2Error, match=name):                     # p < 1
            call((2, 0, 2), (2, 2, 2), 'avg', ok)
        for bad in (0, 3, -1):
            with pytest.raises(backend.E2Error, match=name):                 # a mode outside the enum
                call((2, 2, 2), (2, 2, 2), bad, ok)


# ---- B. small nets ---------------------------------------------------------------------------------
def pool_nodes(m):
    return [n for n in m.nodes.values() if type(n).__name__ == 'Pool']


def check_loss_and_grads(m, x, t, what=""):
    """loss, every parameter gradient and the gradient with respect to every Pool's parent"""
    ref = PoolRef(m)
    lref, pref = ref.loss_and_grads(x, t)
    loss = float(m.loss(x, t))
    e_l = abs(loss - lref) / abs(lref)
    got = m.gradients(x, t)
    names = list(m.loss_node.all_trainable_params.keys())
    want = ref.grads()
    assert len(got) == len(want) == len(names)
    errs = dict((nme, rel(g, w)) for nme, g, w in zip(names, got, want))
    plan = m._grad_func.func
    for node, w in ref.pool_parent_grads().items():
        g = plan.user_view(node.parent, plan.grad[node.parent]).cpu().numpy()
        if node.mode == 'max':
            # max pooling decides: among the exact zeros a relu parent puts into one window the
            # kernel hands the gradient to every tied maximum, autograd to the first.  Such
            # elements are compared where the parent's relu lets a gradient through, which is all
            # of the gradient that goes on; every linear Pool is compared in full.
            live = ref.val[node.parent].detach().numpy() != 0
            g, w = g * live, w * live
        assert np.abs(w).max() > 0, node.name
        errs["d(%s)" % node.parent.name] = rel(g, w)
    print("%s: loss %.7f ref %.7f (%.1e); gradients worst %s"
          % (what, loss, lref, e_l, sorted(errs.items(), key=lambda kv: -kv[1])[:3]))
    assert e_l < TOL_STEP, (loss, lref)
    for nme, w in zip(names, want):
        assert np.abs(w).max() > 0, nme
    for nme, e in errs.items():
        assert e < TOL_STEP, (nme, e)
    return ref


@pytest.mark.parametrize("name,make,ncls,data_seed", NETS, ids=[n[0] for n in NETS])
def test_whole_steps_against_float64(name, make, ncls, data_seed):
    """loss, prediction, every parameter gradient and every Pool parent's gradient (eager, captured,
    replayed), then loss and parameters over 3 Adam steps (eager, captured, replayed step graph)"""
    m = make()
    x, t = batch_for(m, data_seed, ncls)
    assert any(n.mode != 'max' for n in pool_nodes(m))
    ref = None
    for call in range(3):
        ref = check_loss_and_grads(m, x, t, "%s call %d" % (name, call))
        e = rel(m.predict(x), ref.predict(x))
        print("%s call %d: prediction %.2e" % (name, call, e))
        assert e < TOL_STEP
    for step in range(3):
        lref, _ = ref.loss_and_grads(x, t)
        ref.adam(**ADAM)
        loss = float(m.trainingstep(x, t, optimiser='Adam')[0])
        assert abs(loss - lref) / abs(lref) < TOL_STEP, (step, loss, lref)
        worst = ('', 0.0)
        for nme, p in m.loss_node.all_trainable_params.items():
            e = rel(p.get_value(), ref.p(p).detach().numpy())
            worst = max(worst, (nme, e), key=lambda kv: kv[1])
            assert e < TOL_PARAM, (step, nme, e)
        print("%s step %d: loss %.7f ref %.7f, parameters worst %s" % (name, step, loss, lref, worst))
    assert m.optimisers['Adam'].step.func.use_graph


def _steps(m, x, t, n=3):
    losses = [float(m.trainingstep(x, t, optimiser='Adam')[0]) for _ in range(n)]
    return losses, [p.get_value() for p in m.loss_node.all_trainable_params.values()]


def _same_routes(a, b):
    for u, v in zip(a[0], b[0]):
        assert abs(u - v) < 1e-5 * abs(v), (a[0], b[0])
    assert len(a[1]) == len(b[1])
    for u, v in zip(a[1], b[1]):
        assert rel(u, v) < 1e-4


def test_pool_writes_into_the_framed_image_of_a_same_conv():
    """skip net: with pad_inplace the average Pool's launch writes the interior of the framed image
    its 'same' consumer reads (no pad launch); without it the consumer pads by launch; both agree"""
    from elektronn2_amd.neuromancer import plan_options
    res = {}
    for on in (True, False):
        with plan_options(pad_inplace=on):
            m = net_skip()
            x, t = batch_for(m, 93)
            res[on] = _steps(m, x, t)
            plan = m.optimisers['Adam'].step.func
            same, pool = m.nodes['same'], m.nodes['pool_a']
            assert (same, 'xf') in plan.scratch
            assert ((same, 'xf_launch') not in plan.scratch) == on
            assert ((pool, 'frame') in plan.scratch) == on
            if on:
                assert not plan.out[pool].is_contiguous()
                assert plan.out[pool].data_ptr() == plan.scratch[same, 'xf'][:, :, 0:, 1:, 1:].data_ptr()
    _same_routes(res[True], res[False])


def test_graph_replay_equals_eager():
    from elektronn2_amd.neuromancer import plan_options
    res = {}
    for graph in (True, False):
        with plan_options(graph=graph):
            m = net_chain()
            x, t = batch_for(m, 91)
            res[graph] = _steps(m, x, t, 4)
            assert m.optimisers['Adam'].step.func.use_graph == graph
    _same_routes(res[True], res[False])


# ---- C. around the step ----------------------------------------------------------------------------
@pytest.fixture()
def process_bf16():
    import elektronn2_amd
    elektronn2_amd.set_mfma_dtype('bf16')
    yield
    elektronn2_amd.set_mfma_dtype('f32')


def test_bf16_mode_leaves_the_pool_launches_in_f32(process_bf16):
    """local to the layer: each Pool's output is the float64 pooling of the output its parent
    produced on the device (bf16 rounding upstream does not enter); the step runs"""
    m = net_chain()
    x, t = batch_for(m, 91)
    for node in pool_nodes(m):
        src, got = node.parent(x), node(x)
        want = pool_ref(torch.tensor(src.astype(np.float64)), node.pool_shape, node.pool_stride,
                        node.mode).numpy()
        e = rel(got, want)
        print("bf16 mode, %s (%s): %.2e" % (node.name, node.mode, e))
        assert e < TOL, (node.name, e)
    losses = [float(m.trainingstep(x, t, optimiser='Adam')[0]) for _ in range(3)]
    assert np.isfinite(losses).all()


def test_checkpoint_round_trip(tmp_path):
    from elektronn2_amd import neuromancer as nm
    a = net_chain()
    x, t = batch_for(a, 91)
    for _ in range(2):
        a.trainingstep(x, t, optimiser='Adam')
    f = str(tmp_path / "pool.mdl")
    a.save(f)
    pred = a.predict(x)
    third = float(a.trainingstep(x, t, optimiser='Adam')[0])
    b = nm.modelload(f, name='reloaded')
    b.set_opt_meta_params('Adam', ADAM)
    assert [(n.mode, n.pool_shape, n.pool_stride) for n in pool_nodes(b)] == \
        [(n.mode, n.pool_shape, n.pool_stride) for n in pool_nodes(a)]
    assert np.array_equal(bits(b.predict(x)), bits(pred))
    got = float(b.trainingstep(x, t, optimiser='Adam')[0])
    assert abs(got - third) <= 1e-6 * abs(third), (got, third)


def test_predict_dense_against_the_field_of_view_of_single_voxels():
    m = net_chain(batch=None)
    fov = tuple(int(v) for v in m.prediction_node.shape.fov)
    assert fov == (2, 10, 10)
    assert tuple(int(v) for v in m.prediction_node.shape.strides) == (2, 2, 2)
    rng = np.random.RandomState(6)
    raw = rng.rand(1, 9, 31, 29).astype(np.float32)
    got = m.predict_dense(raw)
    off = tuple(f // 2 for f in fov)
    assert got.shape == (2,) + tuple(s - 2 * o for s, o in zip(raw.shape[1:], off))
    ref = PoolRef(m)
    for (z, a, b) in [(0, 0, 0), (6, 20, 18), (3, 7, 11), (5, 1, 16), (2, 13, 4)]:
        patch = raw[None, :, z:z + fov[0], a:a + fov[1], b:b + fov[2]]
        want = ref.predict(patch)
        assert want.shape == (1, 2, 1, 1, 1)
        assert np.abs(got[:, z, a, b] - want[0, :, 0, 0, 0]).max() < 1e-4, (z, a, b)


def test_several_steps_in_one_graph_equal_single_steps():
    m0 = net_chain()
    x, t = batch_for(m0, 91)

    def fresh():
        mm = net_chain()
        for _ in range(2):
            mm.trainingstep(x, t, optimiser='Adam')
        return mm
    a = fresh()
    single = [float(a.trainingstep(x, t, optimiser='Adam')[0]) for _ in range(3)]
    b = fresh()
    pl = b.optimisers['Adam'].step.func
    ring = torch.empty((3, pl.input_arena.numel()), device='cuda')
    ring[:] = pl.input_arena
    losses, tsec = b.trainingsteps(3, optimiser='Adam', ring=ring)
    assert len(losses) == 3
    for u, v in zip(single, losses):
        assert abs(u - float(v)) / abs(u) < 1e-5, (single, list(losses))
