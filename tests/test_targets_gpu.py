"""The target ops of csrc/targets.hip through the C ABI, and the sampler options built on them
(PatchSampler.getbatch: affinities='affinity', nhood_targets, ignore_thresh, ret_ll_mask, NaN ->
-666), on the GPU.

Every op result is a copy, a fill value or 0 / 1: comparisons are for EXACT (bit) equality with the
NumPy restatements of tests/target_cases.py, which tests/test_targets_host.py pins to voxel loops
and to malis.seg_to_affgraph.  Whole training steps use the bounds of the suites they borrow their
nets and references from."""
import ctypes

import numpy as np
import pytest
import torch

import target_cases as tc

pytestmark = pytest.mark.gpu
NAN = float("nan")


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = host(a) if isinstance(a, torch.Tensor) else np.asarray(a, np.float32)
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same(got, want):
    g, w = bits(got), bits(want)
    return g.shape == w.shape and np.array_equal(g, w)


_T = {}


def patch(shape):
    """one read-only patch per shape, shared by the tests"""
    if shape not in _T:
        _T[shape] = tc.patch(shape)
    return _T[shape]


def out_shape(shape, s, c):
    return (shape[0], c) + tc.ext(shape[2:], s)


def run_ops(ctx, t, nh_t, nh_a, s, td=None, outs=None):
    """the three target ops on device tensor ``td`` (default: a dense copy of t) into ``outs``
    (default: fresh NaN-filled dense tensors) -> (stride, nhood, affinity) device tensors"""
    shape = t.shape
    td = dev(t) if td is None else td
    if outs is None:
        outs = [torch.full(out_shape(shape, s, c), NAN, device="cuda")
                for c in (shape[1], len(nh_t) + shape[1] - 1, len(nh_a))]
    ctx.target_stride(td, s, outs[0])
    ctx.target_nhood(td, nh_t, s, outs[1])
    ctx.target_affinity(td, nh_a, s, outs[2])
    torch.cuda.synchronize()
    return outs


OPS = [(sh, s, E) for sh in tc.PATCHES for s in tc.STRIDES for E in sorted(tc.NHOODS)]
OP_IDS = ["%s_s%s_E%d" % ("x".join(map(str, sh)), "".join(map(str, s)), E) for sh, s, E in OPS]


# ---- 1. the kernels through the C ABI ------------------------------------------------------------
@pytest.mark.parametrize("shape,s,E", OPS, ids=OP_IDS)
def test_target_ops_equal_the_restatements(ctx, shape, s, E):
    t = patch(shape)
    nh_a = tc.NHOODS[E]
    nh_t = tc.fit_nhood(nh_a, shape)
    st, nb, af = run_ops(ctx, t, nh_t, nh_a, s)
    assert same(st, tc.stride_np(t, s))
    assert same(nb, tc.nhood_np(t, nh_t, s))
    assert same(af, tc.affinity_np(t, nh_a, s))
    # the wrong variants of the host suite differ from what the kernels wrote wherever they differ
    # from the truth; two of them, as a guard against a vacuous comparison
    if s != (1, 1, 1) and E == 7 and shape[4] > 1:
        assert not same(nb, tc.nhood_np(t, nh_t, s, wrong='stride_first'))
        assert not same(af, tc.affinity_np(t, nh_a, s, wrong='sign'))


def watched(shape, lead, pad):
    """NaN-filled storage with a base 4 bytes off a 16-byte boundary, and the view of extents
    ``shape`` that starts ``lead`` = (c, d, h, w) elements inside it -- a channel slice and an
    interior window at once.  -> (raw 1-D storage, view)"""
    n, c, d, h, w = shape
    full = (n, c + lead[0] + pad[0], d + lead[1] + pad[1], h + lead[2] + pad[2], w + lead[3] + pad[3])
    raw = torch.full((int(np.prod(full)) + 1,), NAN, device="cuda")
    buf = raw[1:].view(full)
    assert buf.data_ptr() % 16 == 4
    view = buf[:, lead[0]:lead[0] + c, lead[1]:lead[1] + d, lead[2]:lead[2] + h, lead[3]:lead[3] + w]
    return raw, view


@pytest.mark.parametrize("shape,s,E", OPS, ids=OP_IDS)
def test_views_in_watched_storage(ctx, shape, s, E):
    """t and every dst as a channel slice / interior window of NaN-filled storage with a misaligned
    base: not a bit changes around the views, and the results are bit-equal to the dense launch"""
    t = patch(shape)
    nh_a = tc.NHOODS[E]
    nh_t = tc.fit_nhood(nh_a, shape)
    dense = run_ops(ctx, t, nh_t, nh_a, s)
    traw, tv = watched(shape, (1, 0, 1, 2), (1, 1, 0, 3))
    tv.copy_(dev(t))
    t_before = traw.clone()
    raws, views = [], []
    for k, c in enumerate((shape[1], len(nh_t) + shape[1] - 1, len(nh_a))):
        raw, v = watched(out_shape(shape, s, c), (2, 1, 1, 1 + k), (0, 0, 2, 2))
        raws.append(raw)
        views.append(v)
    before = [r.clone() for r in raws]
    run_ops(ctx, t, nh_t, nh_a, s, td=tv, outs=views)
    assert same(traw, t_before)
    for raw, v, b, d in zip(raws, views, before, dense):
        assert same(v, d)
        v.copy_(torch.full_like(d, NAN))                    # put the NaN back: all as before
        assert same(raw, b)
    n_neg = tc.count_negative_np(t)
    cnt = torch.tensor([7], dtype=torch.int32, device="cuda")
    ctx.count_negative(tv, cnt)
    assert int(cnt) == 7 + n_neg and same(traw, t_before)


@pytest.mark.parametrize("shape", tc.PATCHES, ids=["x".join(map(str, s)) for s in tc.PATCHES])
def test_count_negative_adds_twice_into_a_non_zero_counter(ctx, shape):
    t = patch(shape)
    n_neg = tc.count_negative_np(t)
    assert 0 < n_neg < tc.count_negative_np(t, wrong='nan_negative')
    cnt = torch.tensor([5, 11], dtype=torch.int32, device="cuda")
    td = dev(t)
    ctx.count_negative(td, cnt)
    ctx.count_negative(td, cnt)
    assert host(cnt).tolist() == [5 + 2 * n_neg, 11]
    big = dev(-np.ones((2, 3, 7, 33, 67)))                  # several work-groups, every lane counts
    big[0, 0, 0, 0, :5] = 1.0
    cnt.zero_()
    ctx.count_negative(big, cnt)
    assert host(cnt).tolist() == [big.numel() - 5, 0]


def test_bad_arguments_are_errors_that_launch_nothing(ctx):
    from elektronn2_amd import backend
    shape = tc.PATCHES[0]
    t = dev(np.nan_to_num(patch(shape)))
    s = (1, 2, 3)
    sp = tc.ext(shape[2:], s)
    out = lambda c, sp=sp: torch.full((shape[0], c) + sp, 7.0, device="cuda")
    nh = tc.NHOODS[3]
    o_s, o_n, o_a = out(2), out(4), out(3)
    big = np.zeros((65, 3), np.int32)
    o_big_n, o_big_a = out(66), out(65)
    bad = [lambda: ctx.target_nhood(t, big, s, o_big_n),                  # E > 64
           lambda: ctx.target_affinity(t, big, s, o_big_a),
           lambda: ctx.target_nhood(t, [[5, 0, 0]], s, out(2)),           # |off| >= extent (5, 9, 11)
           lambda: ctx.target_nhood(t, [[0, -9, 0]], s, out(2)),
           lambda: ctx.target_nhood(t, [[0, 0, 11]], s, out(2)),
           lambda: ctx.target_stride(t, (0, 1, 1), o_s),                  # stride < 1
           lambda: ctx.target_stride(t, s, out(3)),                       # features
           lambda: ctx.target_stride(t, s, out(2, (5, 5, 3))),            # extents (5, 5, 4)
           lambda: ctx.target_nhood(t, nh, s, out(3)),                    # E + C - 1 = 4
           lambda: ctx.target_affinity(t, nh, s, out(4)),                 # E = 3
           lambda: ctx.target_affinity(t[:1], nh, s, o_a)]                # batch
    assert sp == (5, 5, 4)
    for i, f in enumerate(bad):
        with pytest.raises(backend.E2Error):
            f()
            print("bad call %d was accepted" % i)
    with pytest.raises(backend.E2Error):
        vol = torch.zeros((1, 1, 4, 5, 6), device="cuda")
        ctx.ids2barriers(vol, (1, 1, 1), (1, 1, 1), 3, torch.zeros_like(vol))
    # 64 edges are taken
    nh64 = np.zeros((64, 3), np.int32)
    nh64[:, 2] = np.arange(64) % 5 - 2
    o64 = out(64)
    ctx.target_affinity(t, nh64, s, o64)
    torch.cuda.synchronize()
    assert same(o64, tc.affinity_np(host(t), nh64, s))
    for o in (o_s, o_n, o_a, o_big_n, o_big_a):
        assert float(o.min()) == 7.0 and float(o.max()) == 7.0


BARR = [(sh, f) for sh in tc.BARRIER_VOLUMES for f in range(len(tc.BARRIER_FLAGS))]


@pytest.mark.parametrize("sh,f", BARR)
def test_ids2barriers(ctx, sh, f):
    """(6,7,8) and volumes with an axis of length 2; dilute / connectivity all true, all false and
    two mixed settings; the three ecs modes; dense, from a watched view, and through data.image"""
    from elektronn2_amd.data import image
    ids = tc.id_volume(sh)
    dil, conn = tc.BARRIER_FLAGS[f]
    idd = dev(ids)[None, None]
    iraw, iv = watched((1, 1) + sh, (0, 1, 1, 1), (0, 1, 1, 2))
    iv.copy_(idd)
    for ecs, arg in ((0, False), (1, True), (2, 'new_class')):
        want = tc.barriers_np(ids, dil, conn, ecs)
        out = torch.full((1, 1) + sh, NAN, device="cuda")
        ctx.ids2barriers(idd, dil, conn, ecs, out)
        assert same(out[0, 0], want)
        oraw, ov = watched((1, 1) + sh, (0, 2, 0, 3), (0, 0, 1, 1))
        before = oraw.clone()
        ctx.ids2barriers(iv, dil, conn, ecs, ov)
        assert same(ov, out)
        ov.copy_(torch.full_like(out, NAN))
        assert same(oraw, before)
        got = image.ids2barriers(ids, dil, conn, arg)
        assert got.is_cuda and same(got, want)
        assert same(image.ids2barriers(idd[0, 0], dil, conn, arg), want)
    if sh == (6, 7, 8) and all(conn):                        # (the comparison is not vacuous)
        assert not same(out[0, 0], tc.barriers_np(ids, dil, conn, 2, wrong='no_reverse'))


# ---- 2. the sampler --------------------------------------------------------------------------------
PS, STRIDES, OFFS = (9, 30, 30), (1, 2, 3), (2, 5, 5)      # target patch (5, 20, 20) -> (5, 10, 7)


def cubes(nan=False, seed=0):
    """two cubes: images random, targets (ids in blocks with zeros and -1, a smooth channel); the
    target's first channel of cube k holds ids 1 + 10 k .. so that a patch names its cube"""
    rng = np.random.RandomState(seed)
    data, targets = [], []
    for k in range(2):
        sh = (14 + 2 * k, 44, 44)
        data.append(rng.rand(1, *sh).astype(np.float32))
        ids = tc.id_volume(sh, seed=seed + k).copy()
        ids[ids > 0] += 10 * k
        ids[rng.rand(*sh) < 0.1] = -1.0
        reg = rng.rand(*sh).astype(np.float32)
        if nan:
            reg[rng.rand(*sh) < 0.2] = np.nan
            ids[rng.rand(*sh) < 0.05] = np.nan
        targets.append(np.stack([ids, reg]).astype(np.float32))
    return data, targets


def sampler(seed=4, nan=False, strides=STRIDES, **kw):
    from elektronn2_amd.data import PatchSampler
    data, targets = cubes(nan)
    return PatchSampler(data, targets, PS, strides, OFFS, seed=seed, **kw)


KW = dict(grey_augment_channels=[0], warp=0.5)


@pytest.mark.parametrize("nan", [False, True], ids=["nan_free", "nan"])
def test_each_option_equals_the_plain_batch_composed_with_the_restatements(nan):
    """two samplers with one seed: the plain one returns the full-resolution patches
    (force_dense), the restatements make every target form from them"""
    nh7 = tc.DEFAULT_NHOOD
    nh5 = np.array([[0, 0, 0], [-1, 0, 0], [0, 2, 0], [0, 0, -3], [1, -1, 1]], np.int32)
    nh_a = np.array([[-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 2, 1]], np.int32)
    options = [dict(), dict(nhood_targets=True), dict(nhood_targets=nh5),
               dict(affinities='affinity'), dict(affinities='affinity', nhood=nh_a),
               dict(nhood_targets=True, force_dense=True),
               dict(affinities='affinity', nhood=nh_a, force_dense=True)]
    for opt in options:
        plain, other = sampler(nan=nan), sampler(nan=nan)
        assert other.has_nan == nan
        for call in range(2):
            # (the warp's perturbation matrix is drawn from the global generator, as in the
            # reference: transformations.get_random_warpmat)
            np.random.seed(50 + call)
            x0, full = plain.getbatch(2, 'train', force_dense=True, **KW)
            full = host(full)
            if not nan:
                assert not np.isnan(full).any()
            np.random.seed(50 + call)
            got = other.getbatch(2, 'train', **dict(KW, **opt))
            assert len(got) == 2 and same(got[0], x0)
            s = (1, 1, 1) if opt.get('force_dense') else STRIDES
            if 'nhood_targets' in opt:
                nh = nh7 if opt['nhood_targets'] is True else opt['nhood_targets']
                want = tc.nhood_np(full, nh, s)
            elif 'affinities' in opt:
                want = tc.affinity_np(full, opt.get('nhood', np.eye(3, dtype=np.int32)), s)
            else:
                want = tc.stride_np(full, s)
            assert got[1].is_cuda and got[1].dtype == torch.float32
            assert same(got[1], want), opt
        # the options drew no random numbers of their own
        assert plain.rng.rand() == other.rng.rand()


def test_nan_free_plain_path_returns_the_strided_view_itself():
    smp = sampler()
    x, t = smp.getbatch(1, 'train')
    assert tuple(t.shape) == (1, 2, 5, 10, 7) and not t.is_contiguous()
    assert t.stride()[2:] == (400, 40, 3)
    x, t = smp.getbatch(1, 'train', force_dense=True)
    assert t.is_contiguous()


def test_nhood_targets_then_affinities_and_refusals():
    """the reference's order: neighbourhood targets, stride, affinities -- the affinity graph of
    channel 0 of the (already strided) neighbourhood target"""
    a, b = sampler(nan=True), sampler(nan=True)
    nh_a = np.array([[-1, 0, 0], [0, 0, -1]], np.int32)
    x0, full = a.getbatch(1, 'train', force_dense=True)
    x1, aff = b.getbatch(1, 'train', nhood_targets=True, affinities='affinity', nhood=nh_a)
    want = tc.affinity_np(tc.nhood_np(host(full), tc.DEFAULT_NHOOD, STRIDES), nh_a, (1, 1, 1))
    assert same(aff, want)
    with pytest.raises(ValueError):
        b.getbatch(1, 'train', nhood_targets=np.array([[5, 0, 0]]))        # extent 5
    with pytest.raises(ValueError):
        b.getbatch(1, 'train', nhood_targets=np.zeros((65, 3), np.int32))
    with pytest.raises(ValueError):
        b.getbatch(1, 'train', affinities='affinity', nhood=np.zeros((65, 3), np.int32))


def test_ignore_thresh_rejects_the_draws_of_a_host_simulation():
    """a volume with a planted negative half; without grey augmentation a rejected patch consumes
    exactly the draws of an accepted one, so a plain sampler with the same seed yields the
    candidates in order, and the host decides (t < 0).mean() > thresh in float64 for each.  The
    second cube carries a not_present mask: it is never rejected."""
    from elektronn2_amd.data import PatchSampler
    rng = np.random.RandomState(2)
    data = [(0.5 * rng.rand(1, 14, 44, 44) + k).astype(np.float32) for k in range(2)]   # names its cube
    targets = []
    for k in range(2):
        t = rng.randint(1 + 10 * k, 4 + 10 * k, (1, 14, 44, 44)).astype(np.float32)
        t[:, :, :, 22:] = -1.0
        targets.append(t)
    masks = [None, ([1, 0, 1], [0, 1, 0])]
    mk = lambda: PatchSampler(data, targets, PS, STRIDES, OFFS, seed=9, ll_masks=masks)
    plain, other = mk(), mk()
    thresh = 0.5
    accepted, rejected = [], 0
    complete = lambda: (rejected >= 2 and not all(s for _, _, s in accepted) and
                        any(s and (t < 0).mean() > thresh for _, t, s in accepted))
    # (the warp's perturbation matrix comes from the global generator, as in the reference: the
    # same seed in front of either sequence)
    np.random.seed(77)
    while len(accepted) < 40 and not (len(accepted) >= 6 and len(accepted) % 2 == 0 and complete()):
        x, t = plain.getbatch(1, 'train', warp=0.5, force_dense=True)
        t = host(t)
        second = float(x.mean()) > 0.75
        frac = np.float64((t < 0).sum()) / np.float64(t.size)
        if not second and frac > thresh:
            rejected += 1
            continue
        accepted.append((x, t, second))
    # rejections, both cubes, and a patch that only its not_present mask kept
    assert complete(), (rejected, [s for _, _, s in accepted])
    np.random.seed(77)
    for i in range(0, len(accepted), 2):
        x, t, m1, m2 = other.getbatch(2, 'train', warp=0.5, ignore_thresh=thresh,
                                      force_dense=True, ret_ll_mask=True)
        for j in range(2):
            assert same(x[j], accepted[i + j][0][0]) and same(t[j], accepted[i + j][1][0])
            want = masks[1] if accepted[i + j][2] else ([1, 1, 1], [0, 0, 0])
            assert host(m1[j]).tolist() == want[0] and host(m2[j]).tolist() == want[1]
    assert other.n_ignored == rejected
    assert plain.rng.rand() == other.rng.rand()
    # a threshold nothing exceeds rejects nothing; False switches the count off
    for thr in (1.0, False):
        p, o = mk(), mk()
        np.random.seed(78)
        a = p.getbatch(3, 'train', warp=0.5)
        np.random.seed(78)
        b = o.getbatch(3, 'train', warp=0.5, ignore_thresh=thr)
        assert same(a[0], b[0]) and same(a[1], b[1]) and o.n_ignored == 0


def test_ret_ll_mask_returns_the_masks_of_the_cubes_drawn():
    m = [([1, 0, 1, 1], [0, 1, 0, 0]), None]
    smp = sampler(seed=12, ll_masks=m)
    seen = set()
    for _ in range(4):
        x, t, m1, m2 = smp.getbatch(3, 'train', ret_ll_mask=True, **KW)
        assert m1.is_cuda and m1.dtype == torch.float32 and tuple(m1.shape) == tuple(m2.shape) == (3, 4)
        ids = host(t)[:, 0]
        for j in range(3):
            cube = int(ids[j].max() > 10)
            seen.add(cube)
            want = m[0] if cube == 0 else ([1, 1, 1, 1], [0, 0, 0, 0])
            assert host(m1[j]).tolist() == want[0] and host(m2[j]).tolist() == want[1]
    assert seen == {0, 1}
    # all None: L = the target's feature count; the valid source too
    smp = sampler(seed=12, valid=[1])
    x, t, m1, m2 = smp.getbatch(2, 'valid', ret_ll_mask=True)
    assert host(m1).tolist() == [[1, 1]] * 2 and host(m2).tolist() == [[0, 0]] * 2
    from elektronn2_amd.data import PatchSampler
    with pytest.raises(ValueError):
        data, targets = cubes()
        PatchSampler(data, targets, PS, STRIDES, OFFS, ll_masks=[None])


# ---- 3. no host copy, and whole steps --------------------------------------------------------------
def forbid_readbacks(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device tensor was read back on the host")
    for name in ('cpu', 'numpy', 'item', 'tolist'):
        monkeypatch.setattr(torch.Tensor, name, boom)


def affinity_model_and_sampler(seed=1):
    from test_nll_indep_gpu import net_unet
    from elektronn2_amd.data import PatchSampler
    m = net_unet()
    tn = m.target_node
    rng = np.random.RandomState(0)
    vol = rng.rand(1, 14, 40, 40).astype(np.float32)
    ids = np.array(tc.id_volume((14, 40, 40), seed=3))[None]
    smp = PatchSampler([vol], [ids], tuple(m.input_node.shape.spatial_shape), tn.shape.strides,
                       tn.shape.offsets, seed=seed)
    return m, smp


AFF_KW = dict(affinities='affinity',
              nhood=np.array([[-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.int32),
              grey_augment_channels=[0], warp=0.5)


def test_no_target_tensor_is_read_back_on_the_host(monkeypatch):
    from elektronn2_amd.data import RingFeeder
    m, smp = affinity_model_and_sampler()
    d, aff = smp.getbatch(1, 'train', **AFF_KW)
    m.trainingstep(d, aff, optimiser='Adam')                 # builds the plan
    feeder = RingFeeder(smp, m, 'Adam', 2, **AFF_KW)
    nan_smp = sampler(nan=True)
    with monkeypatch.context() as mp:
        forbid_readbacks(mp)
        with pytest.raises(AssertionError):
            torch.zeros(1, device="cuda").item()             # (the patch bites)
        x, a = smp.getbatch(1, 'train', **AFF_KW)
        x, nb = nan_smp.getbatch(2, 'train', nhood_targets=True, **KW)
        x, t, m1, m2 = nan_smp.getbatch(2, 'train', ret_ll_mask=True, **KW)
        feeder.fill()
    torch.cuda.synchronize()
    assert tuple(a.shape) == (1, 3) + tuple(m.target_node.shape.spatial_shape)
    assert tuple(nb.shape) == (2, 8, 5, 10, 7) and not bool(torch.isnan(nb).any())
    assert not bool(torch.isnan(t).any()) and bool((t == -666).any())


def test_ring_feeder_with_affinities_equals_the_same_batches_fed_directly():
    """losses at 1e-5: the bound of tests/test_warp.py's ring-feeder test"""
    from elektronn2_amd.data import RingFeeder
    k = 2
    m, smp = affinity_model_and_sampler()
    ref = []
    for i in range(1 + k):
        d, aff = smp.getbatch(1, 'train', **AFF_KW)
        assert set(np.unique(host(aff))) <= {0.0, 1.0} and bool((aff == 1).any())
        ref.append(float(m.trainingstep(d, aff, optimiser='Adam')[0]))
    m, smp = affinity_model_and_sampler()
    d, aff = smp.getbatch(1, 'train', **AFF_KW)
    got = [float(m.trainingstep(d, aff, optimiser='Adam')[0])]
    feeder = RingFeeder(smp, m, 'Adam', k, **AFF_KW)
    feeder.fill()
    losses, _ = m.trainingsteps(k, optimiser='Adam', ring=feeder.ring)
    got += [float(v) for v in losses]
    print("direct %s, ring %s" % (ref, got))
    for u, v in zip(ref, got):
        assert abs(u - v) <= 1e-5 * abs(u), (ref, got)


def test_lazy_label_masks_from_the_sampler_train_against_the_float64_reference():
    """the net and the float64 reference of tests/test_weighted_nll_gpu.py (its 'generic' path: 5
    classes, both masks), fed from getbatch(ret_ll_mask=True)"""
    import test_weighted_nll_gpu as W
    from oracle import e2_oracle as O
    from elektronn2_amd.data import PatchSampler
    path, ncls = 'generic', 5
    params = O.init_net(W.NETS[path], 1, seed=4)
    m, nll = W.build_net(path, params)
    tn = m.target_node
    rng = np.random.RandomState(5)
    data = [rng.rand(1, 8, 40, 40).astype(np.float32) for _ in range(2)]
    targets = [rng.randint(-1, ncls, (1, 8, 40, 40)).astype(np.float32) for _ in range(2)]
    masks = [([1, 1, 0, 1, 0], [0, 0, 1, 0, 0]), ([0, 1, 1, 1, 1], [1, 0, 0, 0, 0])]
    smp = PatchSampler(data, targets, W.SP, tn.shape.strides, tn.shape.offsets, seed=3,
                       ll_masks=masks)
    for _ in range(16):                                      # until both cubes are in one batch
        x, t, m1, m2 = smp.getbatch(2, 'train', ret_ll_mask=True, grey_augment_channels=[0])
        if not same(m1[0], m1[1]):
            break
    assert not same(m1[0], m1[1])
    ew = torch.ones((2,) + tuple(t.shape[2:]), device="cuda")
    Wd = dict(cw=np.asarray(W.CW0[ncls], np.float32), ew=host(ew), L=host(m1), M=host(m2))
    loss_ref, grads_ref = W.ref_step(path, params, host(x), host(t), Wd)
    loss = float(m.trainingstep(x, t, ew, m1, m2, optimiser='Adam')[0])
    print("lazy labels: loss %.9g ref %.9g" % (loss, loss_ref))
    assert abs(loss - loss_ref) / abs(loss_ref) < W.MODEL_TOL
    Wu = dict(Wd, L=np.ones_like(Wd['L']), M=np.zeros_like(Wd['M']))
    assert abs(W.ref_step(path, params, host(x), host(t), Wu)[0] - loss_ref) > 100 * W.MODEL_TOL * loss_ref


def test_squared_loss_net_on_a_nan_bearing_cube_masks_those_voxels():
    """tests/test_regression_loss_gpu.py's net_b (a lin head under SquaredLoss) and its float64
    restatement RefL; the cube's NaN arrive as -666 and are masked (loss at TOL_STEP)"""
    import test_regression_loss_gpu as R
    from elektronn2_amd.data import PatchSampler
    m = R.net_b()
    tn = m.target_node
    rng = np.random.RandomState(8)
    vol = rng.rand(1, 12, 36, 36).astype(np.float32)
    reg = rng.randn(1, 12, 36, 36).astype(np.float32)
    reg[rng.rand(*reg.shape) < 0.25] = np.nan
    smp = PatchSampler([vol], [reg], tuple(m.input_node.shape.spatial_shape), tn.shape.strides,
                       tn.shape.offsets, seed=2, target_discrete_ix=[0])
    assert smp.has_nan
    x, t = smp.getbatch(1, 'train')
    th = host(t)
    n_masked = int((th == -666.0).sum())
    assert 0 < n_masked < th.size and not np.isnan(th).any()
    ref = R.RefL(m)
    loss_ref, _ = ref.forward({'raw': host(x), 'target': th})
    loss_ref = float(loss_ref.detach())
    name, (_, n_unmasked) = list(ref.terms.items())[0]
    assert n_unmasked == th.size - n_masked
    loss = float(m.trainingstep(x, t, optimiser='Adam')[0])
    print("squared loss on -666: %.9g ref %.9g, %d of %d masked" % (loss, loss_ref, n_masked, th.size))
    assert abs(loss - loss_ref) <= R.TOL_STEP * abs(loss_ref)
    # unmasked, the planted value would dominate the loss
    assert loss < 10.0
