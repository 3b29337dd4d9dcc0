"""No GPU: the NumPy restatements of the target ops (tests/target_cases.py) against plain voxel
loops written from the definitions and against malis.seg_to_affgraph; proof that the case table
tells seven deliberate mistakes from the truth; the sampler's ll_masks defaults and validation,
the default neighbourhood, and the refusals that are decided on the host."""
import numpy as np
import pytest

import target_cases as tc


def same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def cases():
    for shape in tc.PATCHES:
        for s in tc.STRIDES:
            for E in sorted(tc.NHOODS):
                yield shape, s, E


CASES = list(cases())
IDS = ["%s_s%s_E%d" % ("x".join(map(str, sh)), "".join(map(str, s)), E) for sh, s, E in CASES]


@pytest.mark.parametrize("shape,s,E", CASES, ids=IDS)
def test_restatements_equal_the_voxel_loops(shape, s, E):
    t = tc.patch(shape)
    assert np.isnan(t).any() and (t < 0).any() and (t == 0).any()
    assert same(tc.stride_np(t, s), tc.stride_loop(t, s))
    nh = tc.fit_nhood(tc.NHOODS[E], shape)
    assert len(nh) >= 1
    got = tc.nhood_np(t, nh, s)
    assert got.shape == (shape[0], len(nh) + shape[1] - 1) + tc.ext(shape[2:], s)
    assert same(got, tc.nhood_loop(t, nh, s)) and not np.isnan(got).any()
    aff = tc.affinity_np(t, tc.NHOODS[E], s)
    assert same(aff, tc.affinity_loop(t, tc.NHOODS[E], s))
    assert set(np.unique(aff)) <= {0.0, 1.0}
    assert tc.count_negative_np(t) == tc.count_negative_loop(t) > 0


@pytest.mark.parametrize("shape,s,E", CASES, ids=IDS)
def test_affinity_restatement_equals_seg_to_affgraph_on_nan_free_ids(shape, s, E):
    from elektronn2_amd import malis
    t = tc.patch(shape, seed=1, nan=False)
    ts = np.rint(t[:, :, ::s[0], ::s[1], ::s[2]])
    nh = tc.NHOODS[E]
    got = tc.affinity_np(t, nh, s)
    # (seg_to_affgraph's slicing takes edges shorter than the volume only; a longer edge leaves
    # the volume from every voxel: all zero)
    short = [e for e in range(E) if all(abs(nh[e, k]) < ts.shape[2 + k] for k in range(3))]
    for e in set(range(E)) - set(short):
        assert not got[:, e].any()
    for b in range(shape[0] if short else 0):
        want = malis.seg_to_affgraph(ts[b, 0], nh[short])
        assert np.array_equal(got[b][short], want.astype(np.float32))


def test_the_case_table_has_the_long_edge_and_the_single_element_row():
    """(0, 5, 0): longer than a strided x extent, shorter than the full-resolution one"""
    assert any(sh[4] == 1 for sh in tc.PATCHES)
    hits = [(sh, s) for sh in tc.PATCHES for s in tc.STRIDES
            if tc.ext(sh[2:], s)[1] <= 5 < sh[3]]
    assert hits
    assert any(sh[2 + k] % s[k] for sh in tc.PATCHES for s in tc.STRIDES for k in range(3))


@pytest.mark.parametrize("wrong", tc.WRONG)
def test_each_wrong_variant_fails_on_the_case_table(wrong):
    """the same comparison as above (bit equality with the voxel loop), with ONE mistake switched
    on in the vectorised restatement: some case of the table must tell it apart"""
    caught = 0
    if wrong == 'no_reverse':
        for sh in tc.BARRIER_VOLUMES:
            ids = tc.id_volume(sh)
            for dil, conn in tc.BARRIER_FLAGS:
                caught += not same(tc.barriers_np(ids, dil, conn, wrong=wrong),
                                   tc.barriers_loop(ids, dil, conn))
        assert caught
        return
    for shape, s, E in CASES:
        t = tc.patch(shape)
        if wrong == 'nan_negative':
            caught += tc.count_negative_np(t, wrong=wrong) != tc.count_negative_loop(t)
            continue
        nh = tc.fit_nhood(tc.NHOODS[E], shape)
        if wrong in ('sign', 'fill0', 'stride_first'):
            caught += not same(tc.nhood_np(t, nh, s, wrong=wrong), tc.nhood_loop(t, nh, s))
        if wrong in ('sign', 'ge0', 'full_extents'):
            caught += not same(tc.affinity_np(t, tc.NHOODS[E], s, wrong=wrong),
                               tc.affinity_loop(t, tc.NHOODS[E], s))
    assert caught, wrong


def test_sign_mistake_is_caught_by_each_op_on_its_own():
    nh_bad = aff_bad = 0
    for shape, s, E in CASES:
        t = tc.patch(shape)
        nh = tc.fit_nhood(tc.NHOODS[E], shape)
        nh_bad += not same(tc.nhood_np(t, nh, s, wrong='sign'), tc.nhood_loop(t, nh, s))
        aff_bad += not same(tc.affinity_np(t, tc.NHOODS[E], s, wrong='sign'),
                            tc.affinity_loop(t, tc.NHOODS[E], s))
    assert nh_bad and aff_bad


BARR = [(sh, f, ecs) for sh in tc.BARRIER_VOLUMES for f in range(len(tc.BARRIER_FLAGS))
        for ecs in (0, 1, 2)]


@pytest.mark.parametrize("sh,f,ecs", BARR)
def test_barrier_gather_equals_the_two_passes(sh, f, ecs):
    ids = tc.id_volume(sh)
    dil, conn = tc.BARRIER_FLAGS[f]
    got = tc.barriers_np(ids, dil, conn, ecs)
    want = tc.barriers_loop(ids, dil, conn, ecs)
    assert same(got, want)
    if any(conn):
        assert want.any()
    assert set(np.unique(want)) <= ({0.0, 1.0, 2.0} if ecs == 2 else {0.0, 1.0})


def test_barrier_passes_skip_volumes_with_a_single_plane():
    """an axis of length 1: a pass visits no cell at all (all three coordinates below n - 1)"""
    ids = tc.id_volume((1, 5, 6))
    z = np.zeros((1, 5, 6), np.float32)
    assert same(tc.barriers_loop(ids, (1, 1, 1), (1, 1, 1)), z)
    assert same(tc.barriers_np(ids, (1, 1, 1), (1, 1, 1)), z)


# ---- the sampler's host side ----------------------------------------------------------------------
def test_ll_masks_defaults_and_validation():
    from elektronn2_amd.data import PatchSampler
    prep = PatchSampler.prepare_ll_masks
    a = prep(None, 3, 2)
    assert a.shape == (3, 2, 2) and a.dtype == np.float32
    assert (a[:, 0] == 1).all() and (a[:, 1] == 0).all()
    a = prep([None, None], 2, 4)                       # L = n_t where every entry is None
    assert a.shape == (2, 2, 4)
    m1, m2 = [1, 0, 1, 1, 0], [0, 1, 0, 0, 0]
    a = prep([None, (m1, m2), None], 3, 2)             # L from the given entry
    assert a.shape == (3, 2, 5)
    assert a[1, 0].tolist() == m1 and a[1, 1].tolist() == m2
    assert (a[0, 0] == 1).all() and (a[2, 1] == 0).all()
    for bad in ([None], [None, None, None],                              # one entry per cube
                [(m1, m2), (m1[:4], m2[:4])],                            # one common length
                [(m1, m2[:3]), None],                                    # a pair of one length
                [(m1,), None],                                           # a pair
                [(np.ones((2, 2)), np.ones((2, 2))), None],              # 1-D
                [([], []), None]):
        with pytest.raises(ValueError):
            prep(bad, 2, 2)


def test_default_neighbourhood_table():
    from elektronn2_amd.data import image
    assert image.DEFAULT_NHOOD.dtype == np.int32
    assert image.DEFAULT_NHOOD.tolist() == [[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0],
                                            [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    assert np.array_equal(image.DEFAULT_NHOOD, tc.DEFAULT_NHOOD)


def test_host_side_refusals():
    from elektronn2_amd.data import image
    ok = image.check_nhood(np.zeros((64, 3)), (4, 4, 4))
    assert ok.shape == (64, 3) and ok.dtype == np.int32
    with pytest.raises(ValueError, match="edges"):
        image.check_nhood(np.zeros((65, 3), np.int32))
    with pytest.raises(ValueError, match="edges"):
        image.check_nhood(np.zeros((0, 3), np.int32))
    with pytest.raises(ValueError):
        image.check_nhood(np.zeros((3, 2), np.int32))
    with pytest.raises(ValueError):
        image.check_nhood([[0.5, 0, 0]])
    # |off| >= extent: refused for neighbourhood targets, fine for affinities (no extents given)
    assert image.check_nhood([[0, 5, 0]], (4, 6, 3)).tolist() == [[0, 5, 0]]
    with pytest.raises(ValueError, match="extent"):
        image.check_nhood([[0, 6, 0]], (4, 6, 3))
    with pytest.raises(ValueError, match="extent"):
        image.check_nhood([[0, 0, -3]], (4, 6, 3))
    assert image.check_nhood([[0, 9, 0]]).tolist() == [[0, 9, 0]]
    with pytest.raises(NotImplementedError):
        image.ids2barriers(np.zeros((3, 3, 3), np.float32), smoothen=True)
    assert [image.ecs_mode(v) for v in (False, True, 'new_class')] == [0, 1, 2]
    with pytest.raises(ValueError):
        image.ecs_mode('other')
    assert image.strided_extents((5, 9, 11), (2, 3, 4)) == (3, 3, 3)
