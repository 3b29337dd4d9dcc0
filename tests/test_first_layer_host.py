"""The exact-arithmetic first-layer cases hold what test_first_layer_gpu.py relies on (CPU only).

  * The float32 restatement of the kernels' promises (first_layer_cases.first_layer_f32) equals
    the float64 oracle EXACTLY on the whole case table, with the taps walked in either order: the
    inputs' binary grid makes float32 sums order-independent, so equality is the right demand of
    the GPU kernels whatever their order of summation.
  * Per case of shape B or C: the partial sums of dW / dbias stay below 2^24 grid units (the
    condition of that argument), and two-way ties, four-way ties, pre-activations of exactly
    zero, negative and positive ones each make up at least 1 % of the (channel, pooled position)
    pairs -- conditions on the inputs, taken from the reference alone.  (A window of one element
    cannot tie: the tie shares are asked of the pooled geometries.)
  * Every wrong variant of a promise (the switches of first_layer_f32) FAILS check_exact, the
    comparison the GPU test uses, on a named case of every geometry it applies to.  The mutants
    exist in NumPy only; no kernel is altered.
"""
import numpy as np
import pytest

import first_layer_cases as FL

POOLED = ("k4p2", "k6p2")
ALL = tuple(FL.GEOMETRIES)
MIN_SHARE = 0.01


def restate(ref, **kw):
    return FL.first_layer_f32(ref["x"], ref["w"], ref["b"], ref["dout"], ref["geometry"], ref["act"], **kw)


def representable(ref):
    for name in ("out", "dw", "db"):
        a = ref[name]
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a), name
    assert np.array_equal(ref["dw"] * 16, np.round(ref["dw"] * 16))           # the 2^-4 grid
    assert np.array_equal(ref["out"] * 128, np.round(ref["out"] * 128))       # the 2^-7 grid


def conditions(ref, what):
    assert ref["exact_bound"] < 2 ** 24, (what, ref["exact_bound"])
    share = ref["share"]
    wanted = ("pre0", "neg", "pos") + (("tie2", "tie4") if ref["geometry"] in POOLED else ())
    print(what, "bound %.3g" % ref["exact_bound"], {k: round(float(v), 4) for k, v in share.items()})
    for name in wanted:
        assert share[name] >= MIN_SHARE, (what, name, share)


def test_table_is_the_cross_product():
    assert len(FL.TABLE) == 162 and len(set(FL.TABLE)) == 162
    assert {FL.form(c) for c in FL.COUTS} == {"mfma5", "mfma8", "valu"}
    assert [c % 4 for c in FL.COUTS] == [1, 3, 1, 0, 1, 1, 0, 1, 0]


@pytest.mark.parametrize("geometry", ALL)
def test_restatement_equals_the_oracle_in_either_tap_order(geometry):
    for case in FL.TABLE:
        if case[0] != geometry:
            continue
        ref = FL.table_case(case)
        representable(ref)
        fwd = restate(ref, prefill=FL.PREFILL)
        FL.check_exact(*fwd, ref, FL.PREFILL)
        back = restate(ref, prefill=FL.PREFILL, reverse_taps=True)
        for a, b in zip(fwd, back):
            assert np.array_equal(a, b), FL.case_id(case)
        if case[2] != "A":
            conditions(ref, FL.case_id(case))


@pytest.mark.parametrize("name", sorted(FL.LONG))
def test_long_cases_meet_the_conditions(name):
    """the cases with more tiles than the persistent grids: exactly representable, below the
    exactness bound, ties and the kink present; the restatement agrees with the oracle"""
    ref = FL.long_case(name)
    representable(ref)
    conditions(ref, name)
    FL.check_exact(*restate(ref), ref, (0.0, 0.0))


# switch -> (geometries it applies to, the case of each geometry that must show it: cout, shape, act)
MUTANTS = {
    "first_max_only":    (POOLED, (17, "B", "relu")),
    "slope0_is_0":       (ALL, (17, "B", "relu")),
    "slope0_is_1":       (ALL, (17, "B", "relu")),
    "unflipped":         (ALL, (17, "B", "lin")),
    "dbias_per_conv":    (POOLED, (17, "B", "lin")),
    "act_ignored_bwd":   (ALL, (17, "B", "relu")),
    "drop_last_channel": (ALL, (29, "C", "relu")),
    "no_accumulate":     (ALL, (33, "A", "lin")),
}


def test_every_switch_has_a_mutant():
    assert set(MUTANTS) == set(FL.SWITCHES)


@pytest.mark.parametrize("switch", sorted(MUTANTS))
def test_mutant_fails_check_exact(switch):
    geoms, (cout, shape, act) = MUTANTS[switch]
    for g in geoms:
        case = (g, cout, shape, act)
        assert case in FL.TABLE
        ref = FL.table_case(case)
        FL.check_exact(*restate(ref, prefill=FL.PREFILL), ref, FL.PREFILL)      # the control passes
        with pytest.raises(AssertionError, match="differ"):
            FL.check_exact(*restate(ref, prefill=FL.PREFILL, **{switch: True}), ref, FL.PREFILL)
        print(switch, "caught on", FL.case_id(case))


def test_mutants_that_touch_the_gradient_alone_leave_the_output():
    """... so it is the dW / dbias comparison that catches them"""
    ref = FL.table_case(("k4p2", 17, "B", "relu"))
    for switch in ("first_max_only", "slope0_is_0", "slope0_is_1", "dbias_per_conv", "act_ignored_bwd",
                   "no_accumulate"):
        out, dw, db = restate(ref, prefill=FL.PREFILL, **{switch: True})
        FL.check_exact(out, None, None, ref, FL.PREFILL)
        with pytest.raises(AssertionError, match="differ"):
            FL.check_exact(None, dw, db, ref, FL.PREFILL)


def test_check_exact_sees_nan_and_counts_launches():
    ref = FL.table_case(("k3p1", 3, "A", "relu"))
    out, dw, db = restate(ref)
    FL.check_exact(out, dw, db, ref, (0.0, 0.0))
    FL.check_exact(None, 2 * dw + 3, 2 * db - 5, ref, FL.PREFILL, launches=2)
    FL.check_exact(-out * 0 + out, None, None, ref, None)                      # -0.0 equals +0.0
    bad = out.copy()
    bad.flat[0] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        FL.check_exact(bad, None, None, ref, None)
    with pytest.raises(AssertionError):
        FL.check_exact(out[:, :, :, :, :0], None, None, ref, None)


def test_workspace_formula_matches_the_library():
    """ws_floats (what the GPU test cuts its watched workspace to) is e2_conv1_bwd_workspace_bytes"""
    from elektronn2_amd import backend
    for g, cout, shape, _ in FL.TABLE[::2]:
        Ho, Wo = FL.pooled_hw(g, shape)
        dims = (FL.N_SMALL, cout, FL.D_SMALL, Ho, Wo)
        assert backend.Context.conv1_bwd_ws_bytes(dims, FL.GEOMETRIES[g][0]) == 4 * FL.ws_floats(g, cout, FL.N_SMALL, FL.D_SMALL, Ho, Wo)
