"""GPU: every form of the tiling grammar (elektronn2_amd/tiling.py, e2hip.h e2_set_tiling) through
e2_set_tiling into the launch that reads it: the string is accepted, the launch runs, e2_last_launch
names the family, the tiling and "forced", and the result meets the float64 oracle as closely as
test_ops_gpu.py / test_bf16_gpu.py ask of that kernel family (their helpers, their tolerance).

Shapes: kernels with taps on input (1, 5, 4, 9, 21), kernel (2, 3, 3), 20 output channels -> 3 x 7 x 19
(Cin no multiple of 4, 133 positions per plane: more than one position tile with a masked tail);
the pointwise forms on a 1x1x1 problem with 40 -> 70 channels.  Every string is one that
test_ops_gpu.py / test_bf16_gpu.py already force for its family, so an instance exists.  Outputs are
prefilled with NaN."""
import functools

import numpy as np
import pytest
import torch

from oracle import e2_oracle as O
from elektronn2_amd.backend import E2Error
from test_bf16_gpu import bf16_round
from test_ops_gpu import TOL, dev, relerr

pytestmark = pytest.mark.gpu

K, CI, CO, SP = (2, 3, 3), 5, 20, (4, 9, 21)
PW_CI, PW_CO, PW_SP = 40, 70, (2, 5, 23)
REFUSED = "not one this launch can run"


@functools.lru_cache(maxsize=None)
def problem(pointwise):
    """operands and float64 references, computed once and left unchanged"""
    ci, co, k, sp = (PW_CI, PW_CO, (1, 1, 1), PW_SP) if pointwise else (CI, CO, K, SP)
    rng = np.random.RandomState(31 + pointwise)
    x = rng.rand(1, ci, *sp).astype(np.float32)
    w = (rng.randn(co, ci, *k) / np.sqrt(ci * np.prod(k))).astype(np.float32)
    y = O.conv3d_fwd(x, w)
    dy = rng.randn(*y.shape).astype(np.float32)
    p = dict(x=x, w=w, dy=dy, y=y)
    if not pointwise:
        p['dw'] = O.conv3d_wgrad(dy, x, w.shape)
        p['y_bf16'] = O.conv3d_fwd(bf16_round(x), bf16_round(w))
        p['dw_bf16'] = O.conv3d_wgrad(bf16_round(dy), bf16_round(x), w.shape)
    for a in p.values():
        a.setflags(write=False)
    return p


def nan_like(ref):
    return torch.full(ref.shape, float("nan"), device="cuda")


# (string, family, the tiling e2_last_launch reports: the short pointwise form runs with KC = 32 and
# is reported in the long form, every other string as it was set)
IGEMM_FORMS = [("1,1,4,1", "igemm", None), ("3,1,4,4", "igemm", None),          # "MT,NT,CC,SK"; split-K
               ("4,5,2,16,1,1,4,2", "igemm4", None),                            # "4,MG,NT,CC,SK,WM,WN,G"
               ("1,4,1", "pw_gemm", "1,4,1,32,0"), ("1,4,2,64,0", "pw_gemm", None)]


@pytest.mark.parametrize("force,family,ran", IGEMM_FORMS, ids=[f[0] for f in IGEMM_FORMS])
def test_packed_forms_run_forced(ctx, force, family, ran):
    p = problem(family == "pw_gemm")
    y = nan_like(p['y'])
    ctx.set_tiling("igemm", force)
    try:
        ctx.conv3d_fwd(dev(p['x']), dev(p['w']), y)
        assert ctx.last_launch() == (family, ran or force, "forced")
    finally:
        ctx.set_tiling("igemm", None)
    assert relerr(y, p['y']) < TOL


def test_memory_form_runs_forced_on_the_bf16_forward(ctx):
    p = problem(False)
    y = nan_like(p['y'])
    ctx.set_tiling("igemm", "32,1,1")
    try:
        ctx.conv3d_fwd_bf16(dev(p['x']), dev(p['w']), y)
        assert ctx.last_launch() == ("conv_bf16", "32,1,1", "forced")
    finally:
        ctx.set_tiling("igemm", None)
    assert relerr(y, p['y_bf16']) < TOL              # (test_bf16_gpu.py: the oracle on bf16-rounded operands)


def test_wgrad_form_runs_forced(ctx):
    p = problem(False)
    dw = nan_like(p['dw'])
    ctx.set_tiling("wgrad", "1,1,1,64,3")
    try:
        ctx.conv3d_wgrad(dev(p['x']), dev(p['dy']), dw)
        assert ctx.last_launch() == ("wgrad_lds", "1,1,1,64,3", "forced")
    finally:
        ctx.set_tiling("wgrad", None)
    assert relerr(dw, p['dw']) < TOL


def test_memory_form_runs_forced_on_the_bf16_weight_gradient(ctx):
    p = problem(False)
    dw = nan_like(p['dw'])
    ctx.set_tiling("wgrad", "32,1,2,1,3")            # (3 position splits of 3 planes: S stays 3)
    try:
        ctx.conv3d_wgrad_bf16(dev(p['x']), dev(p['dy']), dw)
        assert ctx.last_launch() == ("wgrad_bf16", "32,1,2,1,3", "forced")
    finally:
        ctx.set_tiling("wgrad", None)
    assert relerr(dw, p['dw_bf16']) < TOL


@pytest.mark.parametrize("kind", ["igemm", "wgrad"])
def test_malformed_strings_are_refused_where_they_are_set(ctx, kind):
    """text behind a valid prefix, blanks, more than 8 integers, more than 63 characters: refused by
    e2_set_tiling itself (tests/conv_host_check.cpp holds the whole table), and the setting in
    force stays"""
    good = "1,1,4,1" if kind == "igemm" else "1,1,1,64,3"
    ctx.set_tiling(kind, good)
    try:
        for s in ("1,2,3,4,5,6,7,8,9", "4,1,2,3,", "4,1,2,x", " 4,1,2,3", "4, 1,2,3", "+4,1,2,3",
                  "7,2,32,0" + "0" * 55 + "1", "1,2,3,4,5,6", "7,2"):
            with pytest.raises(E2Error, match="e2_set_tiling"):
                ctx.set_tiling(kind, s)
        if kind == "wgrad":
            for s in ("32,2,2", "1,1,4,1"):
                with pytest.raises(E2Error, match="e2_set_tiling"):
                    ctx.set_tiling(kind, s)
        assert ctx.current_tiling(kind) == good
        ctx.set_tiling(kind, "7,2,32," + "0" * 55 + "1" if kind == "igemm" else good)      # 63 characters
    finally:
        ctx.set_tiling(kind, None)


@pytest.mark.parametrize("force", ["3,4,5,6,7", "32,1,1"])
def test_strings_no_packed_launch_can_run_are_an_error_of_the_launch(ctx, force):
    """five integers that do not start with 1, and the memory form: e2_set_tiling takes them (the
    latter belongs to e2_conv3d_*_bf16), a packed f32 launch refuses them and writes nothing"""
    p = problem(False)
    y = nan_like(p['y'])
    ctx.set_tiling("igemm", force)
    try:
        with pytest.raises(E2Error, match=REFUSED):
            ctx.conv3d_fwd(dev(p['x']), dev(p['w']), y)
    finally:
        ctx.set_tiling("igemm", None)
    assert torch.isnan(y).all()


def test_a_string_of_another_form_is_a_reported_fallback_of_the_memory_launchers(ctx):
    p = problem(False)
    y, dw = nan_like(p['y']), nan_like(p['dw'])
    n0 = ctx.tiling_fallbacks()
    ctx.set_tiling("igemm", "1,1,4,1")
    ctx.allowed_fallbacks = 1
    try:
        ctx.conv3d_fwd_bf16(dev(p['x']), dev(p['w']), y)
        assert ctx.last_launch() == ("conv_bf16", "32,2,2", "fallback")
        assert ctx.tiling_fallbacks() == n0 + 1
    finally:
        ctx.set_tiling("igemm", None)
    assert relerr(y, p['y_bf16']) < TOL
    ctx.set_tiling("wgrad", "1,1,1,64,3")
    ctx.allowed_fallbacks = 1
    try:
        ctx.conv3d_wgrad_bf16(dev(p['x']), dev(p['dy']), dw)
        fam, til, src = ctx.last_launch()
        assert (fam, src) == ("wgrad_bf16", "fallback") and til.startswith("32,2,")
        assert ctx.tiling_fallbacks() == n0 + 2
    finally:
        ctx.set_tiling("wgrad", None)
    assert relerr(dw, p['dw_bf16']) < TOL
