"""Exact-arithmetic cases of the fused first layer (helpers of test_first_layer_host.py and
test_first_layer_gpu.py; no test module).

csrc/conv_first.hip and csrc/conv_first_mfma.hip: conv (one input channel, kd = 1) -> max-pool
(1,py,px) or none -> + bias -> relu / lin, and the gradient wrt w and b with the conv values
recomputed.  With ONE input channel the whole layer is exact in float32 when the inputs lie on a
binary grid:

    x in {0..7}/8,  w in {-16..16}/16,  bias in {-8..8}/16,  dout in the integers {-2..2}.

Every product, every partial sum of the conv (<= 36 taps), every pooled value, every g * x term
and every partial sum of dW / dbias is then a multiple of 2^-7 (forward) or 2^-4 (backward) and
stays below 2^24 such units (``exact_bound``, asserted per case from the reference): float32
arithmetic in ANY order, with or without fma, on the vector ALUs or the matrix cores, gives the
float64 oracle's numbers.  So the comparison is equality (by value: relu may store -0.0), ties of
the pooling window are real ties on the GPU and in the oracle alike, and a pre-activation of
exactly zero happens.

Planted into x so that the tie rule and the kink of relu are hit often:
  * top half of the rows x left third of the columns = 0: every conv value is 0, all window
    elements tie and the pre-activation is the bias -- 0 on every third channel (bias[::3] = 0);
  * bottom half x right third = 0.5: all window elements tie at 0.5 * sum(w);
  * bottom half x left third constant along each row (a random grid value per row): the two
    columns of a pooling window tie, its two rows do not -- the two-way ties that channel counts
    of 1 and 3 would not produce often enough by chance.
For Cout <= 3 the taps of a channel are drawn as pairs (v, -v): sum(w) = 0, so a single channel has
negative and positive pre-activations alike (with free taps one draw in three has one sign only).
"""
import functools

import numpy as np

from oracle import e2_oracle as O

F32, F64 = np.float32, np.float64

#: name -> (kernel, pool): the three variants of first_supported() in csrc/conv_first.hip
GEOMETRIES = {
    "k4p2": ((1, 4, 4), (1, 2, 2)),      # T = 16: four-position MFMA form
    "k6p2": ((1, 6, 6), (1, 2, 2)),      # T = 36: broadcast form
    "k3p1": ((1, 3, 3), (1, 1, 1)),      # T = 9:  four-position form, tap lanes unused
}
#: MG = 5 with 1 / 3 / 1 / 0 padding channels * MG = 8 likewise * the VALU fallback, odd and even
COUTS = (1, 3, 17, 20, 21, 29, 32, 33, 40)
ACTS = ("relu", "lin")
#: pooled (Ho, Wo) per shape name, (pooled geometries, no pooling)
SHAPES = {
    "A": ((1, 1), (1, 1)),               # one valid lane
    "B": ((5, 33), (5, 65)),             # MFMA tiles 2 x 2 with remainders, VALU 1 x 2 (1 x 3)
    "C": ((9, 32), (9, 64)),             # MFMA 3 x 1 full columns, VALU 2 x 1
}
N_SMALL, D_SMALL = 2, 3                  # z = r % D, n = r / D are both exercised
PREFILL = (3.0, -5.0)                    # dW / dbias before the launch (grid values)


def pooled_hw(geometry, shape):
    return SHAPES[shape][1 if GEOMETRIES[geometry][1] == (1, 1, 1) else 0]


def form(cout):
    """the kernel family a channel count runs (e2i_firstm_mg): 'mfma5', 'mfma8' or 'valu'"""
    return "mfma5" if cout <= 20 else ("mfma8" if cout <= 32 else "valu")


def case_id(c):
    return "%s-c%d-%s-%s" % c


#: (geometry, cout, shape, act): 3 * 9 * 3 * 2 = 162 cases at N = 2, D = 3
TABLE = tuple((g, c, s, a) for g in GEOMETRIES for c in COUTS for s in SHAPES for a in ACTS)

#: more tiles than the persistent grids (min(3 * CUs, 1024) MFMA, 8 * CUs VALU forward):
#: name -> (geometry, cout, act, N, D, pooled (Ho, Wo))
LONG = {
    "k4p2-c20": ("k4p2", 20, "relu", 3, 100, (5, 33)),
    "k6p2-c12": ("k6p2", 12, "relu", 3, 100, (5, 33)),
    "k3p1-c32": ("k3p1", 32, "lin", 3, 100, (5, 65)),
    "k4p2-c33-valu": ("k4p2", 33, "relu", 4, 130, (9, 33)),
}


def seed_of(*key):
    """a fixed function of the case"""
    return sum((i + 1) * sum(map(ord, str(k))) for i, k in enumerate(key)) % (2 ** 31)


def tiles(geometry, cout, N, D, Ho, Wo):
    """(tiles, persistent grid as a function of the CU count or None) of the forward launch"""
    px = GEOMETRIES[geometry][1][2]
    if form(cout) == "valu":
        return N * D * -(-Ho // 8) * -(-Wo // 32), lambda cus: 8 * cus
    return N * D * -(-Ho // 4) * -(-Wo * px // 64), lambda cus: min(3 * cus, 1024)


def ws_floats(geometry, cout, N, D, Ho, Wo):
    """what e2_conv1_bwd_workspace_bytes promises, in floats: the larger of the VALU form's
    part[tile][cout][T + 1] and the MFMA form's one slot per work-group (<= 1024)"""
    k = GEOMETRIES[geometry][0]
    T = k[1] * k[2]
    valu = N * D * -(-Ho // 8) * -(-Wo // 32) * cout * (T + 1)
    mfma = min(N * D * -(-Ho // 4) * -(-Wo * 2 // 64), 1024) * cout * (T + 1)
    return max(valu, mfma)


def _inputs(geometry, cout, N, D, Ho, Wo, seed):
    k, pool = GEOMETRIES[geometry]
    H, W = Ho * pool[1] + k[1] - 1, Wo * pool[2] + k[2] - 1
    T = k[1] * k[2]
    rng = np.random.RandomState(seed)
    x = rng.randint(0, 8, (N, 1, D, H, W)).astype(F64) / 8
    rowv = rng.randint(0, 8, (N, 1, D, H, 1)).astype(F64) / 8
    x[..., H - H // 2:, :W // 3] = rowv[..., H - H // 2:, :]
    x[..., :H // 2, :W // 3] = 0.0
    x[..., H - H // 2:, W - W // 3:] = 0.5
    if cout <= 3:
        half = rng.randint(-16, 17, (cout, T // 2)).astype(F64) / 16
        w = np.concatenate([half, -half, np.zeros((cout, T % 2))], axis=1)
        for c in range(cout):
            w[c] = w[c, rng.permutation(T)]
        w = w.reshape((cout, 1) + k)
    else:
        w = rng.randint(-16, 17, (cout, 1) + k).astype(F64) / 16
    b = rng.randint(-8, 9, cout).astype(F64) / 16
    b[::3] = 0.0
    dout = rng.randint(-2, 3, (N, cout, D, Ho, Wo)).astype(F64)
    return tuple(a.astype(F32) for a in (x, w, b, dout))


@functools.lru_cache(maxsize=16)
def make_case(geometry, cout, N, D, Ho, Wo, act, seed):
    """grid inputs (float32), the float64 reference of oracle.e2_oracle.conv_node_fwd / _bwd and
    the counts the conditions on the inputs are stated in; every array read-only (shared)"""
    k, pool = GEOMETRIES[geometry]
    x, w, b, dout = _inputs(geometry, cout, N, D, Ho, Wo, seed)
    out, (c, p) = O.conv_node_fwd(x, w, b, pool, act)
    _, dw, db = O.conv_node_bwd(dout, x, w, b, (c, p), pool, act, need_dx=False)
    # the oracle's gradient of the conv output (the two steps conv_node_bwd takes to it)
    dc = O.maxpool3d_bwd(O.bias_act_bwd(dout, p, b, act)[0], c, pool)
    pre = p + b.astype(F64)[None, :, None, None, None]
    ntied = (O._windows(c, pool) == p[:, :, :, None, :, None, :, None]).sum(axis=(3, 5, 7))
    pairs = float(pre.size)
    ref = dict(geometry=geometry, k=k, pool=pool, act=act, cout=cout, x=x, w=w, b=b, dout=dout,
               out=out, dw=dw, db=db,
               share=dict(tie2=(ntied == 2).sum() / pairs, tie4=(ntied == 4).sum() / pairs,
                          pre0=(pre == 0).sum() / pairs, neg=(pre < 0).sum() / pairs,
                          pos=(pre > 0).sum() / pairs),
               # partial sums of dW / dbias in units of 2^-4: must stay below 2^24
               exact_bound=float(np.abs(dc).sum(axis=(0, 2, 3, 4)).max() * np.abs(x).max() * 16))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def table_case(case):
    g, cout, shape, act = case
    Ho, Wo = pooled_hw(g, shape)
    return make_case(g, cout, N_SMALL, D_SMALL, Ho, Wo, act, seed_of(g, cout, shape))


def long_case(name, D=None):
    g, cout, act, N, D0, (Ho, Wo) = LONG[name]
    return make_case(g, cout, N, D or D0, Ho, Wo, act, seed_of(name))


def _equal(got, want, what):
    got = np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    got = got.astype(F64)
    nan = np.isnan(got)
    assert not nan.any(), "%s: %d NaN (never written, or made from memory nobody wrote); first at %s" % (
        what, nan.sum(), np.argwhere(nan)[0].tolist())
    bad = got != want                          # by value: -0.0 == +0.0
    if bad.any():
        at = np.argwhere(bad)
        raise AssertionError("%s: %d of %d values differ; first at %s: got %r, reference %r; largest "
                             "difference %g" % (what, bad.sum(), bad.size, at[0].tolist(),
                                                got[tuple(at[0])], want[tuple(at[0])],
                                                np.abs(got - want).max()))


def check_exact(got_out, got_dw, got_db, ref, prefill, launches=1):
    """THE comparison of the GPU test and of the host mutants: the output equals the reference,
    dW and dbias equal prefill + launches * reference -- by value, no tolerance.  ``prefill``:
    (value dW held, value dbias held) before the first launch; an argument that is None is not
    compared."""
    if got_out is not None:
        _equal(got_out, ref["out"], "out")
    if got_dw is not None:
        _equal(got_dw, prefill[0] + launches * ref["dw"], "dW")
    if got_db is not None:
        _equal(got_db, prefill[1] + launches * ref["db"], "dbias")


#: the switches of first_layer_f32 -> what the kernels promise instead
SWITCHES = {
    "first_max_only": "every element equal to the window maximum receives the gradient",
    "slope0_is_0": "relu'(0) = 0.5",
    "slope0_is_1": "relu'(0) = 0.5",
    "unflipped": "true convolution: tap t multiplies w[T - 1 - t]",
    "dbias_per_conv": "dbias sums the pooled gradient once per pooled position",
    "act_ignored_bwd": "the gradient passes through the activation's slope",
    "drop_last_channel": "all Cout channels (ch < Cout, not ch < Cout - 1)",
    "no_accumulate": "dW is accumulated onto what the buffer held",
}


def first_layer_f32(x, w, b, dout, geometry, act, prefill=(0.0, 0.0), reverse_taps=False, **switches):
    """Plain NumPy FLOAT32 restatement of what the kernels promise (out, dW, dbias): flipped taps,
    max over the window, bias after the max, relu with slope 0.5 at 0, the gradient to every tied
    maximum, dbias once per pooled position, dW / dbias accumulated onto ``prefill``.  Each name
    of SWITCHES turns one promise into its wrong variant; ``reverse_taps`` walks the taps in the
    opposite order (no promise: the sums are exact in any order)."""
    unknown = set(switches) - set(SWITCHES)
    assert not unknown, unknown
    sw = lambda name: bool(switches.get(name))
    k, pool = GEOMETRIES[geometry]
    KH, KW, PY, PX = k[1], k[2], pool[1], pool[2]
    T = KH * KW
    x, w, b, dout = (np.asarray(a, F32) for a in (x, w, b, dout))
    N, _, D, H, W = x.shape
    cout = w.shape[0]
    Hc, Wc = H - KH + 1, W - KW + 1
    Ho, Wo = Hc // PY, Wc // PX
    wt = w.reshape(cout, T).copy()
    bb, g = b.copy(), dout.copy()
    if sw("drop_last_channel"):                  # the last channel is loaded as a padding channel
        wt[-1], bb[-1], g[:, -1] = 0, 0, 0
    taps = list(range(T))[::-1] if reverse_taps else list(range(T))
    wtap = (lambda t: wt[:, t]) if sw("unflipped") else (lambda t: wt[:, T - 1 - t])

    def xs(t):
        ty, tx = divmod(t, KW)
        return x[:, :, :, ty:ty + Hc, tx:tx + Wc]                     # (N, 1, D, Hc, Wc)

    c = np.zeros((N, cout, D, Hc, Wc), F32)
    for t in taps:
        c += wtap(t)[None, :, None, None, None] * xs(t)
    assert c.dtype == F32
    cw = c.reshape(N, cout, D, Ho, PY, Wo, PX)
    m = cw.max(axis=(4, 6))
    pre = m + bb[None, :, None, None, None]
    out = np.maximum(pre, F32(0)) if act == "relu" else pre
    if act == "relu" and not sw("act_ignored_bwd"):
        at0 = F32(0.0 if sw("slope0_is_0") else (1.0 if sw("slope0_is_1") else 0.5))
        g = g * np.where(pre > 0, F32(1), np.where(pre == 0, at0, F32(0)))
    tied = cw == m[:, :, :, :, None, :, None]
    if sw("first_max_only"):                     # the first maximum in window order (a, b) alone
        flat = tied.transpose(0, 1, 2, 3, 5, 4, 6).reshape(N, cout, D, Ho, Wo, PY * PX)
        first = np.zeros_like(flat)
        np.put_along_axis(first, flat.argmax(axis=-1)[..., None], True, axis=-1)
        tied = first.reshape(N, cout, D, Ho, Wo, PY, PX).transpose(0, 1, 2, 3, 5, 4, 6)
    dc = (tied * g[:, :, :, :, None, :, None]).astype(F32).reshape(N, cout, D, Hc, Wc)
    dw = np.zeros((cout, T), F32)
    for t in taps:
        col = (dc * xs(t)).sum(axis=(0, 2, 3, 4), dtype=F32)
        if sw("unflipped"):
            dw[:, t] = col
        else:
            dw[:, T - 1 - t] = col
    db = (dc if sw("dbias_per_conv") else g).sum(axis=(0, 2, 3, 4), dtype=F32)
    dw = dw.reshape(w.shape) + (F32(0) if sw("no_accumulate") else F32(prefill[0]))
    db = db + F32(prefill[1])
    assert out.dtype == F32 and dw.dtype == F32 and db.dtype == F32
    return out, dw, db
