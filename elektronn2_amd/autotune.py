"""Empirical tiling selection for the conv kernels.

The analytic cost models inside libe2hip.so pick a valid tiling; this module
refines the choice per problem by timing a short list of candidates on the GPU
(HIP events on the context's stream) the first time a problem is seen -- the
moral equivalent of the seconds Theano spent in ``theano.function`` compile
(graphutils.py:376-387), here it is ~20 ms per layer.  Results are cached in
the process and in ``$E2HIP_TUNE_CACHE`` (default: ``.tune_cache.json`` next to this
file, git-ignored);
``elektronn2_amd/tuned.json`` ships the choices for the BASELINE workloads.

Tilings reach the library through the C ABI (``e2_set_tiling`` /
``Context.set_tiling``), per context, around each launch; a launch captured into a
hipGraph keeps whatever tiling was active at capture time.  ``force(kind, cfg)`` pins a
tiling for every problem of a kind (tests, experiments); it outranks the cache.
"""
from __future__ import annotations

import json
import math
import os

from . import tiling
from .backend import E2Error

_HERE = os.path.dirname(os.path.abspath(__file__))
_SHIPPED = os.path.join(_HERE, "tuned.json")
_cache = None
_dirty = False
IGEMM_MTS = [1, 2, 3, 4, 5, 6, 7, 8, 10, 13]
WGRAD_MTS = [1, 2, 3, 4, 5, 7]


def _cache_path():
    return os.environ.get("E2HIP_TUNE_CACHE", os.path.join(_HERE, ".tune_cache.json"))


def _load():
    global _cache
    if _cache is None:
        _cache = {}
        for path in (_SHIPPED, _cache_path()):
            try:
                with open(path) as f:
                    _cache.update(json.load(f))
            except Exception:
                pass
    return _cache


def save():
    global _dirty
    if not _dirty:
        return
    try:
        os.makedirs(os.path.dirname(_cache_path()), exist_ok=True)
        with open(_cache_path(), "w") as f:
            json.dump(_cache, f, indent=0, sort_keys=True)
        _dirty = False
    except Exception:
        pass


def enabled():
    return os.environ.get("E2HIP_AUTOTUNE", "1") != "0"


def _best_mts(mblocks, options, keep=3):
    """tile heights with the least padding, larger first on ties"""
    scored = []
    for mt in options:
        if mt > mblocks and mt != 1:
            continue
        n = -(-mblocks // mt)
        scored.append((n * mt, -mt, mt))
    scored.sort()
    return [s[2] for s in scored[:keep]]


def _near_divisors(n, target):
    """the divisors of n just below and just above target (balanced position splits)"""
    lo = [d for d in range(1, target + 1) if n % d == 0]
    hi = [d for d in range(target, min(n, 2 * target) + 1) if n % d == 0]
    return ([lo[-1]] if lo else []) + ([hi[0]] if hi else [])


BF16_MEMORY_TILES = ("32,1,1", "32,1,2", "32,2,1", "32,2,2", "32,1,4", "32,4,1")


def bf16_memory_candidates(cin):
    """"32,MB,NB": the conv kernel with bf16 operands in memory (csrc/conv_bf16.hip), a
    candidate of the bf16 mode next to the operand-rounding tilings; it pads the reduction
    channels to 16, so it is not offered for very few of them"""
    return list(BF16_MEMORY_TILES) if cin >= 16 else []


def bf16_wgrad_candidates(cin, k):
    """"32,MB,NB,R,S": the weight-gradient kernel with bf16 operands in memory
    (csrc/wgrad_bf16.hip): MB x NB blocks of 32 out channels x (32 input channels of one
    tap) per wave, NB taps of one kernel row, S position splits (0: one work-group per CU).
    R = 0: a work-group spans 128 input channels and one kernel row; R = 1: 32 input channels
    and four kernel rows (layers with few input channels)."""
    if cin < 12:
        return []
    nbs = sorted({min(k[2], n) for n in (1, 2, 3, 4)})
    forms = ([0] if cin >= 48 else []) + ([1] if cin <= 112 else [])
    return ["32,%d,%d,%d,%d" % (mb, nb, r, s) for r in forms for mb in (1, 2) for nb in nbs
            for s in (0, 8, 16)]


def igemm_candidates(cout, cin, k, out_sp, split_k=True):
    mblocks = -(-cout // 16)
    q = out_sp[1] * out_sp[2]
    cands = []
    cinp = -(-cin // 4) * 4
    fast = k[2] in (1, 3, 4, 5)
    # channel-chunk sizes: fewest barriers first, but several so that LDS limits
    # and the number of work-groups per CU can trade off
    opts = (8, 16, 24, 32, 48, 64, cinp) if fast else (4, 8, 16, 32, cinp)
    # ... plus the chunk sizes that split Cin into n EQUAL chunks (balanced split-K ranges)
    even = tuple(-(-(-(-cin // n)) // 4) * 4 for n in range(1, 9)) if fast else ()
    ccs = sorted(set(c for c in opts + even if 4 <= c <= max(cinp, 4) and c <= (64 if fast else 32)))
    for mt in _best_mts(mblocks, IGEMM_MTS, keep=4):
        nmt = -(-mblocks // mt)
        for nt in (1, 2, 4):
            if (nt == 4 and mt > 5) or (nt == 2 and mt > 10):
                continue
            base = out_sp[0] * (-(-q // (64 * nt))) * nmt
            sks = (1,) if (base >= 200 or not split_k) else (1, 2, 3, 4, 5, 6, 8)
            for cc in ccs:
                for sk in sks:
                    cands.append("%d,%d,%d,%d" % (mt, nt, cc, sk))
    return cands + igemm4_candidates(cout, cin, k, out_sp, split_k) + pointwise_candidates(cout, k, cin)


PW_MTS = (4, 5, 6, 7, 8, 10, 13, 16)


def pointwise_candidates(cout, k, cin=1 << 30):
    """"1,MT,NT": the 1x1x1 GEMM with LDS-staged weights (csrc/conv_pw.hip): all 16*MT
    channels of an M tile x 64*NT positions per work-group"""
    if tuple(k) != (1, 1, 1) or cout < 48:
        return []
    mblocks = -(-cout // 16)
    out = []
    for mt in _best_mts(mblocks, PW_MTS, keep=3):
        for nt in (1, 2):
            if mt == 16 and nt == 2:
                continue
            out.append("1,%d,%d" % (mt, nt))
            # longer pipeline chunks ("1,MT,NT,KC,0"): what fits LDS twice and the registers
            for kc in (64, 128):
                bms = 16 * mt if (16 * mt) % 32 == 16 else 16 * mt + 16
                if 2 * kc * bms * 4 <= 160 * 1024 and nt * (kc // 4) * 2 <= 64 and cin > 32:
                    out.append("1,%d,%d,%d,0" % (mt, nt, kc))
    return out


IGEMM4_INSTANCES = [(4, 2), (5, 1), (5, 2), (7, 1), (7, 2), (8, 1), (10, 1), (13, 1), (16, 1)]


def g4_pairs(mg, nt, kw):
    """input channels per pipeline step of an igemm4 instance (csrc/igemm4_core.hpp g4_pairs)"""
    na = (4 * mg + 63) // 64
    u = 1
    while u < 8 and u * kw * mg * nt < 40 and 2 * (2 * u) * kw * (na + nt) + 4 * mg * nt <= 88:
        u *= 2
    return u


def igemm4_candidates(cout, cin, k, out_sp, split_k=True, n_cu=256):
    """"4,MG,NT,CC,SK,WM,WN,G": the 4x4x1-MFMA kernel (channels padded to 4, not 16; small
    tiles per wave, WM x WN <= 12 compute waves per work-group, persistent work-groups).
    Channel coverage 4*MG*WM with the least padding, a few position widths 64*NT*WN, small
    channel chunks (they only set the LDS footprint), split-K only when the grid is small."""
    if k[2] not in (1, 3, 4, 5):
        return []
    q = out_sp[1] * out_sp[2]
    cinp = -(-cin // 4) * 4
    groups = -(-cout // 4)
    shapes = []
    for mg, nt in IGEMM4_INSTANCES:
        for wm in range(1, 13):
            bm = 4 * mg * wm
            nmt = -(-cout // bm)
            pad = nmt * bm - cout
            if pad >= 4 * mg and wm > 1:          # a whole wave of the tile would idle
                continue
            if nmt > 1 and wm < 3 and mg * wm < groups / 4.0:
                continue
            for wn in (1, 2, 3, 4, 6, 12):
                if wm * wn > 12 or (wm * wn < 6 and wm * wn != 4):
                    continue
                shapes.append((round(pad / float(cout), 3), -wm * wn, mg, nt, wm, wn, nmt))
    shapes.sort()
    best_pad = shapes[0][0] if shapes else 0
    cands = []
    for padf, _, mg, nt, wm, wn, nmt in shapes:
        if padf > best_pad + 0.06:
            break
        u = g4_pairs(mg, nt, k[2])
        step = u * 4 // math.gcd(u, 4)
        if ((step // u) * k[1]) % 2:               # an even number of pipeline steps per chunk
            step *= 2
        bn = 64 * nt * wn
        if bn > 2 * q:
            continue
        base = out_sp[0] * (-(-q // bn)) * nmt
        sks = (1,) if (base >= 160 or not split_k) else (1, 2, 4)
        ccs = sorted(set(-(-c // step) * step for c in (8, 16) if c >= 4))
        ccs = [c for c in ccs if -(-cin // c) * c <= cinp + 32][:2]
        for cc in ccs:
            for sk in sks:
                tiles = base * sk
                for g in (1, 2):
                    if g > 1 and (tiles <= n_cu or wm * wn > 6):
                        continue
                    cands.append("4,%d,%d,%d,%d,%d,%d,%d" % (mg, nt, cc, sk, wm, wn, g))
    return cands


def wgrad_candidates(cout, cin, k, out_sp, n_cu=256):
    """"MT,NT,WK,BP,PS": WK 1 = direct kernel (dy from global memory; BP 128/256),
    WK 14 = direct kernel whose four waves share one 16*NT n-tile and split the quads,
    WK 101 / 114 = the same two with the XCD-grouped block order (the work-groups that read
    the same gradient rows share one L2; needs nMT * PS % 8 == 0),
    WK 0 = LDS-staged kernel (BP 64/128), WK 4 = LDS-staged, waves split K (tiny N)."""
    mblocks = -(-cout // 16)
    T = k[0] * k[1] * k[2]
    nblocks = -(-(cin * T) // 16)
    q = out_sp[1] * out_sp[2]
    qpad = out_sp[1] * (out_sp[2] + 2 * (k[2] - 1))       # span of a padded gradient plane
    cands = []
    for mt in _best_mts(mblocks, WGRAD_MTS, keep=3):
        nmt = -(-mblocks // mt)
        variants = [(1, 1), (2, 1), (4, 1), (2, 14), (4, 14), (1, 0), (2, 0), (4, 0)]
        if nblocks <= 2:
            variants = [(1, 4), (1, 0), (1, 1), (2, 14)]
        for nt, wk in variants:
            wn = 1 if wk in (4, 14) else 4
            if nt > 1 and 16 * nt * wn > 16 * nblocks:
                continue
            nnt = -(-nblocks // (nt * wn))
            for bp in ((128, 256) if wk in (1, 14) else (64, 128)):
                tiles = out_sp[0] * (-(-(qpad if wk in (1, 14) else q) // bp))
                for fill in (1, 1.5, 2, 3, 4):
                    ps = max(1, min(tiles, int(n_cu * fill) // max(1, nmt * nnt)))
                    # ... and the nearest split counts that divide the tiles evenly
                    for q in {ps} | set(_near_divisors(tiles, ps)):
                        cands.append("%d,%d,%d,%d,%d" % (mt, nt, wk, bp, q))
                        if wk in (1, 14) and nnt >= 2 and nmt * q * nnt > 8:
                            # the same launch in the XCD-grouped block order (balanced for any
                            # group count: csrc/conv_wgrad_direct.hip)
                            cands.append("%d,%d,%d,%d,%d" % (mt, nt, wk + 100, bp, q))
    return sorted(set(cands) | set(pointwise_wgrad_candidates(cout, cin, k, out_sp, n_cu))
                  | set(position_split_wgrad_candidates(cout, cin, k, out_sp, n_cu))
                  | set(even_split_wgrad_candidates(cout, cin, k, out_sp, n_cu))
                  | set(six_product_wgrad_candidates(cout, cin, k, out_sp, n_cu)))


def six_product_form(c):
    """the "MT,NT,18,..." / "MT,NT,19,..." string of an 8 / 9 tiling -- the same kernel with every
    f32 product made of six bf16 MFMA products (csrc/conv_pw_wgrad.hip) -- else None"""
    v = c.split(",")
    if len(v) == 5 and v[2] in ("8", "9"):
        return ",".join(v[:2] + ["1" + v[2]] + v[3:])
    return None


def six_product_wgrad_candidates(cout, cin, k, out_sp, n_cu=256):
    """every 8 / 9 candidate of the three generators below in its six-product form (a list of its
    own: theirs hold one form each, which tests/test_host_logic.py pins)"""
    out = []
    for gen in (pointwise_wgrad_candidates, position_split_wgrad_candidates, even_split_wgrad_candidates):
        out += [six_product_form(c) for c in gen(cout, cin, k, out_sp, n_cu)]
    return sorted(set(c for c in out if c))


WGRAD_KS_TILES = [(13, 2), (10, 2), (8, 2), (8, 4), (7, 2), (7, 4), (6, 4), (5, 4), (4, 4), (3, 4), (2, 4)]


def position_split_wgrad_candidates(cout, cin, k, out_sp, n_cu=256):
    """"MT,NT,9,0,S": the weight gradient of a kernel WITH taps as the K-contiguous GEMM of
    csrc/conv_pw_wgrad.hip -- one 16 MT x 16 NT tile of dW (cout x cin * taps) per work-group, its
    four waves split the positions of the gradient planes; needs (kh - 1) input rows >= 31 zeros
    behind a plane of the padded gradient (the library refuses otherwise: the tuner skips it)"""
    T = k[0] * k[1] * k[2]
    if T == 1 or cout < 24:
        return []
    pitch = out_sp[2] + k[2] - 1
    if (k[1] - 1) * pitch + k[2] - 1 < 31:
        return []
    units = out_sp[0] * (-(-((out_sp[1] - 1) * pitch + out_sp[2]) // 32))
    scored = []
    for mt, nt in WGRAD_KS_TILES:
        nm, nn = -(-cout // (16 * mt)), -(-(cin * T) // (16 * nt))
        eff = (cout * cin * T) / float(nm * 16 * mt * nn * 16 * nt)
        scored.append((-eff, -mt * nt, mt, nt, nm * nn))
    scored.sort()
    out = []
    for _, _, mt, nt, tiles in scored[:4]:
        for fill in (0.5, 1, 2):
            s = max(1, min(-(-units // 4), int(n_cu * fill) // tiles))
            out.append("%d,%d,9,0,%d" % (mt, nt, s))
    return sorted(set(out))


def even_split_wgrad_candidates(cout, cin, k, out_sp, n_cu=256):
    """"MT,NT,9,B,G" / "MT,NT,8,B,G", B >= 1: the tiles of the two position-split forms with EVEN
    position ranges (csrc/wgrad_even.hpp) -- G work-groups share the tiles x units pairs, so the
    grid fills the chip whatever the tile count: G = CUs x r for r = 1, 2 where a work-group's LDS
    (its four partial tiles, 4 x 16 MT x (16 NT + 4) floats of 160 KB per CU) allows two per CU,
    for the tiles that waste the fewest MFMAs (the registers allow two work-groups per CU at
    most as well, but for the 2 x 4 and 3 x 4 tiles).  B = 1 orders the pairs tile by tile; B > 1
    band by band of positions, with as many bands as the position-split form would take splits
    to reach G work-groups (the tiles of one band then share the gradient rows in L2)"""
    T = k[0] * k[1] * k[2]
    if T == 1:
        if cout < 32 or cin < 32 or out_sp[0] * out_sp[1] * out_sp[2] < 32:
            return []
        tiles, form = PW_WGRAD_KS_TILES, 8
        units = out_sp[0] * out_sp[1] * out_sp[2] // 32     # (of ONE sample; the library refuses B > units)
    else:
        if not position_split_wgrad_candidates(cout, cin, k, out_sp, n_cu):
            return []
        tiles, form = WGRAD_KS_TILES, 9
        pitch = out_sp[2] + k[2] - 1
        units = out_sp[0] * (-(-((out_sp[1] - 1) * pitch + out_sp[2]) // 32))
    scored = []
    for mt, nt in tiles:
        nm, nn = -(-cout // (16 * mt)), -(-(cin * T) // (16 * nt))
        eff = (cout * cin * T) / float(nm * 16 * mt * nn * 16 * nt)
        scored.append((-eff, -mt * nt, mt, nt, nm * nn))
    scored.sort()
    out = []
    for _, _, mt, nt, ntiles in scored[:3]:
        lds = 4 * 16 * mt * (16 * nt + 4) * 4
        for r in range(1, min(2, (160 * 1024) // lds) + 1):
            g = n_cu * r
            for b in sorted({1, max(1, min(-(-units // 4), g // ntiles))}):
                out.append("%d,%d,%d,%d,%d" % (mt, nt, form, b, g))
    return sorted(set(out))


PW_WGRAD_KS_TILES = [(13, 2), (10, 2), (7, 2), (7, 4), (4, 4)]
PW_WGRAD_TILES = [(2, 2), (4, 2), (2, 4), (4, 4), (4, 3), (3, 4), (7, 2), (2, 7), (7, 4), (4, 7)]


def pointwise_wgrad_candidates(cout, cin, k, out_sp, n_cu=256):
    """"MT,NT,7,0,S": the 1x1x1 (and UpConv) weight gradient as a GEMM with K-contiguous
    operands (csrc/conv_pw_wgrad.hip): 2 x 2 waves of MT x NT blocks of 16 x 16 per
    work-group, S splits of the positions"""
    if tuple(k) != (1, 1, 1) or cout < 32 or cin < 32:
        return []
    steps = -(-(out_sp[0] * out_sp[1] * out_sp[2]) // 16)
    scored = []
    for mt, nt in PW_WGRAD_TILES:
        nm, nn = -(-cout // (32 * mt)), -(-cin // (32 * nt))
        eff = (cout * cin) / float(nm * 32 * mt * nn * 32 * nt)
        scored.append((-eff, mt * nt, mt, nt, nm * nn))
    scored.sort()
    out = []
    for _, _, mt, nt, tiles in scored[:5]:
        for fill in (0.5, 1, 2, 4):
            s = max(1, min(steps, int(n_cu * fill) // tiles))
            out.append("%d,%d,7,0,%d" % (mt, nt, s))
    # "MT,NT,8,0,S": ONE 16 MT x 16 NT tile per work-group, its four waves split the positions
    units = max(1, (out_sp[0] * out_sp[1] * out_sp[2]) // 32)
    scored = []
    for mt, nt in PW_WGRAD_KS_TILES:
        nm, nn = -(-cout // (16 * mt)), -(-cin // (16 * nt))
        eff = (cout * cin) / float(nm * 16 * mt * nn * 16 * nt)
        scored.append((-eff, -mt * nt, mt, nt, nm * nn))
    scored.sort()
    for _, _, mt, nt, tiles in scored[:3]:
        for fill in (0.5, 0.75, 1, 2):
            s = max(1, min(-(-units // 4), int(n_cu * fill) // tiles))
            out.append("%d,%d,8,0,%d" % (mt, nt, s))
    return sorted(set(out))


_forced = {}
last_ranking = {}     # key -> [(seconds, tiling), ...] of the most recent tuning of that problem


def force(kind, cfg):
    """pin ('igemm' | 'wgrad') launches to one tiling string; None lifts the pin"""
    if cfg:
        _forced[kind] = cfg
    else:
        _forced.pop(kind, None)


def _bf16(ctx):
    return getattr(ctx, "mfma_dtype", "f32") == "bf16"


def known(ctx, kind, sig):
    """the tiling tuned_call would run (kind, sig) with WITHOUT tuning: the pinned one, the
    table's entry, or None when the problem has not been tuned yet"""
    if kind in _forced:
        return _forced[kind]
    return _load().get(tiling.key(kind, sig, _bf16(ctx)))


def side_flag(ctx, sig):
    """f32 mode: does the weight gradient of problem ``sig`` (the 'wgrad' signature) run on the
    plan's side stream?  A measured, per-problem entry of the table like the tilings
    ("side|<sig>": "1"; tools/tune_side.py writes them, DESIGN finding 56)"""
    if _bf16(ctx):
        return False
    return _load().get(tiling.side_key(sig)) == "1"


def set_side_flag(sig, on):
    global _dirty
    key = tiling.side_key(sig)
    c = _load()
    if on:
        c[key] = "1"
    else:
        c.pop(key, None)
    _dirty = True


def _time(ctx, fn, iters=4):
    fn()
    e0, e1 = ctx.event(), ctx.event()
    ctx.record(e0)
    for _ in range(iters):
        fn()
    ctx.record(e1)
    return ctx.elapsed_ms(e0, e1) / iters


# Launches whose tiling string (pinned or from the table) was NOT the one the library ran:
# (key, tiling asked for, Context.last_launch()).  Only the weight-gradient forms 7 / 8 / 9 can
# fall back (e2hip.h, e2_set_tiling); the native-size tests assert this list stays empty for the
# shipped table.  ``launch_log``: set to a list to record (key, tiling, last_launch) of EVERY call.
fallbacks = []
launch_log = None


def _note(ctx, key, tiling):
    if not hasattr(ctx, "last_launch"):
        return
    ll = ctx.last_launch()
    if launch_log is not None:
        launch_log.append((key, tiling, ll))
    if tiling and ll is not None and ll[2] == "fallback":
        fallbacks.append((key, tiling, ll))


def tuned_call(ctx, kind, sig, cands, fn, allow_tune=True, fn_tune=None, fn_once=None):
    """Run ``fn`` with the best known tiling for (kind, sig); tune on first sight.
    kind: 'igemm' | 'wgrad'.  ``fn_tune`` (default ``fn``) is the IDEMPOTENT form of
    the launch used for the timing runs (e.g. wgrad that overwrites instead of
    accumulating); when tuning ran, the result is produced by one final
    ``fn_tune`` call instead of ``fn`` -- or by ``fn_once`` when given (a launch whose side
    effect must happen exactly once and that leaves the timed outputs as ``fn_tune`` does).
    Returns the tiling string used."""
    global _dirty
    ft = fn_tune if fn_tune is not None else fn
    key = tiling.key(kind, sig, _bf16(ctx))
    if kind in _forced:
        ctx.set_tiling(kind, _forced[kind])
        try:
            fn()
        finally:
            ctx.set_tiling(kind, None)
        _note(ctx, key, _forced[kind])
        return _forced[kind]
    cache = _load()
    best = cache.get(key)
    tuned_now = False
    if best is None and enabled() and allow_tune:
        tuned_now = True
        results = []
        try:
            try:
                results.append((_time(ctx, ft), ""))
            except E2Error:
                pass
            for c in cands:
                ctx.set_tiling(kind, c)
                try:
                    t = _time(ctx, ft)
                except E2Error:
                    continue
                ll = ctx.last_launch() if hasattr(ctx, "last_launch") else None
                if ll is not None and ll[2] == "fallback":
                    continue          # (another kernel ran under this name: not a measurement of c)
                results.append((t, c))
        finally:
            ctx.set_tiling(kind, None)
        if results and len(results) > 2:
            # second pass: the first one ranks ~100 candidates on 4 launches apiece, and its
            # +-3 % noise is more than what separates the leaders -- the best few again,
            # interleaved, on 3 x 12 launches, ranked by their fastest round
            results.sort()
            top = [c for _, c in results[:6]]
            fine = {c: [] for c in top}
            try:
                for _ in range(3):
                    for c in top:
                        ctx.set_tiling(kind, c or None)
                        try:
                            fine[c].append(_time(ctx, ft, iters=12))
                        except E2Error:
                            fine[c].append(float("inf"))
            finally:
                ctx.set_tiling(kind, None)
            results = sorted((min(v), c) for c, v in fine.items()) + results[6:]
        if results:
            results.sort()
            last_ranking[key] = list(results[:10])
            best = results[0][1]
            if kind == "wgrad":
                # at (nearly) equal time prefer the XCD-grouped block order (WK >= 100): the
                # gradient rows are then fetched once per L2 instead of once per XCD
                for t, c in results:
                    if t > 1.015 * results[0][0]:
                        break
                    if c and tiling.parse(kind, c).xcd_grouped:
                        best = c
                        break
            cache[key] = best
            _dirty = True
    final = (fn_once if fn_once is not None else ft) if tuned_now else fn
    if best:
        ctx.set_tiling(kind, best)
        try:
            final()
        finally:
            ctx.set_tiling(kind, None)
    else:
        final()
    _note(ctx, key, best)
    return best
