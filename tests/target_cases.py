"""Cases and host restatements for the target ops of csrc/targets.hip (tests/test_targets_host.py,
tests/test_targets_gpu.py).

Definitions (t: full-resolution target patches (n, C, D, H, W); s = (sz, sx, sy) >= 1;
ts[n,c,z,x,y] = t[n,c,z sz,x sx,y sy], extents ceil(D/sz) ...; off_e = nhood[e]):

  stride    dst = ts, NaN -> -666
  nhood     dst[:, e] (e < E) = t[n, 0, p s - off_e] inside (D, H, W), else -1; dst[:, E:] = ts[:, 1:];
            NaN -> -666
  affinity  dst[n, e, p] = 1 iff p + off_e inside the STRIDED extents and a = rint(ts[n,0,p]),
            b = rint(ts[n,0,p+off_e]) have a == b, a > 0, b > 0
  count     #{t < 0} (NaN is not negative)
  barriers  the union of the reference's forward pass and the same pass over the fully reversed
            volume (a pass visits only cells whose three coordinates are all below n - 1), then the
            ECS mode

Every op has a vectorised NumPy restatement (``*_np``) and a plain voxel loop (``*_loop``) written
from the definition alone; the vectorised ones take a ``wrong`` keyword that switches ONE deliberate
mistake on, so that the tests can show the case table tells each of them from the truth."""
import numpy as np

PATCHES = [(2, 2, 5, 9, 11), (1, 1, 4, 6, 1)]
STRIDES = [(1, 1, 1), (1, 2, 3), (2, 3, 4)]

# E = 1, 3, 7: negative displacements, displacements of 2, and (0, 5, 0): longer than the strided
# x extent of (.., 9, ..) under strides 2 and 3 (5 and 3) -- for (.., 6, ..) it is shorter than the
# full-resolution extent only
NHOODS = {
    1: np.array([[0, 0, -1]], np.int32),
    3: np.array([[-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.int32),
    7: np.array([[0, 0, 0], [1, 0, 0], [-2, 0, 0], [0, 5, 0], [0, -1, 2], [1, -2, 0], [0, 0, -1]],
                np.int32),
}
DEFAULT_NHOOD = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0],
                          [0, 0, 1], [0, 0, -1]], np.int32)

WRONG = ['sign', 'fill0', 'stride_first', 'ge0', 'full_extents', 'nan_negative', 'no_reverse']


def fit_nhood(nhood, shape):
    """the rows of ``nhood`` whose displacements are all shorter than the full-resolution extents
    (the nhood-target op refuses the others); y displacements go to zero on a single-element row"""
    nh = np.array(nhood, np.int32)
    if shape[4] == 1:
        nh[:, 2] = 0
    keep = [e for e in range(len(nh)) if all(abs(nh[e, k]) < shape[2 + k] for k in range(3))]
    return nh[keep]


def patch(shape, seed=0, nan=True):
    """ids 0..3 in blocks (so that neighbours often agree), with zeros, negatives, fractions that
    round to an id or to zero, and planted NaN"""
    rng = np.random.RandomState(seed)
    n, c, d, h, w = shape
    coarse = rng.randint(0, 4, (n, c, (d + 1) // 2, (h + 2) // 3, (w + 1) // 2))
    t = np.repeat(np.repeat(np.repeat(coarse, 2, 2), 3, 3), 2, 4)[:, :, :d, :h, :w].astype(np.float32)
    flat = t.reshape(-1)
    k = flat.size
    flat[rng.choice(k, max(1, k // 9), replace=False)] = -1.0
    flat[rng.choice(k, max(1, k // 11), replace=False)] += 0.25          # rounds back
    flat[rng.choice(k, max(1, k // 13), replace=False)] = 0.4             # rounds to zero
    flat[rng.choice(k, max(1, k // 17), replace=False)] = -0.3            # rounds to -0
    if nan:
        flat[rng.choice(k, max(1, k // 10), replace=False)] = np.nan
    t = flat.reshape(shape)
    t.setflags(write=False)
    return t


def ext(sp, s):
    return tuple(-(-int(a) // int(b)) for a, b in zip(sp, s))


def nan666(a):
    a = np.array(a, np.float32)
    a[np.isnan(a)] = -666.0
    return a


# ---- vectorised restatements ----------------------------------------------------------------------
def stride_np(t, s):
    return nan666(t[:, :, ::s[0], ::s[1], ::s[2]])


def _shift(t0, off, fill):
    """out[..., p] = t0[..., p - off] inside, fill outside; t0 (n, D, H, W)"""
    out = np.full(t0.shape, fill, np.float32)
    src, dst = [slice(None)], [slice(None)]
    for k in range(3):
        n, o = t0.shape[1 + k], int(off[k])
        lo, hi = max(0, o), n + min(0, o)           # p in [lo, hi)
        if hi <= lo:
            return out
        dst.append(slice(lo, hi))
        src.append(slice(lo - o, hi - o))
    out[tuple(dst)] = t0[tuple(src)]
    return out


def nhood_np(t, nhood, s, wrong=None):
    nhood = np.asarray(nhood, np.int32)
    fill = 0.0 if wrong == 'fill0' else -1.0
    sgn = -1 if wrong == 'sign' else 1
    chans = []
    for off in nhood:
        if wrong == 'stride_first':
            chans.append(_shift(t[:, 0, ::s[0], ::s[1], ::s[2]], sgn * off, fill))
        else:
            chans.append(_shift(t[:, 0], sgn * off, fill)[:, ::s[0], ::s[1], ::s[2]])
    out = np.stack(chans, axis=1)
    return nan666(np.concatenate([out, t[:, 1:, ::s[0], ::s[1], ::s[2]]], axis=1))


def affinity_np(t, nhood, s, wrong=None):
    nhood = np.asarray(nhood, np.int32)
    with np.errstate(invalid='ignore'):
        A = np.rint(t[:, 0, ::s[0], ::s[1], ::s[2]])
        sp = A.shape[1:]
        # ('full_extents': the edge is bounded by (D, H, W); a neighbour between the strided and
        # the full-resolution extents is read at the last strided voxel, as a clamped read would)
        bound = t.shape[2:] if wrong == 'full_extents' else sp
        sgn = -1 if wrong == 'sign' else 1
        idx = np.indices(sp)
        out = np.zeros((A.shape[0], len(nhood)) + sp, np.float32)
        for e, off in enumerate(nhood):
            q = [idx[k] + sgn * int(off[k]) for k in range(3)]
            inside = np.ones(sp, bool)
            for k in range(3):
                inside &= (q[k] >= 0) & (q[k] < bound[k])
            B = A[:, np.clip(q[0], 0, sp[0] - 1), np.clip(q[1], 0, sp[1] - 1),
                  np.clip(q[2], 0, sp[2] - 1)]
            pos = (A >= 0) & (B >= 0) if wrong == 'ge0' else (A > 0) & (B > 0)
            out[:, e] = inside[None] & (A == B) & pos
    return out


def count_negative_np(t, wrong=None):
    with np.errstate(invalid='ignore'):
        if wrong == 'nan_negative':
            return int((~(t >= 0)).sum())
        return int((t < 0).sum())


def barriers_np(ids, dilute, conn, ecs=0, wrong=None):
    """gather form: voxel v is marked through axis a iff one of the edges (v-2,v-1), (v-1,v),
    (v,v+1), (v+1,v+2) along a exists and differs (the outer two only when diluted) and v's other
    two coordinates are all <= n - 2 (forward pass) or all >= 1 (reversed pass)"""
    ids = np.asarray(ids, np.float32)
    sh = ids.shape
    barr = np.zeros(sh, bool)
    idx = np.indices(sh)
    for a in range(3):
        if not conn[a] or sh[a] < 2:
            continue
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, sh[a] - 1), slice(1, sh[a])
        diff = ids[tuple(lo)] != ids[tuple(hi)]               # edge (m, m + 1) at index m
        near = np.zeros(sh, bool)
        for k in ((-2, -1, 0, 1) if dilute[a] else (-1, 0)):   # edge index m = v + k
            m0, m1 = max(0, k), min(sh[a] - 1, sh[a] + k)      # m in [m0, m1) valid with v = m - k
            if m1 <= m0:
                continue
            src, dst = [slice(None)] * 3, [slice(None)] * 3
            src[a], dst[a] = slice(m0, m1), slice(m0 - k, m1 - k)
            near[tuple(dst)] |= diff[tuple(src)]
        others = [b for b in range(3) if b != a]
        fwd = np.ones(sh, bool)
        rev = np.ones(sh, bool)
        for b in others:
            fwd &= idx[b] <= sh[b] - 2
            rev &= idx[b] >= 1
        barr |= near & (fwd if wrong == 'no_reverse' else (fwd | rev))
    return _ecs(ids, barr.astype(np.float32), ecs)


def _ecs(ids, barr, ecs):
    if ecs == 1:
        return np.maximum((ids == 0).astype(np.float32), barr)
    if ecs == 2:
        barr = barr.copy()
        barr[(ids == 0) & (barr != 1)] = 2
    return barr


# ---- plain loops, from the definitions --------------------------------------------------------------
def stride_loop(t, s):
    n, c = t.shape[:2]
    d, h, w = ext(t.shape[2:], s)
    out = np.empty((n, c, d, h, w), np.float32)
    for i in np.ndindex(n, c, d, h, w):
        v = t[i[0], i[1], i[2] * s[0], i[3] * s[1], i[4] * s[2]]
        out[i] = -666.0 if np.isnan(v) else v
    return out


def nhood_loop(t, nhood, s):
    n, C, D, H, W = t.shape
    d, h, w = ext((D, H, W), s)
    E = len(nhood)
    out = np.empty((n, E + C - 1, d, h, w), np.float32)
    for b, z, x, y in np.ndindex(n, d, h, w):
        for e in range(E):
            q = (z * s[0] - nhood[e][0], x * s[1] - nhood[e][1], y * s[2] - nhood[e][2])
            v = t[b, 0, q[0], q[1], q[2]] if (0 <= q[0] < D and 0 <= q[1] < H and 0 <= q[2] < W) \
                else -1.0
            out[b, e, z, x, y] = -666.0 if np.isnan(v) else v
        for c in range(1, C):
            v = t[b, c, z * s[0], x * s[1], y * s[2]]
            out[b, E + c - 1, z, x, y] = -666.0 if np.isnan(v) else v
    return out


def affinity_loop(t, nhood, s):
    n, C, D, H, W = t.shape
    d, h, w = ext((D, H, W), s)
    out = np.zeros((n, len(nhood), d, h, w), np.float32)
    for b, z, x, y in np.ndindex(n, d, h, w):
        a = np.rint(t[b, 0, z * s[0], x * s[1], y * s[2]])
        for e, off in enumerate(nhood):
            q = (z + off[0], x + off[1], y + off[2])
            if not (0 <= q[0] < d and 0 <= q[1] < h and 0 <= q[2] < w):
                continue
            c = np.rint(t[b, 0, q[0] * s[0], q[1] * s[1], q[2] * s[2]])
            if a == c and a > 0 and c > 0:
                out[b, e, z, x, y] = 1.0
    return out


def count_negative_loop(t):
    return sum(1 for v in t.ravel() if v < 0)


def _pass(ids, barr, dilute, conn):
    n = ids.shape
    for c in np.ndindex(n[0] - 1, n[1] - 1, n[2] - 1) if min(n) > 1 else ():
        for a in range(3):
            if not conn[a]:
                continue
            e = [0, 0, 0]
            e[a] = 1
            at = lambda k: (c[0] + k * e[0], c[1] + k * e[1], c[2] + k * e[2])
            if ids[at(0)] != ids[at(1)]:
                barr[at(0)] = 1
                barr[at(1)] = 1
                if dilute[a]:
                    if c[a] > 0:
                        barr[at(-1)] = 1
                    if c[a] < n[a] - 2:
                        barr[at(2)] = 1


def barriers_loop(ids, dilute, conn, ecs=0):
    ids = np.asarray(ids, np.float32)
    barr = np.zeros(ids.shape, np.float32)
    _pass(ids, barr, dilute, conn)
    _pass(ids[::-1, ::-1, ::-1], barr[::-1, ::-1, ::-1], dilute, conn)   # (views: marks land in barr)
    return _ecs(ids, barr, ecs)


def id_volume(shape, seed=0):
    """a few labels in blocks, with zeros (ECS)"""
    rng = np.random.RandomState(seed)
    coarse = rng.randint(0, 4, tuple((n + 1) // 2 for n in shape))
    v = np.repeat(np.repeat(np.repeat(coarse, 2, 0), 2, 1), 2, 2)[:shape[0], :shape[1], :shape[2]]
    v = v.astype(np.float32)
    v[rng.rand(*shape) < 0.08] = 0.0
    v[rng.rand(*shape) < 0.05] = 5.0
    v.setflags(write=False)
    return v


BARRIER_VOLUMES = [(6, 7, 8), (2, 7, 8), (6, 2, 5), (5, 6, 2)]
BARRIER_FLAGS = [((True, True, True), (True, True, True)),
                 ((False, False, False), (False, False, False)),
                 ((False, True, True), (True, True, True)),
                 ((True, False, True), (True, True, False))]          # (dilute, connectivity)
