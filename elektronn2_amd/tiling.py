"""The tiling strings of the conv GEMM launches and the keys of the tuning table, read and
written in ONE place on the host side.  The library reads a string in one place too,
``e2_set_tiling`` (csrc/conv_host.hpp), and keeps the parsed list; both sides state the grammar in
the same words (include/e2hip.h, e2_set_tiling):

A tiling string is a comma-separated list of at most 8 integers (an optional '-' and decimal
digits each, within 32 bits), nothing else -- no blanks, no '+', no trailing comma -- of at most
63 characters.  With n integers v0, v1, ...: ``kind == 'igemm'`` (forward and data gradient):
  n == 4                "MT,NT,CC,SK"               the 16x16x4 kernel             family '16x16x4'
  n == 8, v0 == 4       "4,MG,NT,CC,SK,WM,WN,G"     the 4x4x1 kernel               family '4x4x1'
  n == 3 or 5, v0 == 1  "1,MT,NT" / "1,MT,NT,KC,0"  the pointwise (1x1x1) GEMM     family 'pointwise'
  n >= 3, v0 == 32      "32,MB,NB"                  bf16 operands in memory        family 'memory'
``kind == 'wgrad'`` (weight gradient), n == 5:
  v0 == 32              "32,MB,NB,R,S"              bf16 operands in memory        family 'memory'
  otherwise             "MT,NT,WK,BP,PS"            its kernel: wgrad_route        family 'wgrad'
The rows are tried in this order.  "32,2,2,1" is therefore a 16x16x4 string here and to the
library's packed launches, while e2_conv3d_*_bf16 -- which asks only for the last 'igemm' row --
reads the tile (2, 2) out of it: the one string that two launchers take for their own.
``e2_set_tiling`` also takes any 5 integers for 'igemm'; a packed launch then refuses those that
do not start with 1.

A table key is "<kind>[_bf16]|<sig>", or "side|<sig>" for the per-problem side-stream flag of a
weight gradient; <sig> is the launch's signature, integers joined by commas.

This module imports nothing from the package: it works without the shared library."""
import re
from collections import namedtuple

_LIST = re.compile(r"-?[0-9]+(,-?[0-9]+){0,7}")


WgradRoute = namedtuple('WgradRoute', 'family MT NT WK BP wave_split xcd splits bands groups refuse six')


class Tiling(namedtuple('Tiling', 'kind family v')):
    """a parsed tiling string: its kind, its kernel family and its integers"""
    __slots__ = ()

    @property
    def WK(self):
        return wgrad_route(self, True).WK if self.family == 'wgrad' else None

    @property
    def xcd_grouped(self):
        """weight gradient: the direct kernel with the XCD-grouped block order (as the launch plan
        calls it: through the padded-gradient entry point)"""
        return self.family == 'wgrad' and wgrad_route(self, True).xcd


def wgrad_route(t, dy_padded, bf16=False):
    """The kernel a 'wgrad' tiling "MT,NT,WK,BP,PS" runs, as the library decodes it -- once per
    launch, csrc/conv_host.hpp e2_wgrad_route; ``family`` is the name e2_last_launch reports.  Tried
    in this order (the same words: conv_host.hpp):
      WK == 7                          the K-contiguous 1x1x1 GEMM (BP ignored)           pw_wgrad
      WK == 8                          ... one tile per work-group, waves split positions pw_wgrad_ks
      WK == 9                          ... for kernels with taps                          wgrad_ks
          (8 / 9 with BP >= 1: the "even" form, PS work-groups over BP bands)
      WK == 18 / 19                    8 / 9 with every f32 product made of six bf16
                                       MFMA products (same families, same BP / PS)       pw_wgrad_ks / wgrad_ks
      dy padded, WK in {1, 14, 101, 114}, BP in {128, 256}
                                       the direct kernel; WK % 100 == 14: the waves split
                                       the quads; WK >= 100: XCD-grouped block order      wgrad_direct
      otherwise WK == 14 or WK >= 100  refused
      otherwise BP not 64 or 128       refused
      otherwise WK in {0, 1}, or WK == 4 with NT == 1 (the waves split K)
                                       the LDS-staged kernel                              wgrad_lds
      otherwise                        refused
    A refused route keeps the family of the LDS-staged kernel (``refuse``: why).  ``dy_padded``: the
    launch comes through the padded-gradient entry point (the launch plan's always do); ``bf16``:
    the operands are rounded to bf16, which only the direct kernel's name shows.  BP is 0 where it
    is no tile length, bands / groups are 0 outside the even form; WK is the field as written; ``six``:
    the six-product form (WK 18 / 19)."""
    assert t.kind == 'wgrad' and t.family == 'wgrad', t
    MT, NT, WK, BP, PS = t.v
    r = dict(family='wgrad_lds', MT=MT, NT=NT, WK=WK, BP=0, wave_split=False, xcd=False, splits=PS,
             bands=0, groups=0, refuse=None, six=False)
    if WK == 7:
        r.update(family='pw_wgrad')
    elif WK in (8, 9, 18, 19):
        r.update(family='pw_wgrad_ks' if WK % 10 == 8 else 'wgrad_ks', six=WK >= 18)
        if BP >= 1:
            r.update(bands=BP, groups=PS)
    elif dy_padded and WK in (1, 14, 101, 114) and BP in (128, 256):
        r.update(family='wgrad_direct_bf16r' if bf16 else 'wgrad_direct', BP=BP,
                 wave_split=WK % 100 == 14, xcd=WK >= 100)
    else:
        r.update(BP=BP)
        if WK == 14 or WK >= 100:
            r.update(refuse="WK=14/101/114 need the padded-gradient entry point and BP 128/256")
        elif BP not in (64, 128):
            r.update(refuse="BP must be 64 or 128")
        elif not (WK in (0, 1) or (WK == 4 and NT == 1)):
            r.update(refuse="WK=4 needs NT=1")
        else:
            r.update(wave_split=WK == 4)
    return WgradRoute(**r)


def parse(kind, s):
    """the Tiling of a string, or None for an empty, malformed or unknown one"""
    if not s or len(s) > 63 or not _LIST.fullmatch(s):
        return None
    v = tuple(int(t) for t in s.split(","))
    if any(abs(q) >= 2 ** 31 for q in v):
        return None
    fam = None
    if kind == 'igemm':
        if len(v) == 4:
            fam = '16x16x4'
        elif len(v) == 8 and v[0] == 4:
            fam = '4x4x1'
        elif len(v) in (3, 5) and v[0] == 1:
            fam = 'pointwise'
        elif len(v) >= 3 and v[0] == 32:
            fam = 'memory'
    elif kind == 'wgrad' and len(v) == 5:
        fam = 'memory' if v[0] == 32 else 'wgrad'
    return Tiling(kind, fam, v) if fam else None


def rows_reached(t, m):
    """how far the M tiles of a conv GEMM launch with the ('igemm') tiling ``t`` reach for m output
    rows, or 0 (= the repack's default) when there is none / it is of another kernel family"""
    if t is None or t.kind != 'igemm':
        return 0
    v = t.v
    if t.family == '16x16x4':
        per = 16 * v[0]
    elif t.family == '4x4x1':
        per = 4 * v[1] * v[5]
    elif t.family == 'pointwise':
        per = 16 * v[1]
    else:                                             # bf16 operands in memory: image not read
        per = 16
    # (whole 128-byte lines: a line the repack writes only in part is merged with memory when the
    # GEMM fetches it -- rows cut at 80 made the 5 x 2 tiles 6 % slower)
    return -(-(-(-m // per) * per) // 32) * 32


def own_row_length(t):
    """does the weight image a launch with tiling ``t`` reads get a row length of its own?  Only
    for the 16x16x4 / pointwise kernels (the 4x4x1 kernel's lanes read 64 consecutive floats per
    row; a memory-form tiling does not read the image, but the launch that replaces it under
    another pin would)
    (measured for the 4x4x1 kernel too -- rows of 64 floats for 20 channels --: neuro3d_lite
    +5 us, neuro3d -5 us, not of one sign: its images keep the formula)"""
    return t is not None and t.family in ('16x16x4', 'pointwise')


def is_memory_form(kind, s):
    """the string selects the kernel of its kind that reads bf16 operands from memory"""
    t = parse(kind, s)
    return t is not None and t.family == 'memory'


def bf16_tile(s):
    """(MB, NB) of a memory-form 'igemm' tiling string, else None"""
    t = parse('igemm', s)
    return (t.v[1], t.v[2]) if t is not None and t.family == 'memory' else None


def _sig(sig):
    return ",".join(str(int(v)) for v in sig)


def key(kind, sig, bf16):
    """the table key of a launch (the bf16 operand form of a kernel has its own best tiling)"""
    return "%s%s|%s" % (kind, "_bf16" if bf16 else "", _sig(sig))


def side_key(sig):
    """the table key of the side-stream flag of the weight gradient with signature ``sig``"""
    return "side|" + _sig(sig)
