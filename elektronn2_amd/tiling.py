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
  otherwise             "MT,NT,WK,BP,PS"            WK >= 100: XCD-grouped         family 'wgrad'
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


class Tiling(namedtuple('Tiling', 'kind family v')):
    """a parsed tiling string: its kind, its kernel family and its integers"""
    __slots__ = ()

    @property
    def WK(self):
        return self.v[2] if self.family == 'wgrad' else None

    @property
    def xcd_grouped(self):
        """weight gradient: the XCD-grouped block order"""
        return self.family == 'wgrad' and self.v[2] >= 100


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
