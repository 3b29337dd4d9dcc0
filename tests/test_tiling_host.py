"""CPU: elektronn2_amd/tiling.py -- the one reader of the tiling strings and the one writer of the
tuning table's keys -- against literal expectations and against every string the project really
uses: the shipped table, the tuner's candidate generators, the tilings the tests pin."""
import glob
import json
import os
import re

import pytest

from elektronn2_amd import tiling

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# the forms of test_host_logic.test_tiling_candidate_lists, one expression per family
IGEMM_FORMS = {'16x16x4': r"\d+,\d+,\d+,\d+", '4x4x1': r"4(,\d+){7}",
               'pointwise': r"1,\d+,[12](,(32|64|128),0)?", 'memory': r"32,\d+,\d+"}
WGRAD_FORM = r"\d+,\d+,\d+,\d+,\d+"


def shipped():
    with open(os.path.join(ROOT, "elektronn2_amd", "tuned.json")) as f:
        return json.load(f)


def family_by_form(kind, s):
    if kind == 'wgrad':
        assert re.fullmatch(WGRAD_FORM, s), s
        return 'memory' if s.startswith('32,') else 'wgrad'
    fams = [f for f, rx in IGEMM_FORMS.items() if re.fullmatch(rx, s)]
    # ("4,a,b,c" is a 16x16x4 string with MT = 4 AND nothing else: the 4x4x1 form has 8 fields)
    assert len(fams) == 1, (s, fams)
    return fams[0]


def real_strings():
    """(kind, string) of every tiling the project holds: non-empty values of the shipped table and of
    the table fixtures under tests/golden, the candidate generators on the problems of
    test_tiling_candidate_lists, and the literals the tests pin"""
    from elektronn2_amd import autotune as A
    out = set()
    tables = [shipped()]
    for p in glob.glob(os.path.join(HERE, "golden", "*.json")):
        with open(p) as f:
            d = json.load(f)
        if isinstance(d, dict) and all(isinstance(v, str) and "|" in k for k, v in d.items()):
            tables.append(d)
    for d in tables:
        for k, v in d.items():
            kind = k.split("|")[0].replace("_bf16", "")
            if kind != 'side' and v:
                out.add((kind, v))
    k1, k3, sp = (1, 1, 1), (1, 3, 3), (10, 37, 37)
    ig = (A.pointwise_candidates(200, k1) + A.pointwise_candidates(200, k1, cin=20) +
          A.igemm_candidates(200, 200, k1, sp) + A.igemm_candidates(200, 200, k3, sp) +
          A.igemm_candidates(200, 200, k3, sp, split_k=False) + A.igemm4_candidates(20, 40, k3, sp) +
          A.igemm4_candidates(200, 200, k1, sp) + A.bf16_memory_candidates(20) +
          A.bf16_memory_candidates(200))
    wg = (A.wgrad_candidates(200, 200, k3, sp) + A.wgrad_candidates(2048, 256, k1, (18, 10, 10)) +
          A.position_split_wgrad_candidates(200, 200, k3, sp) +
          A.even_split_wgrad_candidates(200, 200, k3, sp) +
          A.pointwise_wgrad_candidates(2048, 256, k1, (18, 10, 10)) +
          A.pointwise_wgrad_candidates(200, 200, k1, sp) + A.bf16_wgrad_candidates(64, (2, 4, 4)))
    for cin in (20, 40, 100, 200, 8):
        wg += A.bf16_wgrad_candidates(cin, k3)
    assert len(ig) > 100 and len(wg) > 100
    out.update(('igemm', c) for c in ig)
    out.update(('wgrad', c) for c in wg)
    # literals of the test sources: 3, 4 or 8 fields are 'igemm' strings, 5 fields a 'wgrad' string
    # or the long pointwise form
    me = os.path.abspath(__file__)
    n_lit = 0
    for p in glob.glob(os.path.join(HERE, "*.py")):
        if os.path.abspath(p) == me:
            continue
        with open(p) as f:
            src = f.read()
        for s in re.findall(r"""["'](\d+(?:,\d+){2,7})["']""", src):
            n = s.count(",") + 1
            if n in (3, 4, 8):
                out.add(('igemm', s))
            elif n == 5:
                out.add(('igemm' if re.fullmatch(IGEMM_FORMS['pointwise'], s) else 'wgrad', s))
            else:
                continue
            n_lit += 1
    assert n_lit > 200
    return sorted(out)


@pytest.mark.parametrize("s,m,want", [
    ("7,2,32,1", 100, 128), ("5,2,16,1", 20, 96), ("13,1,64,1", 200, 224),
    ("4,5,1,8,1,3,4,1", 20, 64), ("1,13,1", 200, 224), ("1,13,1,64,0", 200, 224),
    ("32,1,2", 200, 224), ("", 64, 0), ("7,2,9", 64, 0), ("x,1", 64, 0),
    # (further rows, taken the same way from Plan._tile_rows before it moved)
    ("10,2,16,2", 150, 160), ("3,4,12,1", 40, 64), ("1,7,2", 2, 128), ("4,13,1,16,1,2,4,1", 200, 224),
    ("32,4,1", 20, 32), (None, 64, 0), ("4,5,1,8,1,3,4", 20, 0), ("2,1,8", 20, 0)])
def test_rows_reached(s, m, want):
    assert tiling.rows_reached(tiling.parse('igemm', s), m) == want


def test_parse_rejects_what_is_no_tiling():
    for kind in ('igemm', 'wgrad'):
        for s in ("", None, "x,1", "7,2,9,", "7", "7,2", "1.5,2,3,4"):
            assert tiling.parse(kind, s) is None, (kind, s)
    assert tiling.parse('igemm', "7,2,9") is None and tiling.parse('igemm', "4,5,1,8,1,3,4") is None
    assert tiling.parse('wgrad', "7,2,32,1") is None and tiling.parse('other', "7,2,32,1") is None
    t = tiling.parse('wgrad', "7,2,101,128,8")
    assert (t.kind, t.family, t.v, t.WK, t.xcd_grouped) == ('wgrad', 'wgrad', (7, 2, 101, 128, 8), 101, True)
    assert not tiling.parse('wgrad', "7,2,9,0,4").xcd_grouped
    assert not tiling.parse('wgrad', "32,1,200,0,1").xcd_grouped      # (NB of a memory form is no WK)
    # the four families of a forward / data-gradient launch, and which images get rows of their own
    own = {s: tiling.own_row_length(tiling.parse('igemm', s))
           for s in ("7,2,32,1", "4,5,1,8,1,3,4,1", "1,13,1", "1,13,1,64,0", "32,1,2")}
    assert own == {"7,2,32,1": True, "4,5,1,8,1,3,4,1": False, "1,13,1": True, "1,13,1,64,0": True,
                   "32,1,2": False}
    assert not tiling.own_row_length(None)


def test_every_real_string_parses_into_the_family_of_its_form():
    strings = real_strings()
    seen = set()
    for kind, s in strings:
        t = tiling.parse(kind, s)
        assert t is not None, (kind, s)
        assert t.kind == kind and t.v == tuple(int(q) for q in s.split(","))
        assert t.family == family_by_form(kind, s), (kind, s, t.family)
        seen.add((kind, t.family))
    assert seen == {('igemm', '16x16x4'), ('igemm', '4x4x1'), ('igemm', 'pointwise'),
                    ('igemm', 'memory'), ('wgrad', 'wgrad'), ('wgrad', 'memory')}


def test_predicates_agree_with_the_tests_they_replace():
    def old_bf16_tile(s):          # (the body Context.bf16_tile had)
        v = (s or '').split(',')
        if len(v) >= 3 and v[0] == '32':
            return int(v[1]), int(v[2])
    n_mem = n_grp = 0
    for kind, s in real_strings():
        assert tiling.is_memory_form(kind, s) == s.startswith('32,'), (kind, s)
        n_mem += s.startswith('32,')
        if kind == 'igemm':
            assert tiling.bf16_tile(s) == old_bf16_tile(s), s
        else:
            # the tuner's preference for the XCD-grouped order (autotune.tuned_call)
            assert tiling.parse(kind, s).xcd_grouped == \
                (not s.startswith('32,') and int(s.split(",")[2]) >= 100), s
            n_grp += tiling.parse(kind, s).xcd_grouped
    assert n_mem > 20 and n_grp > 5
    for s in ("", None):
        assert not tiling.is_memory_form('igemm', s) and not tiling.is_memory_form('wgrad', s)
        assert tiling.bf16_tile(s) is None


def test_table_keys():
    sig = (0, 8, 1, 1, 3, 3, 5, 45, 45, 47)
    assert tiling.key('igemm', sig, False) == "igemm|0,8,1,1,3,3,5,45,45,47"
    assert tiling.key('igemm', sig, True) == "igemm_bf16|0,8,1,1,3,3,5,45,45,47"
    assert tiling.key('wgrad', sig[1:], True).startswith("wgrad_bf16|8,1,")
    assert tiling.side_key(sig) == "side|" + "0,8,1,1,3,3,5,45,45,47"
    import numpy as np
    assert tiling.key('igemm', [np.int64(3), 4.0, True], False) == "igemm|3,4,1"
    # every key of the shipped table from its own parts
    table = shipped()
    assert len(table) > 100
    for k in table:
        head, sig = k.split("|")
        sig = [int(v) for v in sig.split(",")]
        if head == 'side':
            assert tiling.side_key(sig) == k
        else:
            assert head.replace("_bf16", "") in ('igemm', 'wgrad')
            assert tiling.key(head.replace("_bf16", ""), sig, head.endswith("_bf16")) == k
