"""CPU: the host side of the conv launches (csrc/conv_host.hpp) -- the tiling grammar behind
e2_set_tiling and the builders of the conv GEMM arguments -- checked with the definitions the
library itself compiles.

tests/conv_host_check.cpp includes the header, is compiled with the host compiler and
-fsanitize=address,undefined into a stand-alone program and run.  It holds a table, written out by
hand, of tiling strings with what the one parser must make of each (n, v), whether e2_set_tiling
accepts it per kind, and which of the launch sites' predicates hold; and literal IgemmArgs /
WgradArgs for dense and strided views (forward, data gradient, padded weight gradient, UpConv) and
for the defaults.  The program prints its table; this module holds elektronn2_amd/tiling.py -- the
host side's reader of the same strings -- against it.

The same program holds the route of a weight-gradient tiling (e2_wgrad_route: which kernel runs
"MT,NT,WK,BP,PS", with which named fields, or that it is refused) to a table written out by hand
and, over a grid of the five integers, to a copy of the if-chain it replaced; and the limits of the
K-contiguous weight-gradient GEMMs to literal problems.  It prints the route table too, and
tiling.wgrad_route is held to every row."""
import os
import shutil
import subprocess

import pytest

from elektronn2_amd import tiling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKED = {0: '16x16x4', 1: 'pointwise', 4: '4x4x1'}
# (put together: test_tiling_host.py collects the tiling literals of every test module and holds
# each to ONE form, which is just what this string has not)
AMBIGUOUS = "32,2,2" + ",1"


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    # (the library's own build needs a host compiler too: csrc/Makefile, malis.cpp)
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("conv_host") / "conv_host_check")
    # always with the sanitizers: a compiler without their runtimes fails the test, it does not
    # quietly check less
    build = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "elektronn2_amd", "csrc"),
                            os.path.join(ROOT, "tests", "conv_host_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    word, checks = lines[-1].split()
    assert word == "ok" and int(checks) > 1000, lines[-1]
    out = dict(row=[], route=[], grid=[])
    for ln in lines[:-1]:
        tag, s, *f = ln.split("\t")
        if tag == "row":
            assert len(f) == 8, ln
            wf, n, ig, wg, form, cb, cand, wb = (int(q) for q in f)
            out[tag].append(dict(s=s, well_formed=bool(wf), n=n, igemm=bool(ig), wgrad=bool(wg), form=form,
                                 cb=bool(cb), cand=bool(cand), wb=bool(wb)))
        elif tag == "route":
            assert len(f) == 12, ln
            padded, name, name_bf16 = bool(int(f[0])), f[1], f[2]
            MT, NT, BP, ws, xcd, splits, bands, groups, refused = (int(q) for q in f[3:])
            out[tag].append(dict(s=s, padded=padded, name=name, name_bf16=name_bf16, MT=MT, NT=NT, BP=BP,
                                 wave_split=bool(ws), xcd=bool(xcd), splits=splits, bands=bands,
                                 groups=groups, refused=bool(refused)))
        else:
            assert tag == "grid" and len(f) == 1, ln
            out[tag].append((int(s), int(f[0])))
    return out


@pytest.fixture(scope="module")
def rows(tables):
    return tables['row']


def test_the_parser_and_the_builders_pass_their_host_check(rows):
    by = {r['s']: r for r in rows}
    assert len(rows) >= 35 and len(by) == len(rows)
    # the rows the issue of this check names, as the table holds them
    assert by["1,2,2,64,0"]['igemm'] and by["1,2,2,64,0"]['form'] == 1
    assert by["3,4,5,6,7"]['igemm'] and by["3,4,5,6,7"]['form'] == -1
    assert by["32,2,2"]['igemm'] and not by["32,2,2"]['wgrad']
    for s in ("1,2,3,4,5,6,7,8,9", "4,1,2,3,", "4,1,2,x", " 4,1,2,3"):
        assert not by[s]['well_formed']
    assert by["1,2,3,4,5,6"]['well_formed'] and not by["1,2,3,4,5,6"]['igemm'] and not by["1,2,3,4,5,6"]['wgrad']
    assert sorted(len(s) for s in by)[-2:] == [63, 64]
    assert [r['well_formed'] for r in rows if len(r['s']) >= 63] == [True, False]


def test_tiling_py_reads_every_row_as_the_library_does(rows):
    """the two grammars agree: on what is a list of integers at all, on its integers, and on the
    kernel family for every string e2_set_tiling accepts"""
    n_fam = 0
    for r in rows:
        s = r['s']
        for kind in ('igemm', 'wgrad'):
            t = tiling.parse(kind, s)
            if not r['well_formed'] or not s:
                assert t is None, (kind, s)
                continue
            if t is not None:
                assert len(t.v) == r['n'] and ",".join(map(str, t.v)) == ",".join(str(int(q)) for q in s.split(","))
            if not r[kind]:
                continue
            if kind == 'wgrad':
                lib = 'memory' if r['wb'] else 'wgrad'
            else:
                lib = PACKED.get(r['form'], 'memory' if r['cb'] else None)
            assert (t.family if t is not None else None) == lib, (kind, s, t, lib)
            n_fam += lib is not None
    assert n_fam >= 19            # (kind, accepted row) pairs with a family in the table


def test_the_one_string_two_launchers_take_for_their_own(rows):
    """AMBIGUOUS: four integers -- a 16x16x4 tiling (MT = 32) to tiling.py, to e2_set_tiling and
    to the packed launches; e2_conv3d_*_bf16 asks only for three integers behind a 32 and reads the
    tile (2, 2).  Pinned, not resolved: no shipped or generated string is of this kind
    (test_tiling_host.py holds every real string to ONE form)."""
    r = next(q for q in rows if q['s'] == AMBIGUOUS)
    assert r['igemm'] and r['form'] == 0 and r['cb']
    t = tiling.parse('igemm', AMBIGUOUS)
    assert t.family == '16x16x4' and tiling.bf16_tile(AMBIGUOUS) is None and not tiling.is_memory_form('igemm', AMBIGUOUS)
    # every other accepted row has one reading
    for q in rows:
        if q['igemm'] and q['s'] != AMBIGUOUS:
            assert not (q['form'] in PACKED and q['cb']), q['s']


def test_the_wgrad_route_equals_the_chain_it_replaced(tables):
    """the check program's grid: MT x NT x WK (-1 .. 15, 99 .. 115) x BP x PS x padded x bf16, family
    name, every field and refused-or-not against the if-chain of e2i_wgrad_conv before the route"""
    assert tables['grid'] == [(2 * 3 * 34 * 7 * 3 * 2 * 2, 0)]


def test_tiling_py_decodes_every_route_as_the_library_does(tables):
    routes = tables['route']
    assert len(routes) >= 35
    by = {(r['s'], r['padded']): r for r in routes}
    assert len(by) == len(routes)
    # rows the table must hold, as it holds them
    assert by["1,1,1,128,2", False]['name'] == "wgrad_lds" and by["1,1,1,128,2", True]['name'] == "wgrad_direct"
    assert by["1,1,1,64,2", True]['name'] == "wgrad_lds" and not by["1,1,1,64,2", True]['refused']
    for k in (("1,2,14,128,2", False), ("1,1,14,64,2", True), ("1,1,55,128,1", True), ("1,1,55,128,1", False),
              ("1,2,4,64,1", False)):
        assert by[k]['refused'] and by[k]['name'] == "wgrad_lds", k
    assert by["2,2,7,5,3", True]['name'] == "pw_wgrad" and by["2,2,7,5,3", True]['BP'] == 0
    assert (by["7,2,9,3,512", True]['bands'], by["7,2,9,3,512", True]['groups']) == (3, 512)
    assert {r['name'] for r in routes} == {"wgrad_lds", "wgrad_direct", "pw_wgrad", "pw_wgrad_ks", "wgrad_ks"}
    wks = {int(r['s'].split(",")[2]) for r in routes if not r['refused']}
    assert wks >= {0, 1, 4, 14, 101, 114, 7, 8, 9}
    for r in routes:
        t = tiling.parse('wgrad', r['s'])
        assert t is not None and t.family == 'wgrad', r['s']
        for bf16 in (False, True):
            g = tiling.wgrad_route(t, r['padded'], bf16)
            assert g.family == (r['name_bf16'] if bf16 else r['name']), (r, g)
            assert (g.MT, g.NT, g.BP, g.wave_split, g.xcd, g.splits, g.bands, g.groups, g.refuse is not None) == \
                (r['MT'], r['NT'], r['BP'], r['wave_split'], r['xcd'], r['splits'], r['bands'], r['groups'],
                 r['refused']), (r, g)
        assert g.WK == t.v[2] == t.WK
        # the XCD-grouped order is the direct kernel's: the padded entry point's reading
        if r['padded']:
            assert t.xcd_grouped == r['xcd'], r
