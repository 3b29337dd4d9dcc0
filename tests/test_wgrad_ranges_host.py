"""CPU: the even position ranges of the weight-gradient GEMM (csrc/wgrad_even.hpp), checked on
the host with the definition the kernel itself compiles.

tests/wgrad_ranges_check.cpp includes the header, is compiled with the host compiler and
-fsanitize=address,undefined into a stand-alone program and run: for
T in 1..12 tiles, U in 1..60 units, G in 1..2 T U work-groups and the two flagship geometries
(57, 460, 256) and (43, 500, 256) the segments of all work-groups cover every (tile, unit) pair
exactly once, none is empty, a work-group has at most ceil(range / U) + 1 of them, range lengths
differ by at most one unit, and every tile's last unit (the owner of the masked K % 32 step of the
1x1x1 form) has exactly one owner.  The same for the band-major order (B > 1 bands of units) on a
thinner grid of shapes, where a segment is at most a band and the bound counts the shortest band."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_even_ranges_cover_every_pair_exactly_once(tmp_path):
    # (the library's own build needs a host compiler too: csrc/Makefile, malis.cpp)
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "wgrad_ranges_check")
    # always with the sanitizers: a compiler without their runtimes fails the test, it does not
    # quietly check less
    build = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "elektronn2_amd", "csrc"),
                            os.path.join(ROOT, "tests", "wgrad_ranges_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    word, cases = r.stdout.split()
    # tile-major: sum over T, U of 2 T U work-group counts; + the band cases and flagship geometries
    assert word == "ok" and int(cases) > 2 * 78 * 1830 + 16, r.stdout
