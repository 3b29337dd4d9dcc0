"""CPU: what csrc/stream_common.hpp shares among the streaming op files, checked on the host.

tests/stream_common_check.cpp includes the header, is compiled with the host compiler into a
stand-alone program and run: mk_div / fdiv against n / d on every divisor and dividend listed
there (exact equality, every magic below 2^32), stream_chunk against the loop it replaced.
Skipped where no host compiler or no HIP headers (common.hpp includes hip_runtime.h) are found."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hip_include_dir():
    roots = [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    for r in roots:
        if r and os.path.exists(os.path.join(r, "include", "hip", "hip_runtime.h")):
            return os.path.join(r, "include")
    return None


def test_divider_is_exact_and_chunk_sizing_is_the_loop_it_replaced(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    inc = hip_include_dir()
    if cxx is None or inc is None:
        pytest.skip("no host C++ compiler or no HIP headers")
    exe = str(tmp_path / "stream_common_check")
    base = [cxx, "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", inc,
            "-I", os.path.join(ROOT, "elektronn2_amd", "csrc"),
            os.path.join(ROOT, "tests", "stream_common_check.cpp"), "-o", exe]
    # with the sanitizers where the compiler has their runtimes, plain otherwise
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    checks, failed = [int(w) for w in r.stdout.split() if w.isdigit()][-2:]
    assert failed == 0 and checks > 2000, r.stdout
