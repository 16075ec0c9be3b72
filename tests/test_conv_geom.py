"""Host-side convolution geometry shared by the fp32 and bf16 contraction files (cultionet_amd/csrc/cn_conv_geom.h):
output sizes, floor division, the dense tap table of the gather form, and the parity classes of the scatter form
out[o] += src[(o + pad - k*dil) / s] * W[k] (where divisible) with their stable "more taps first" order.

tests/conv_geom_check.cpp includes that header alone, compares it with brute-force definitions over every kernel size
1..3, stride 1..4, padding 0..2, dilation 1..3 and output size 1..9 per axis, and is built here with the system C++
compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once as a child process. No GPU.
"""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cultionet_amd", "csrc")

N_GEOM = 3 * 3 * 4 * 3 * 3  # (KH, KW, stride, pad, dil)
N_SIZES = sum(
    (1 if n + 2 * pad >= dil * (k - 1) + 1 else 0) + s  # one Conv2d case where the kernel fits, out_pad 0..s-1
    for _kh in range(3) for _kw in range(3)
    for s in range(1, 5) for pad in range(3) for dil in range(1, 4) for k in range(1, 4) for n in range(1, 10)
)
EXPECTED_CASES = {
    "cover": N_GEOM * 81,  # every (Ho, Wo) in 1..9 x 1..9
    "taps": N_GEOM * 45 * 45,  # every output position of every (Ho, Wo)
    "order": N_GEOM * 81,
    "gather": N_GEOM,
    "sizes": N_SIZES,
    "floordiv": 4 * 81,
}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("conv_geom") / "conv_geom_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(HERE, "conv_geom_check.cpp"), "-o", exe]
    # gcc links the sanitizer runtimes as shared libraries unless told otherwise, and a shared ASan runtime refuses to
    # start in an environment that preloads any other library: link them into the program where the compiler can
    for extra in (["-static-libasan", "-static-libubsan"], []):
        build = subprocess.run(cmd + extra, capture_output=True, text=True)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = {}
    for line in run.stdout.splitlines():
        name, cases, failures = line.split()
        lines[name] = (int(cases.split("=")[1]), int(failures.split("=")[1]))
    return run, lines


def test_runs_clean_under_sanitizers(report):
    run, lines = report
    assert run.returncode == 0, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
    assert set(lines) == set(EXPECTED_CASES)


@pytest.mark.parametrize("check", sorted(EXPECTED_CASES))
def test_geometry_check(report, check):
    """cover: every output position belongs to exactly one parity class; taps: a class's taps are exactly the brute-force
    (input offset, k) pairs, each once, with wt = ky*KW + kx; order: descending tap count, ties in enumeration order;
    gather: the dense tap table; sizes: cn_conv_out / cn_convt_out against counting and the closed forms; floordiv."""
    run, lines = report
    assert check in lines, run.stdout + run.stderr
    cases, failures = lines[check]
    assert failures == 0, run.stderr
    assert cases == EXPECTED_CASES[check]
