"""CPU, nothing loaded into Python: tests/host/umi_directional_check.cpp includes the directional
clusters' header (sctools_amd/csrc/umi_directional.h: the edge test written without overflow, the
labels' order), is compiled by the host C++ compiler with AddressSanitizer and UBSan, and its answers
are compared with the big-integer statements of tests/umi_directional_reference.py case by case."""

import os
import random
import shutil
import subprocess

import pytest

import umi_collapse_reference as U
import umi_directional_reference as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNERS = [1, 2, 3, 2 ** 32, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1]


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("umidir") / "umi_directional_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, os.path.join(ROOT, "tests", "host", "umi_directional_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, cases):
    """cases: (u_reads, v_reads, a_reads, a_code, b_reads, b_code)."""
    text = "".join("%d %d %d %d %d %d\n" % c for c in cases)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True, timeout=120)
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok %d" % len(cases), lines[-1]
    for (u, v, ra, ca, rb, cb), line in zip(cases, lines[:-1]):
        edge, label_less, support_less = (int(x) for x in line.split())
        assert edge == int(u >= 2 * v - 1) == int(D.edge(u, v)), (u, v)
        assert label_less == support_less == int(U.support_less(ra, ca, rb, cb)), (ra, ca, rb, cb)


def test_every_pair_of_corner_counts(check_program):
    """All 49 pairs of {1, 2, 3, 2^32, 2^63 - 1, 2^63, 2^64 - 1} as reads of u and v, and as the
    reads and codes of two labels: 2 * v - 1 does not fit 64 bits for the upper three."""
    cases = [(u, v, u, v, v, u) for u in CORNERS for v in CORNERS]
    cases += [(u, v, u, 5, v, 5) for u in CORNERS for v in CORNERS]
    cases += [(1, 1, r, a, r, b) for r in CORNERS for a in CORNERS for b in CORNERS]
    _run(check_program, cases)
    assert D.edge(2 ** 64 - 1, 2 ** 63) and not D.edge(2 ** 64 - 2, 2 ** 63) and not D.edge(2 ** 63, 2 ** 63)


def test_random_counts(check_program):
    """4,000 random pairs: small counts around 2 * v - 1, and full-width ones."""
    rng = random.Random(9)
    cases = []
    for _ in range(2000):
        v = rng.randint(1, 40)
        u = max(1, 2 * v - 1 + rng.randint(-2, 2))
        cases.append((u, v, rng.randint(0, 3), rng.getrandbits(30), rng.randint(0, 3), rng.getrandbits(30)))
    for _ in range(2000):
        v = rng.randint(1, 2 ** 64 - 1)
        u = rng.choice((rng.randint(1, 2 ** 64 - 1), min(2 ** 64 - 1, max(1, 2 * v - 1 + rng.randint(-1, 1))), v))
        a, b = rng.getrandbits(63), rng.getrandbits(63)
        cases.append((u, v, u, a, rng.choice((u, v)), rng.choice((a, b))))
    _run(check_program, cases)
