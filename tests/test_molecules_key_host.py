"""CPU, nothing loaded into Python: tests/host/molecules_key_check.cpp includes the molecule
counter's key header (sctools_amd/csrc/molecules_key.h: key packing, the SWAR bad-UMI test, the
parameter check), is compiled by the host C++ compiler with AddressSanitizer and UBSan, and its
answers are compared with tests/molecules_reference.py case by case."""

import os
import random
import shutil
import subprocess

import pytest

import molecules_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("molkey") / "molecules_key_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, os.path.join(ROOT, "tests", "host", "molecules_key_check.cpp"), "-o", exe], check=True)
    return exe


def _expected(nw, kind, L, index, umi):
    try:
        umi_bits = R.check_params(nw, kind, L)
    except ValueError:
        return [0, 0, 0, 0, 0, 0]
    bad = R.umi_is_bad(umi, kind, L)
    if bad:
        return [umi_bits, R.idx_bits(nw), 1, 0, 0, 0]
    return [umi_bits, R.idx_bits(nw), 0, R.key(index, umi, kind, L), index, umi]


def _run(exe, cases):
    text = "".join("%d %d %d %d %d\n" % c for c in cases)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True, timeout=120)
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok %d" % len(cases), lines[-1]
    got = [[int(x) for x in ln.split()] for ln in lines[:-1]]
    for case, g in zip(cases, got):
        assert g == _expected(*case), (case, g, _expected(*case))


def test_every_two_base_threebit_value(check_program):
    """All 128 values of 7 bits against a 6-bit UMI: 16 good ones, N, 0 / 5 / 7, the high bit."""
    cases = [(3, 3, 2, u % 3, u) for u in range(128)]
    assert sum(not R.umi_is_bad(u, 3, 2) for u in range(128)) == 16
    _run(check_program, cases)


def test_random_twelve_base_threebit_values(check_program):
    """2,000 seeded values of 12 triplets: any bits, all-good UMIs, and good UMIs with one bad triplet
    (0, 5, 6 or 7) at the first, a middle or the last position."""
    rng = random.Random(20)
    nw, L = 737280, 12
    good = lambda: sum(rng.choice((1, 2, 3, 4)) << (3 * p) for p in range(L))  # noqa: E731
    cases = []
    for k in range(2000):
        index = rng.randrange(nw)
        if k % 4 == 0:
            umi = rng.getrandbits(36 + (k // 4) % 2)
        elif k % 4 == 1:
            umi = good()
        else:
            p = (L - 1, L // 2, 0)[(k // 4) % 3]  # first base = the high triplet
            umi = (good() & ~(7 << (3 * p))) | (rng.choice((0, 5, 6, 7)) << (3 * p))
        cases.append((nw, 3, L, index, umi))
    flags = [R.umi_is_bad(c[4], 3, L) for c in cases]
    assert 500 <= sum(not f for f in flags) <= 600  # the all-good quarter, and hardly any random one
    _run(check_program, cases)


def test_the_63_bit_corner_and_illegal_counters(check_program):
    """TwoBit, L = 24, nw = 2^15: keys use all 63 bits.  And what create rejects."""
    nw, L = 2 ** 15, 24
    top = 2 ** 48 - 1
    cases = [(nw, 2, L, 32767, top), (nw, 2, L, 0, 0), (nw, 2, L, 5, 2 ** 48), (nw, 2, L, 32767, 2 ** 48 - 2),
             (nw, 2, L, 32766, top), (nw, 2, L, 1, 2 ** 47), (1, 2, 31, 0, 2 ** 62 - 1), (1, 2, 31, 0, 2 ** 62),
             (1, 3, 21, 0, 2 ** 63), (2, 3, 20, 1, int("4" * 20, 8))]
    assert _expected(*cases[0])[3] == 2 ** 63 - 1 and _expected(*cases[1])[3] == 0 and _expected(*cases[2])[2] == 1
    cases += [(0, 3, 10, 0, 0), (2 ** 31, 2, 4, 0, 0), (10, 4, 4, 0, 0), (10, 3, 0, 0, 0), (2 ** 16, 2, 24, 0, 0),
              (2 ** 15 + 1, 2, 24, 0, 0), (2 ** 31 - 1, 2, 16, 2 ** 31 - 2, 2 ** 32 - 1), (10, 2, 40, 0, 0)]
    _run(check_program, cases)
