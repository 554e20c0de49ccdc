"""CPU, nothing loaded into Python: tests/host/umi_neighbours_check.cpp includes the collapse's
neighbour header (sctools_amd/csrc/umi_neighbours.h: the j-th one-base neighbour of a code, the
(reads, code) order), is compiled by the host C++ compiler with AddressSanitizer and UBSan, and its
answers are compared with tests/umi_collapse_reference.py case by case."""

import os
import random
import shutil
import subprocess

import pytest

import molecules_reference as R
import umi_collapse_reference as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("uminb") / "umi_neighbours_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, os.path.join(ROOT, "tests", "host", "umi_neighbours_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, cases, umi_bits=None):
    """cases: (kind, L, code, a_reads, b_reads, b_code).  The program's neighbours, as a set and with
    none repeated, are the reference's; with umi_bits, `code` is a key whose bits from umi_bits up
    must come back unchanged in every neighbour."""
    text = "".join("%d %d %d %d %d %d\n" % c for c in cases)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True, timeout=120)
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok %d" % len(cases), lines[-1]
    for (kind, L, code, ra, rb, other), line in zip(cases, lines[:-1]):
        got = [int(x) for x in line.split()]
        nbs, less = got[:-1], got[-1]
        assert len(nbs) == 3 * L
        if umi_bits is None:
            want = U.neighbours(code, kind, L)
        else:
            high, umi = code >> umi_bits << umi_bits, code & (2 ** umi_bits - 1)
            want = [high | v for v in U.neighbours(umi, kind, L)]
        assert sorted(nbs) == sorted(want) and len(set(nbs)) == 3 * L, (kind, L, code)
        assert less == int(U.support_less(ra, code, rb, other)), (ra, code, rb, other)


def test_every_two_base_threebit_and_three_base_twobit_code(check_program):
    """The 16 good ThreeBit codes of 2 bases and all 64 TwoBit codes of 3, each against every other
    code of its kind in the order predicate with fewer, equal and more reads."""
    good3 = [u for u in range(64) if not R.umi_is_bad(u, 3, 2)]
    assert len(good3) == 16
    cases = [(3, 2, u, 5, rb, v) for u in good3 for v in good3 for rb in (4, 5, 6)]
    cases += [(2, 3, u, 5, rb, v) for u in range(64) for v in range(0, 64, 7) for rb in (4, 5, 6)]
    _run(check_program, cases)
    for u in good3:  # what the comparison stands on: never N, never invalid
        assert all(not R.umi_is_bad(v, 3, 2) for v in U.neighbours(u, 3, 2))


def test_random_twelve_base_threebit_codes(check_program):
    rng = random.Random(7)
    L = 12
    good = lambda: sum(rng.choice((1, 2, 3, 4)) << (3 * p) for p in range(L))  # noqa: E731
    cases = [(3, L, good(), rng.randrange(4), rng.randrange(4), good()) for _ in range(3000)]
    cases += [(3, L, int("1" * L, 8), 1, 1, int("4" * L, 8)), (3, L, int("4" * L, 8), 1, 1, int("1" * L, 8)),
              (3, L, int("4" * L, 8), 2 ** 64 - 1, 2 ** 64 - 1, int("4" * L, 8)),
              (3, L, int("4" * L, 8), 0, 2 ** 64 - 1, 0)]
    _run(check_program, cases)


def test_the_63_bit_corner_keeps_its_index_bits(check_program):
    """TwoBit, L = 24, nw = 2^15: the key of index 32767 and UMI 2^48 - 1 is 2^63 - 1.  A neighbour of
    the top digit (3 -> 0, 1, 2) must not carry into the index bits, nor one of digit 0 borrow."""
    L, index = 24, 32767
    keys = [R.key(index, u, 2, L) for u in (2 ** 48 - 1, 0, 2 ** 47, 1 << 46, 0xABCDEF012345)]
    keys += [R.key(i, 2 ** 48 - 1, 2, L) for i in (0, 1, 16384)]
    assert keys[0] == 2 ** 63 - 1
    _run(check_program, [(2, L, k, 1, 1, k ^ 1) for k in keys], umi_bits=48)
    # and as plain UMIs, at the widest legal lengths of both kinds
    _run(check_program, [(2, 31, 2 ** 62 - 1, 0, 0, 0), (2, 31, 0, 0, 0, 0), (3, 20, int("4" * 20, 8), 0, 0, 0),
                         (3, 20, int("1" * 20, 8), 0, 0, 0)])
