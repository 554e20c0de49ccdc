"""CPU, nothing loaded into Python: tests/host/swapped_keep_check.cpp includes the swapped-molecule
removal's judgement header (sctools_amd/csrc/swapped_keep.h: the saturating add, the exact comparison
of two 96-bit products and the parameter check), is compiled by the host C++ compiler with
AddressSanitizer and UBSan, runs as a child process, and its answers are compared with
tests/swapped_reference.py case by case."""

import os
import random
import shutil
import subprocess

import pytest

import swapped_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 2 ** 64 - 1
READS = [0, 1, 2 ** 32 - 1, 2 ** 32 + 1, 2 ** 63, TOP]
FRACTIONS = [(1, 1), (4, 5), (2, 3), (2 ** 31 + 1, 2 ** 32), (2 ** 32, 2 ** 32)]


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("swapped") / "swapped_keep_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, os.path.join(ROOT, "tests", "host", "swapped_keep_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, cases):
    """cases: tuples whose first element is the program's case letter.  Returns one int per case."""
    text = "".join(" ".join(str(x) for x in c) + "\n" for c in cases)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True, timeout=120)
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok %d" % len(cases), lines[-1]
    return [int(line) for line in lines[:-1]]


def test_keeps_at_the_corners_and_at_random(check_program):
    """r and others at 0, 1, 2^32 - 1, 2^32 + 1, 2^63 and 2^64 - 1 under every fraction: the products
    reach 2^96, which a 64-bit multiply would wrap; then 2,000 random cases whose operands are drawn
    at every width."""
    cases = [("k", r, o, num, den) for r in READS for o in READS for num, den in FRACTIONS]
    rng = random.Random(7)
    for _ in range(2000):
        num, den = rng.choice(FRACTIONS) if rng.random() < 0.5 else (0, 0)
        while not S.params_ok(1, num, den):
            den = rng.randrange(1, 2 ** rng.randrange(1, 33) + 1)
            num = rng.randrange(den // 2 + 1, den + 1)
        r = rng.getrandbits(rng.randrange(1, 65))
        # near the boundary r * (den - num) == num * others as often as far from it
        o = rng.getrandbits(rng.randrange(1, 65))
        if rng.random() < 0.5 and den > num:
            o = min(TOP, max(0, r * (den - num) // num + rng.randrange(-1, 2)))
        cases.append(("k", r, o, num, den))
    got = _run(check_program, cases)
    assert len({c[1:] for c in cases if S.keeps(*c[1:])}) > 500 < len({c[1:] for c in cases if not S.keeps(*c[1:])})
    for (_, r, o, num, den), kept in zip(cases, got):
        assert kept == int(S.keeps(r, o, num, den)), (r, o, num, den)
        if o == 0:
            assert kept == 1
        if num == den and o > 0:
            assert kept == 0


def test_equality_is_kept(check_program):
    """4 of 5 reads at 4/5 keeps, 3 of 4 does not; the same at the largest denominators and reads."""
    cases = [("k", 4, 1, 4, 5), ("k", 3, 1, 4, 5), ("k", 2, 1, 2, 3), ("k", 1, 1, 2, 3),
             ("k", 4 * 2 ** 60, 2 ** 60, 4, 5), ("k", 4 * 2 ** 60 - 1, 2 ** 60, 4, 5),
             ("k", 2 ** 31 + 1, 2 ** 31 - 1, 2 ** 31 + 1, 2 ** 32), ("k", 2 ** 31, 2 ** 31 - 1, 2 ** 31 + 1, 2 ** 32),
             ("k", TOP, 0, 2 ** 32, 2 ** 32), ("k", TOP, 1, 2 ** 32, 2 ** 32), ("k", TOP, TOP, 2 ** 31 + 1, 2 ** 32)]
    assert _run(check_program, cases) == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0]
    assert [int(S.keeps(*c[1:])) for c in cases] == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0]


def test_the_sum_saturates(check_program):
    values = [0, 1, 2 ** 32, 2 ** 63 - 1, 2 ** 63, TOP - 1, TOP]
    cases = [("a", x, y) for x in values for y in values]
    got = _run(check_program, cases)
    for (_, x, y), total in zip(cases, got):
        assert total == S.add_sat(x, y) == min(x + y, TOP), (x, y)
    assert _run(check_program, [("a", TOP, 1), ("a", 2 ** 63, 2 ** 63), ("a", TOP - 1, 1)]) == [TOP, TOP, TOP]


def test_params_on_both_sides_of_every_bound(check_program):
    """s in [1, 16]; 1 <= num <= den <= 2^32; 2 * num > den, with 2 * num == den refused."""
    good = [(1, 1, 1), (16, 4, 5), (2, 2, 3), (3, 2 ** 32, 2 ** 32), (2, 2 ** 31 + 1, 2 ** 32), (2, 3, 5), (1, 2, 3)]
    bad = [(0, 4, 5), (17, 4, 5), (-1, 4, 5), (2, 0, 1), (2, 0, 0), (2, 5, 4), (2, 2 ** 32 + 1, 2 ** 32 + 1),
           (2, 2 ** 32, 2 ** 32 + 1), (2, 1, 2), (2, 2 ** 31, 2 ** 32), (2, 2, 4), (2, 2, 5), (2, 2 ** 63, TOP),
           (2, TOP, TOP)]
    assert _run(check_program, [("p",) + c for c in good]) == [1] * len(good)
    assert _run(check_program, [("p",) + c for c in bad]) == [0] * len(bad)
    assert all(S.params_ok(*c) for c in good) and not any(S.params_ok(*c) for c in bad)


def test_at_most_one_sample_keeps(check_program):
    """For random reads r_0 .. r_{s-1} >= 1 of one molecule, small and near 2^64 where the sum of the
    others saturates, at most one sample keeps it under every legal fraction -- a property of
    2 * num > den that the contract states and does not assume."""
    rng = random.Random(13)
    cases = []
    for _ in range(1500):
        s = rng.randrange(1, 17)
        num, den = rng.choice(FRACTIONS[1:4] + [(3, 5), (51, 100), (2 ** 31 + 1, 2 ** 32 - 1)])
        style = rng.randrange(3)
        if style == 0:  # one dominant sample
            r = [rng.randrange(1, 4) for _ in range(s)]
            r[rng.randrange(s)] = rng.randrange(1, 200)
        elif style == 1:
            r = [rng.randrange(1, 30) for _ in range(s)]
        else:
            r = [max(1, rng.getrandbits(rng.randrange(1, 65))) for _ in range(s)]
        cases.append(("m", s, num, den, *r))
    got = _run(check_program, cases)
    seen = set()
    for (_, s, num, den, *r), keepers in zip(cases, got):
        want = sum(S.keeps(r[k], S.others([_Reads(x) for x in r], k, "m"), num, den) for k in range(s))
        assert keepers == want <= 1, (s, num, den, r)
        seen.add(keepers if s > 1 else 2)
    assert seen == {0, 1, 2}  # nobody reaches the fraction, one sample does, and s = 1 (always kept)


class _Reads:
    """A sample that holds one molecule, "m", with r reads: what swapped_reference.others walks."""

    def __init__(self, r):
        self.mreads = {"m": r}
