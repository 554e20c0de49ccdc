"""CPU, nothing loaded into Python: tests/host/downsample_draw_check.cpp includes the downsampling's
draw header (sctools_amd/csrc/downsample_draw.h: stream, draw, thin, the tally keys, the bucket search
and the threshold check), is compiled by the host C++ compiler with AddressSanitizer and UBSan, runs
as a child process, and its answers are compared with tests/downsample_reference.py case by case."""

import os
import random
import shutil
import subprocess

import pytest

import downsample_reference as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = 2 ** 64 - 1
SEEDS = [0, 1, TOP]
KEYS = [0, 2 ** 63 - 1] + [D.tally_key(k) for k in range(4)]


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("dsdraw") / "downsample_draw_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, os.path.join(ROOT, "tests", "host", "downsample_draw_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, cases):
    """cases: tuples whose first element is the program's case letter.  Returns the answers as lists
    of ints, one per case."""
    text = "".join(" ".join(str(x) for x in c) + "\n" for c in cases)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True, timeout=120)
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok %d" % len(cases), lines[-1]
    return [[int(x) for x in line.split()] for line in lines[:-1]]


def test_draws_at_the_corners_of_seed_key_and_read_number(check_program):
    """Seeds 0, 1 and 2^64 - 1; keys 0, 2^63 - 1 and the four tally keys; j up to 2^64 - 2, where
    (j + 1) * G wraps, and j = 2^64 - 1, where j + 1 is 0."""
    js = [0, 1, 2, 63, 64, 2 ** 32 - 1, 2 ** 32, 2 ** 63, TOP - 1, TOP]
    cases = [("d", seed, key, j) for seed in SEEDS for key in KEYS for j in js]
    rng = random.Random(5)
    cases += [("d", rng.getrandbits(64), rng.getrandbits(63), rng.getrandbits(64)) for _ in range(2000)]
    got = _run(check_program, cases)
    for (_, seed, key, j), (stream, draw) in zip(cases, got):
        assert stream == D.stream(seed, key), (seed, key)
        assert draw == D.draw(seed, key, j) < 2 ** 32, (seed, key, j)


def test_thin_as_a_loop_and_as_strided_shares(check_program):
    """thin at T = 0, 1, mid values, 2^32 - 1 and 2^32 for molecules on both sides of 64 reads; the
    64 strided shares of the wave path sum to the same number."""
    thresholds = [0, 1, 2 ** 30, 429496730, 2 ** 31, 2 ** 32 - 1, 2 ** 32]
    reads = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1000]
    cases = [("t", seed, key, r, T) for seed in SEEDS for key in KEYS[:3] for r in reads for T in thresholds]
    got = _run(check_program, cases)
    for (_, seed, key, r, T), (loop, shares) in zip(cases, got):
        assert loop == shares == D.thin(seed, key, r, T), (seed, key, r, T)
        if T == 0:
            assert loop == 0
        if T == 2 ** 32:
            assert loop == r


def test_tally_keys_and_their_thinning(check_program):
    cases = [("y", seed, k, n, T) for seed in SEEDS for k in range(4) for n in (0, 1, 77, 500)
             for T in (0, 2 ** 31, 2 ** 32)]
    got = _run(check_program, cases)
    for (_, seed, k, n, T), (key, kept) in zip(cases, got):
        assert key == D.tally_key(k) == 2 ** 63 + k
        assert kept == D.thin_tally(seed, k, n, T), (seed, k, n, T)


def test_bucket_search_and_threshold_check(check_program):
    """k = 1 and k = 64, repeated thresholds, thresholds 0 and 2^32, every draw at and beside a
    threshold; and the sets the check must refuse."""
    rng = random.Random(11)
    sets = [[0], [1], [2 ** 32], [2 ** 31], [0, 0], [2 ** 32, 2 ** 32], [0, 2 ** 32], [0, 5, 5, 5, 9, 2 ** 32],
            sorted(rng.randrange(2 ** 32 + 1) for _ in range(64)), [7] * 64, list(range(64)),
            [0] * 10 + sorted(rng.randrange(2 ** 32) for _ in range(44)) + [2 ** 32] * 10,
            sorted(rng.randrange(100) for _ in range(17)), sorted(rng.randrange(2 ** 32 + 1) for _ in range(63))]
    assert {len(s) for s in sets} >= {1, 64}
    cases = []
    for th in sets:
        beside = {0, 2 ** 32 - 1}
        for t in th:
            beside.update(d for d in (t - 1, t, t + 1) if 0 <= d < 2 ** 32)
        cases += [("b", d, len(th), *th) for d in sorted(beside)]
    got = _run(check_program, cases)
    for (_, d, k, *th), (at, ok) in zip(cases, got):
        assert ok == 1 and D.thresholds_ok(th)
        assert at == D.bucket(d, th), (d, th)
    bad = [[], [2 ** 32 + 1], [5, 4], [0, 2 ** 32, 2 ** 32 - 1], list(range(65)), [1, 2, 2 ** 33]]
    got = _run(check_program, [("b", 0, len(th), *th) for th in bad])
    for th, (at, ok) in zip(bad, got):
        assert ok == 0 and at == -1 and not D.thresholds_ok(th), th
