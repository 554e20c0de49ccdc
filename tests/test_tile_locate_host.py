"""CPU, nothing loaded into Python: tests/host/tile_locate_check.cpp includes the header with which
line_end_kernel finds the tile that holds a terminator (sctools_amd/csrc/tile_locate.h), is compiled by
the host C++ compiler with AddressSanitizer and UBSan, and its answers are held against a plain prefix
sum: the tile is the first whose inclusive prefix exceeds the target, `before` is that tile's exclusive
prefix, and a target at or past the total finds none.  The program forms the coarse levels as plain
sums over blocks of 32 and 1,024 tiles, in arrays of exactly their sizes."""

import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTILES = (1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3000)
EDGES = (32, 1024)  # a block of the middle level, a block of the top level


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("tilelocate") / "tile_locate_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, os.path.join(ROOT, "tests", "host", "tile_locate_check.cpp"), "-o", exe], check=True)
    return exe


def _targets(counts):
    """Every target below the total when that is at most 4,096, else every tile's first and last item;
    and the total and one past it, which no tile holds."""
    incl = np.cumsum(counts)
    total = int(incl[-1])
    if total <= 4096:
        some = list(range(total))
    else:
        has = counts > 0
        some = sorted(set((incl - counts)[has].tolist()) | set((incl - 1)[has].tolist()))
    return some + [total, total + 1]


def _run_and_check(exe, cases):
    """cases: int64 count arrays.  Runs them all in one process; every answer against the prefix sum."""
    targets = [_targets(c) for c in cases]
    text = "".join("%d %s %d %s\n" % (len(c), " ".join(map(str, c.tolist())), len(t), " ".join(map(str, t)))
                   for c, t in zip(cases, targets))
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True, timeout=120)
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok %d %d" % (len(cases), sum(len(t) for t in targets)), lines[-1]
    at = 0
    for c, ts in zip(cases, targets):
        incl = np.cumsum(c)
        total = int(incl[-1])
        got = np.array([ln.split() for ln in lines[at:at + len(ts)]], dtype=np.int64).reshape(len(ts), 2)
        at += len(ts)
        t = np.asarray(ts, dtype=np.int64)
        inside = t < total
        assert inside[:-2].all() and not inside[-2:].any()
        want_tile = np.searchsorted(incl, t[inside], side="right")  # the first inclusive prefix > target
        assert (c[want_tile] > 0).all()  # (a tile that holds an item is never an empty one)
        bad = np.flatnonzero((got[inside, 0] != want_tile) | (got[inside, 1] != (incl - c)[want_tile]))
        assert bad.size == 0, (len(c), "target %d: got %s, want tile %d before %d"
                               % (t[bad[0]], got[bad[0]].tolist(), want_tile[bad[0]], (incl - c)[want_tile[bad[0]]]))
        assert (got[~inside, 0] == -1).all(), (len(c), total, got[~inside].tolist())


def test_every_tile_holds_one(check_program):
    _run_and_check(check_program, [np.ones(n, dtype=np.int64) for n in NTILES])


def test_one_tile_holds_everything(check_program):
    """All counts 0 but one tile's: the first, the last, and the tiles on each side of a 32-block and a
    1,024-block edge -- whole empty blocks of both levels lie before and after it."""
    cases = []
    for n in NTILES:
        for pos in sorted({0, n - 1} | {e + d for e in EDGES for d in (-1, 0) if 0 <= e + d < n}):
            for cnt in (1, 5, 8192):
                c = np.zeros(n, dtype=np.int64)
                c[pos] = cnt
                cases.append(c)
    assert len(cases) > 150
    _run_and_check(check_program, cases)


def test_random_counts_with_empty_runs_across_the_block_edges(check_program):
    """Counts in 0..8192 (what an 8 KiB tile can hold), with runs of empty tiles laid across every
    32-block and 1,024-block edge the size has, and leading and trailing runs."""
    rng = np.random.default_rng(20260)
    cases = []
    for n in NTILES:
        for rep in range(4):
            c = rng.integers(0, 8193, size=n, dtype=np.int64)
            c[rng.random(n) < 0.2] = 0
            for e in EDGES:
                for edge in range(e, n, e):
                    if rng.random() < (0.25 if e == 32 else 1.0):
                        a, b = int(rng.integers(0, 2 * e + 2)), int(rng.integers(0, 2 * e + 2))
                        c[max(0, edge - a):min(n, edge + b)] = 0  # (one side, both, or more than a whole block)
            if rep & 1:
                c[:int(rng.integers(1, max(2, n // 3 + 1)))] = 0
            if rep & 2:
                c[n - int(rng.integers(1, max(2, n // 3 + 1))):] = 0
            if not c.any():
                c[int(rng.integers(0, n))] = int(rng.integers(1, 8193))
            cases.append(c)
    _run_and_check(check_program, cases)
