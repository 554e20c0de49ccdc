"""CPU, nothing loaded into Python: tests/host/molecules_feature_key_check.cpp includes the feature
counter's key header (sctools_amd/csrc/molecules_feature_key.h), is compiled by the host C++ compiler
with AddressSanitizer and UBSan, and its answers are held against tests/count_matrix_reference.py
(include/sctools_hip.h, "counting molecules per feature"): the width of a feature, which
(nw, nf, kind, L) are legal, the key packed and taken apart at the extremes of every part, and the
test that opens a matrix entry."""

import os
import shutil
import subprocess

import pytest

import count_matrix_reference as M
import molecules_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("molfkey") / "molecules_feature_key_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, os.path.join(ROOT, "tests", "host", "molecules_feature_key_check.cpp"), "-o", exe],
                   check=True)
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), check=True, capture_output=True, text=True,
                         timeout=120)
    got = out.stdout.splitlines()
    assert got[-1] == "ok %d" % len(lines), (got[-1], out.stderr)
    return got[:-1]


def _legal(nw, nf, kind, L):
    try:
        return M.check_params(nw, nf, kind, L)
    except ValueError:
        return 0


def test_feat_bits(check_program):
    nfs = [1, 2, 3]
    for k in range(2, 31):
        nfs += [2 ** k - 1, 2 ** k, 2 ** k + 1]
    nfs.append(2 ** 31 - 1)
    got = _run(check_program, ["bits %d" % nf for nf in nfs])
    assert [int(g) for g in got] == [M.feat_bits(nf) for nf in nfs]
    by = dict(zip(nfs, (int(g) for g in got)))
    assert (by[1], by[2], by[3], by[4], by[5]) == (1, 1, 2, 2, 3)
    for k in range(2, 31):
        assert by[2 ** k] == k and by[2 ** k + 1] == k + 1


def test_legal_counters(check_program):
    cases = []
    # widths that sum to exactly 63 (legal) and to 64 (not), every split of the 63 - umi_bits bits
    for kind, L in ((3, 10), (2, 12), (2, 30), (3, 1), (2, 1), (3, 19)):
        rest = 63 - kind * L
        for ib in range(1, min(31, rest - 1) + 1):
            fb = rest - ib
            if not 1 <= fb <= 31:
                continue
            nw, nf = (2 ** ib if ib > 1 else 2), (2 ** fb if fb > 1 else 2)
            nw, nf = min(nw, 2 ** 31 - 1), min(nf, 2 ** 31 - 1)
            cases += [(nw, nf, kind, L), (nw, nf + 1, kind, L), (nw + 1, nf, kind, L)]
    # the header's two practical limits, and the bounds of nf
    cases += [(737280, 8192, 3, 10), (737280, 8193, 3, 10), (3_700_000, 2 ** 17, 2, 12),
              (3_700_000, 2 ** 17 + 1, 2, 12), (10, 0, 3, 4), (10, -1, 3, 4), (10, 1, 3, 4), (10, 2 ** 31 - 1, 2, 4),
              (10, 2 ** 31, 2, 4), (0, 4, 3, 4), (10, 4, 4, 4), (10, 4, 3, 0), (2, 2, 2, 31), (1, 1, 2, 30)]
    got = _run(check_program, ["legal %d %d %d %d" % c for c in cases])
    want = [_legal(*c) for c in cases]
    assert [int(g) for g in got] == want
    assert want[cases.index((737280, 8192, 3, 10))] == 30 and want[cases.index((737280, 8193, 3, 10))] == 0
    assert any(w for w in want) and not all(w for w in want)
    legal = [c for c, w in zip(cases, want) if w]
    assert any(R.idx_bits(c[0]) + M.feat_bits(c[1]) + c[2] * c[3] == 63 for c in legal)


def _extremes(nw, nf, kind, L):
    top = (1 << (kind * L)) - 1 if kind == 2 else int("100" * L, 2)  # T...T is ThreeBit's largest good code
    low = 0 if kind == 2 else int("001" * L, 2)
    return [(i, f, u) for i in (0, nw - 1) for f in (0, nf - 1) for u in (low, top)]


def test_pack_round_trip_at_the_extremes(check_program):
    counters = [(3, 2, 3, 2), (1, 1, 3, 1), (1, 1, 2, 30), (737280, 8192, 3, 10), (3_700_000, 2 ** 17, 2, 12),
                (2 ** 31 - 1, 2, 2, 15), (2, 2 ** 31 - 1, 2, 15), (5, 3, 2, 4)]
    cases = [c + part for c in counters for part in _extremes(*c)]
    got = _run(check_program, ["pack %d %d %d %d %d %d %d" % c for c in cases])
    for (nw, nf, kind, L, i, f, u), line in zip(cases, got):
        key, gi, gf, gu = (int(x) for x in line.split())
        assert key == M.key(i, f, u, nf, kind, L) and key < 2 ** 63, (nw, nf, kind, L, i, f, u)
        assert (gi, gf, gu) == (i, f, u) == M.unkey(key, nf, kind, L)
    # ascending key order is (index, feature, umi) order
    for c in counters:
        parts = _extremes(*c)
        keys = [M.key(i, f, u, c[1], c[2], c[3]) for i, f, u in sorted(set(parts))]
        assert keys == sorted(keys)


def test_head(check_program):
    nw, nf, kind, L = 737280, 8192, 3, 10
    k = lambda i, f, u: M.key(i, f, u, nf, kind, L)  # noqa: E731
    lo, hi = int("001" * L, 2), int("100" * L, 2)
    cases = [(k(5, 7, lo), k(5, 7, lo), 0), (k(5, 7, hi), k(5, 7, lo), 0), (k(5, 8, lo), k(5, 7, hi), 1),
             (k(6, 7, lo), k(5, 7, lo), 1), (k(6, 0, lo), k(5, nf - 1, hi), 1), (k(nw - 1, nf - 1, hi), k(nw - 1, nf - 1, lo), 0),
             (k(nw - 1, nf - 1, hi), k(nw - 1, nf - 2, hi), 1), (k(0, 0, lo), k(0, 0, lo), 0), (k(0, 1, lo), k(0, 0, lo), 1)]
    got = _run(check_program, ["head %d %d %d" % (kind * L, key, prev) for key, prev, _ in cases])
    assert [int(g) for g in got] == [w for _, _, w in cases]
