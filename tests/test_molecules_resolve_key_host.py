"""CPU, nothing loaded into Python: tests/host/molecules_resolve_key_check.cpp includes the resolve
pass's pure functions (sctools_amd/csrc/molecules_resolve_key.h), is compiled by the host C++ compiler
with AddressSanitizer and UBSan, and its answers are held against tests/feature_resolve_reference.py
(include/sctools_hip.h, "resolving features"): the re-packed sort word at the extremes of every part,
its order, the two head tests and the group fold at every split point."""

import itertools
import os
import shutil
import subprocess

import pytest

import count_matrix_reference as M
import feature_resolve_reference as F
import molecules_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("molrkey") / "molecules_resolve_key_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, os.path.join(ROOT, "tests", "host", "molecules_resolve_key_check.cpp"), "-o", exe],
                   check=True)
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), check=True, capture_output=True, text=True,
                         timeout=120)
    got = out.stdout.splitlines()
    assert got[-1] == "ok %d" % len(lines), (got[-1], out.stderr)
    return got[:-1]


def word(index, feature, image, nf, kind, L):
    """The contract's sort word: (((index << umi_bits) | image) << feat_bits) | feature."""
    return (((index << (kind * L)) | image) << M.feat_bits(nf)) | feature


# (nw, nf, kind, L); the fifth, sixth and seventh fill all 63 bits
COUNTERS = [(3, 2, 3, 2), (2 ** 31 - 1, 2, 2, 15), (2, 2 ** 31 - 1, 2, 15), (737280, 8192, 3, 10),
            (2 ** 20, 2 ** 13, 3, 10), (4, 2, 2, 30), (2, 4, 2, 30), (5, 3, 2, 4), (1, 1, 2, 30), (1, 1, 3, 1)]


def _extremes(nw, nf, kind, L):
    top = (1 << (kind * L)) - 1 if kind == 2 else int("100" * L, 2)  # T...T is ThreeBit's largest good code
    low = 0 if kind == 2 else int("001" * L, 2)
    return [(i, f, u) for i in (0, nw - 1) for f in (0, nf - 1) for u in (low, top)]


def test_word_round_trip_at_the_extremes(check_program):
    cases = [c + part for c in COUNTERS for part in _extremes(*c)]
    got = _run(check_program, ["word %d %d %d %d %d %d %d" % c for c in cases])
    widths = set()
    for (nw, nf, kind, L, i, f, u), line in zip(cases, got):
        w, gi, gf, gu = (int(x) for x in line.split())
        assert w == word(i, f, u, nf, kind, L) and w < 2 ** 63, (nw, nf, kind, L, i, f, u)
        assert (gi, gf, gu) == (i, f, u)
        # the key's own three parts in another order: as wide as the key
        assert w.bit_length() <= R.idx_bits(nw) + M.feat_bits(nf) + kind * L
        widths.add(w.bit_length())
    assert 63 in widths  # a word that fills all 63 bits is among them


def test_word_of_a_key_and_its_image(check_program):
    cases = []
    for c in COUNTERS:
        parts = _extremes(*c)
        cases += [c + (i, f, u, parts[-1 - k][2]) for k, (i, f, u) in enumerate(parts)]
    got = _run(check_program, ["of %d %d %d %d %d %d %d %d" % c for c in cases])
    for (nw, nf, kind, L, i, f, u, image), line in zip(cases, got):
        assert [int(x) for x in line.split()] == [word(i, f, image, nf, kind, L), i, f, image]


def test_ascending_word_order_is_index_image_feature_order():
    for nw, nf, kind, L in COUNTERS:
        parts = sorted(set((i, u, f) for i, f, u in _extremes(nw, nf, kind, L)))
        words = [word(i, f, u, nf, kind, L) for i, u, f in parts]
        assert words == sorted(words) and len(set(words)) == len(words)


def test_heads(check_program):
    nw, nf, kind, L = 737280, 8192, 3, 10
    fb = M.feat_bits(nf)
    w = lambda i, f, u: word(i, f, u, nf, kind, L)  # noqa: E731
    lo, hi = int("001" * L, 2), int("100" * L, 2)
    # (word, previous word, opens a group, opens a collapsed molecule)
    cases = [(w(5, 7, lo), w(5, 7, lo), 0, 0), (w(5, 8, lo), w(5, 7, lo), 0, 1), (w(5, 0, hi), w(5, nf - 1, lo), 1, 1),
             (w(6, 7, lo), w(5, 7, lo), 1, 1), (w(6, 0, lo), w(5, nf - 1, hi), 1, 1), (w(0, 0, lo), w(0, 0, lo), 0, 0),
             (w(nw - 1, nf - 1, hi), w(nw - 1, nf - 2, hi), 0, 1), (w(nw - 1, 0, hi), w(nw - 1, 0, lo), 1, 1),
             (w(0, 1, lo), w(0, 0, lo), 0, 1), (2 ** 64 - 1, w(nw - 1, nf - 1, hi), 1, 1)]
    got = _run(check_program, ["heads %d %d %d" % (fb, a, b) for a, b, _, _ in cases])
    assert [tuple(int(x) for x in g.split()) for g in got] == [(g, m) for _, _, g, m in cases]
    # a 63-bit word, and the word past the last row against it
    top = word(2 ** 20 - 1, 8191, hi, 8192, 3, 10)
    assert top.bit_length() == 63
    got = _run(check_program, ["heads 13 %d %d" % (top, top - 1), "heads 13 %d %d" % (2 ** 64 - 1, top),
                               "heads 13 %d %d" % (top, word(2 ** 20 - 1, 8191, hi - 1, 8192, 3, 10))])
    assert got == ["0 1", "1 1", "1 1"]


def _want(reads):
    top, at_top, members, total = F.fold(reads)
    return "%d %d %d %d %d" % (top, at_top, members, total, at_top == 1)


def test_fold_is_the_reference_rule_at_every_split(check_program):
    lists = [[], [4], [5, 3, 3], [3, 3, 1], [2, 2, 2, 1], [1, 1], [2 ** 62, 2 ** 62, 1], [2 ** 63 - 1, 2 ** 63]]
    # every 6-member list over three values: every pattern of ties, and the top at every position
    lists += [list(p) for p in itertools.product((1, 2, 3), repeat=6)]
    lines, want = [], []
    for r in lists:
        text = " ".join(str(x) for x in r)
        lines.append(("fold %d %s" % (len(r), text)).strip())
        want.append(_want(r))
        for k in range(len(r) + 1):  # associativity: any cut of the list folds to the same
            lines.append(("split %d %d %s" % (len(r), k, text)).strip())
            want.append(_want(r))
    assert _run(check_program, lines) == want
    assert _want([5, 3, 3]).endswith(" 1") and _want([3, 3, 1]).endswith(" 0") and _want([]).endswith(" 0")
