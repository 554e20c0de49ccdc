"""CPU: tests/molecules_reference.py, the molecule counter's contract in plain Python, pinned on a
case worked by hand.  nw = 3, ThreeBit UMIs of 2 bases (C 1, A 2, G 3, T 4, N 6, first base in the
high triplet): AC = 17, CA = 10, TT = 36, AN = 22; 64 has a bit above the UMI and 5 = 0o05 a zero
leading triplet (and an invalid 5)."""

import math

import pytest

import molecules_reference as R

READS = [(0, 17), (0, 17), (1, 17), (0, 10), (-1, 17), (-2, 36), (2, 22), (1, 36), (1, 17), (2, 64), (2, 5)]


def _fed(reads):
    return R.Molecules(3, 3, 2).update([i for i, _ in reads], [u for _, u in reads])


def test_hand_worked_case():
    m = _fed(READS)
    reads, molecules, n_none, n_ambiguous, n_bad = m.counts()
    assert reads == [3, 3, 0]
    assert molecules == [2, 2, 0]
    assert (n_none, n_ambiguous, n_bad) == (1, 1, 3)
    assert m.pairs() == [(0, 10), (0, 17), (1, 17), (1, 36)]
    assert m.saturation() == 1 - 4 / 6
    assert m.total == len(READS)


def test_codes_of_the_case():
    code = {"C": 1, "A": 2, "G": 3, "T": 4, "N": 6}
    enc = lambda s: code[s[0]] * 8 + code[s[1]]  # noqa: E731
    assert (enc("AC"), enc("CA"), enc("TT"), enc("AN")) == (17, 10, 36, 22)
    assert [R.umi_is_bad(u, 3, 2) for u in (17, 10, 36, 22, 64, 5)] == [False, False, False, True, True, True]
    assert not R.umi_is_bad(5, 2, 2) and R.umi_is_bad(16, 2, 2)  # TwoBit: only the high bits are bad
    assert R.key(1, 36, 3, 2) == (1 << 6) | 36


@pytest.mark.parametrize("bad", [3, -3])
def test_out_of_range_index_raises_and_the_rest_is_counted(bad):
    m = R.Molecules(3, 3, 2)
    with pytest.raises(ValueError):
        m.update([i for i, _ in READS[:4]] + [bad] + [i for i, _ in READS[4:]],
                 [u for _, u in READS[:4]] + [17] + [u for _, u in READS[4:]])
    assert m.counts() == _fed(READS).counts()
    assert m.pairs() == _fed(READS).pairs()
    assert m.total == len(READS) + 1
    m.update([2], [17])  # and it goes on counting
    assert m.counts()[:2] == ([3, 3, 1], [2, 2, 1])


def test_empty_and_parameters():
    m = R.Molecules(1, 2, 31)  # idx_bits 1 + 62
    assert math.isnan(m.saturation()) and m.pairs() == [] and m.counts() == ([0], [0], 0, 0, 0)
    assert R.check_params(2 ** 15, 2, 24) == 48  # 15 + 48 = 63
    for nw, kind, L in [(0, 3, 10), (2 ** 31, 2, 4), (10, 4, 4), (10, 3, 0), (2 ** 16, 2, 24), (2 ** 15 + 1, 2, 24)]:
        with pytest.raises(ValueError):
            R.check_params(nw, kind, L)
