"""CPU: the brute-force reference of posterior correction (tests/posterior_reference.py) on
hand-worked cases, the default quality weights, and the argument checks of the Python layer that
need no device."""

import numpy as np
import pytest

import posterior_reference as R
from sctools_amd import barcode

FLAT = [1] * 256  # every quality weighs the same


def run(kind, wl, queries, prior, num, den, quals=None, qweight=FLAT):
    L = len(wl[0])
    codes = [R.encode(kind, w) for w in wl]
    qs = [R.encode(kind, q) for q in queries]
    quals = quals or [[40] * L] * len(qs)
    return R.correct(kind, L, codes, qs, quals, prior, qweight, num, den)


@pytest.mark.parametrize("kind", [2, 3])
def test_threshold_is_inclusive(kind):
    wl = ["ACGT", "ACGA", "TTTT"]
    # ACGC is one base from the first two; priors 3 and 1: 3/4 of the total, exactly the bound
    assert run(kind, wl, ["ACGC"], [3, 1, 5], 3, 4) == ([0], [1])
    assert run(kind, wl, ["ACGC"], [3, 1, 5], 4, 5) == ([-2], [1])
    assert run(kind, wl, ["ACGC"], [2, 1, 5], 3, 4) == ([-2], [1])
    assert run(kind, wl, ["ACGC"], [1, 3, 5], 3, 4) == ([1], [1])


@pytest.mark.parametrize("kind", [2, 3])
def test_zero_prior_is_no_candidate(kind):
    wl = ["ACGT", "TTTT"]
    assert run(kind, wl, ["ACGA"], [0, 7], 39, 40) == ([-1], [255])
    assert run(kind, wl, ["ACGA"], [1, 7], 39, 40) == ([0], [1])  # a single candidate always passes
    assert run(kind, wl + ["ACGC"], ["ACGA"], [0, 7, 2], 39, 40) == ([2], [1])
    assert run(kind, wl, ["ACGA"], None, 39, 40) == ([0], [1])


@pytest.mark.parametrize("kind", [2, 3])
def test_exact_matches_ignore_priors(kind):
    wl = ["ACGT", "ACGT", "ACGA"]
    assert run(kind, wl, ["ACGT", "ACGA"], [0, 0, 0], 39, 40) == ([-2, 2], [0, 0])


def test_quality_picks_the_likelier_error():
    wl = ["AAAA", "CCAA", "TTTT"]
    # CAAA: base 0 wrong (-> AAAA) or base 1 wrong (-> CCAA); row byte b belongs to base b
    w = R.phred_weights()
    low0 = [[33 + 2, 33 + 30, 70, 70]]  # base 0 is the doubtful one
    low1 = [[33 + 30, 33 + 2, 70, 70]]
    for kind in (2, 3):
        assert run(kind, wl, ["CAAA"], None, 39, 40, low0, w) == ([0], [1])
        assert run(kind, wl, ["CAAA"], None, 39, 40, low1, w) == ([1], [1])
        assert run(kind, wl, ["CAAA"], None, 39, 40, [[50, 50, 70, 70]], w) == ([-2], [1])


def test_n_and_invalid_triplets():
    wl = ["ACGT", "CCGT", "ACGA"]
    # one N: both codes that agree elsewhere are candidates, whatever base they hold there
    assert run(3, wl, ["NCGT"], [3, 1, 9], 3, 4) == ([0], [1])
    assert run(3, wl, ["NCGT"], [1, 1, 9], 3, 4) == ([-2], [1])
    assert run(3, wl, ["NCGN"], [1, 1, 9], 3, 4) == ([-1], [255])  # two N: nothing within 1
    for bad in "057":
        assert run(3, wl, [bad + "CGT"], [3, 1, 9], 3, 4) == ([0], [1])
        assert run(3, wl, ["ACG" + bad], [2, 9, 3], 3, 4) == ([-2], [1])


def test_bits_above_the_barcode():
    codes = [R.encode(2, "ACGT")]
    q = [codes[0] | (1 << 8), codes[0]]
    assert R.correct(2, 4, codes, q, [[40] * 4] * 2, None, FLAT, 39, 40) == ([-1, 0], [255, 0])


def test_default_weights():
    w = R.phred_weights()
    assert (w[33], w[43], w[53], w[63]) == (1048576, 104858, 10486, 1049)
    assert set(w[66:]) == {526} and set(w[:34]) == {1048576}
    got = barcode.phred_weights()
    assert got.dtype == np.uint32 and got.tolist() == w
    assert barcode.phred_weights(offset=64, cap=40).tolist() == R.phred_weights(64, 40)


def test_barcode_length_rejects_longer_codes():
    with pytest.raises(ValueError, match="barcode_length"):
        barcode.WhitelistCorrector([R.encode(2, "CCGTA")], encoding="TwoBit", barcode_length=4)
    with pytest.raises(ValueError, match="2\\*\\*30"):
        barcode.PriorBarcodeSet({1: 1 << 30, 2: 1}, 4).corrector()
