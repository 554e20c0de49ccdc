"""CPU: the vectorised encode reference (tests/encode_reference.py) against the oracle's
per-record functions, against the oracle's random draws for ambiguous bytes, and against the
golden encode records; and the input generator's promises."""

import random

import numpy as np
import pytest

import encode_reference as R
from oracle import oracle as O

LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 21, 22, 28, 31, 32, 33, 43, 64, 100]


def test_tables_restate_the_oracle_maps():
    for b in range(256):
        assert R.V2[b] == O._TWO.get(b, 0)
        assert R.F2[b] == (0 if b in O._TWO else 1 if b in O._AMBIG else 2)
        assert R.V3[b] == O._THREE.get(b, 6)
    assert set(R.IUPAC.tolist()) == O._AMBIG and len(R.IUPAC) == 22
    assert len(R.GARBAGE) == 256 - 8 - 22


@pytest.mark.parametrize("L", LENGTHS)
def test_clean_records_equal_the_oracle(L):
    rng = np.random.default_rng(L)
    recs = R.BASES[rng.integers(0, 8, (300, L))]
    c2, g2, f2 = R.encode(2, recs)
    assert c2.shape == (300, R.words_for(2, L)) and not f2.any()
    want = [O.two_bit_encode(r.tobytes()) for r in recs]
    assert R.ints(c2) == want
    assert g2.tolist() == [O.two_bit_gc(w, L) for w in want]
    # ThreeBit: any byte is a valid input (every other byte reads as N)
    recs3 = np.where(rng.random(recs.shape) < 0.2, rng.integers(0, 256, recs.shape, dtype=np.uint8), recs)
    for batch in (recs, recs3):
        c3, g3, f3 = R.encode(3, batch)
        assert c3.shape == (300, R.words_for(3, L)) and not f3.any()
        want = [O.three_bit_encode(r.tobytes()) for r in batch]
        assert R.ints(c3) == want
        assert g3.tolist() == [O.three_bit_gc(w) for w in want]


@pytest.mark.parametrize("L", [1, 4, 15, 16, 32, 33, 64, 100])
def test_ambiguous_records_with_the_oracle_draws(L):
    """The helper leaves 0 where a byte is ambiguous: OR-ing the reference's draws (one
    random.randint(0, 3) per ambiguous byte, records in order, left to right) into its code gives
    oracle.two_bit_encode under the same seed."""
    rng = np.random.default_rng(100 + L)
    recs = R.BASES[rng.integers(0, 8, (200, L))]
    amb = rng.random(recs.shape) < 0.15
    recs[amb] = R.IUPAC[rng.integers(0, len(R.IUPAC), int(amb.sum()))]
    codes, gc, flags = R.encode(2, recs)
    assert flags.tolist() == [1 if a else 0 for a in amb.any(axis=1)]
    random.seed(7 + L)
    want = [O.two_bit_encode(r.tobytes()) for r in recs]
    state = random.getstate()
    random.seed(7 + L)
    got = R.ints(codes)
    for r in range(len(recs)):
        for p in range(L):
            if int(recs[r, p]) in O._AMBIG:
                got[r] |= random.randint(0, 3) << (2 * (L - 1 - p))
    assert got == want
    assert random.getstate() == state


def test_flags_agree_with_the_golden_records(golden):
    seen = set()
    for rec in golden["encode"]:
        seq = np.frombuffer(bytes.fromhex(rec["seq"]), np.uint8).reshape(1, -1)
        L = seq.shape[1]
        if L == 0:
            continue
        codes, gc, flags = R.encode(rec["enc"], seq)
        if "error" in rec:
            assert rec["enc"] == 2 and rec["error"]["type"] == "KeyError"
            assert flags[0] & 2
            first = next(b for b in seq[0].tolist() if R.F2[b] == 2)
            assert rec["error"]["args"] == ["%s is not a valid IUPAC nucleotide code" % chr(first)]
        elif rec["enc"] == 3:
            assert flags[0] == 0 and R.ints(codes) == [int(rec["code"])]
        else:
            assert not flags[0] & 2
            if flags[0] == 0:
                assert R.ints(codes) == [int(rec["code"])]
                assert gc[0] == O.two_bit_gc(int(rec["code"]), L)
            else:  # ambiguous: the golden code holds the reference's draws where the helper has 0
                amb = sum(3 << (2 * (L - 1 - p)) for p in range(L) if int(seq[0, p]) in O._AMBIG)
                assert int(rec["code"]) & ~amb == R.ints(codes)[0]
        seen.add((rec["enc"], int(flags[0])))
    # the ambiguous cases: lists of records encoded in order under a seed
    for case in golden["encode_ambiguous"]:
        for k, s in enumerate(case["seqs"]):
            seq = np.frombuffer(bytes.fromhex(s), np.uint8).reshape(1, -1)
            L = seq.shape[1]
            if L == 0:
                continue
            codes, gc, flags = R.encode(2, seq)
            assert bool(flags[0] & 1) == any(b in O._AMBIG for b in seq[0].tolist())
            if k < len(case["codes"]):
                assert not flags[0] & 2
                amb = sum(3 << (2 * (L - 1 - p)) for p in range(L) if int(seq[0, p]) in O._AMBIG)
                assert int(case["codes"][k]) & ~amb == R.ints(codes)[0]
            elif k == len(case["codes"]):  # the record the reference raised on
                assert case["error"]["type"] == "KeyError" and flags[0] & 2
            seen.add((2, int(flags[0])))
    assert {(2, 0), (2, 1), (2, 2), (3, 0)} <= seen


def test_encode_var_gathers_by_length():
    rng = np.random.default_rng(5)
    buf = rng.integers(0, 256, 4096, dtype=np.uint8)
    lens = rng.integers(0, 22, 500)
    starts = rng.integers(0, 4096 - 22, 500)
    for kind in (2, 3):
        codes, gc, flags = R.encode_var(kind, buf, starts, lens)
        for r in range(500):
            rec = buf[starts[r]:starts[r] + lens[r]].reshape(1, -1)
            c, g, f = R.encode(kind, rec) if lens[r] else (np.zeros((1, 1), np.uint64), [0], [0])
            assert (int(codes[r]), int(gc[r]), int(flags[r])) == (int(c[0, 0]), int(g[0]), int(f[0]))


@pytest.mark.parametrize("L", [1, 3, 4, 15, 16, 32])
def test_generator_covers_every_value_at_every_position(L):
    n = max(2 * 256 * L, 2048) + 1024 + 37
    recs = R.records(n, L, seed=L)
    seen = R.check_input(recs)
    assert seen.all()
    # the vectorised generator writes what the per-record statement says, on ACGTacgt elsewhere
    base = R.BASES[np.random.default_rng(L).integers(0, 8, (n, L))]
    for phase, got in ((0, recs), (12345, R.records(n, L, seed=L, phase=12345))):
        want = base.copy()
        for i in range(1, n, 2):  # every odd record
            for pos, val in R.substitutions(i, L, phase):
                want[i, pos] = val
        assert np.array_equal(got, want), phase
    assert np.isin(recs[0::2], R.BASES).all()
    changed = (recs[1::2] != base[1::2]).sum(axis=1)
    assert changed.max() <= 3


def test_generator_phase_moves_the_window():
    """Small batches: n // 2 consecutive (value, position) pairs from `phase` on, so batches with
    consecutive phases tile the table."""
    L, n = 16, 1000
    total = np.zeros((L, 256), bool)
    for k in range(9):
        recs = R.records(n, L, seed=k, phase=k * (n // 2))
        total |= R.check_input(recs, phase=k * (n // 2))
    assert total.all()  # 9 * 500 >= 256 * 16
    with pytest.raises(AssertionError):
        R.check_input(R.records(n, L, seed=0), full=True)
    with pytest.raises(AssertionError):  # uniform random bytes: no clean record
        R.check_input(np.random.default_rng(0).integers(0, 256, (4096, 16), dtype=np.uint8), full=False)
