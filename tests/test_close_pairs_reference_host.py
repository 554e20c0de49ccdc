"""CPU: the numpy contract of the close-pairs pass (tests/close_pairs_reference.py) against the
reference's own distance, pair by pair (oracle.two_bit_hamming, encodings.py:113-121), and its
per-distance totals against the all-pairs histogram (oracle.allpairs_hist_numpy)."""

import numpy as np
import pytest

import close_pairs_reference as C
from oracle import oracle as O


def _sets():
    rng = np.random.default_rng(5)
    out = []
    # 1 base: four codes, everything is a duplicate or one base away
    out.append(("1 base", rng.integers(0, 4, size=60).astype(np.uint64), 2))
    # 4 bases: a dense multiset
    out.append(("4 bases", rng.integers(0, 256, size=300).astype(np.uint64), 8))
    # 16 bases: random codes, copies and neighbours 1..4 bases away
    base = rng.integers(0, 1 << 32, size=120).astype(np.uint64)
    near = []
    for k in range(1, 5):
        c = base[:30].copy()
        for p in rng.choice(16, size=k, replace=False):
            c ^= np.uint64(int(rng.integers(1, 4))) << np.uint64(2 * int(p))
        near.append(c)
    out.append(("16 bases", np.concatenate([base, base[:20]] + near), 32))
    # 32 bases, the top bit in use
    wide = rng.integers(0, 1 << 63, size=80).astype(np.uint64) | np.uint64(1 << 63)
    out.append(("32 bases", np.concatenate([wide, wide[:10] ^ np.uint64(3 << 62), wide[:10] ^ np.uint64(1)]), 64))
    out.append(("two codes", np.array([7, 7], dtype=np.uint64), 4))
    out.append(("one code", np.array([7], dtype=np.uint64), 4))
    out.append(("no code", np.zeros(0, dtype=np.uint64), 4))
    return out


@pytest.mark.parametrize("name,codes,bits", _sets(), ids=[s[0] for s in _sets()])
@pytest.mark.parametrize("max_d", [0, 1, 2, 3])
def test_contract_pair_by_pair(name, codes, bits, max_d):
    n = codes.size
    assert n <= 300
    want = [(i, j, O.two_bit_hamming(int(codes[i]), int(codes[j]))) for i in range(n) for j in range(i + 1, n)]
    want = [w for w in want if w[2] <= max_d]
    i, j, dist = C.close_pairs(codes, bits, max_d)
    assert i.dtype == np.int32 and j.dtype == np.int32 and dist.dtype == np.uint8
    assert list(zip(i.tolist(), j.tolist(), dist.tolist())) == want  # (and so ascending by (i, j))
    # per-distance totals = the headline histogram's first bins
    hist = O.allpairs_hist_numpy(codes)[:max_d + 1]
    assert np.bincount(dist, minlength=max_d + 1).tolist() == hist.tolist()
    # neighbour counts: both ends of every pair
    deg = C.neighbour_counts(codes, bits, max_d)
    assert deg.shape == (n, max_d + 1) and deg.dtype == np.int64
    ref = np.zeros((n, max_d + 1), dtype=np.int64)
    for a, b, d in want:
        ref[a, d] += 1
        ref[b, d] += 1
    assert np.array_equal(deg, ref)
    assert deg.sum(axis=0).tolist() == (2 * hist).tolist()


def test_duplicates_are_pairs_at_distance_zero():
    codes = np.array([5, 9, 5, 5, 9], dtype=np.uint64)
    i, j, dist = C.close_pairs(codes, 4, 0)
    assert list(zip(i.tolist(), j.tolist())) == [(0, 2), (0, 3), (1, 4), (2, 3)]
    assert dist.tolist() == [0, 0, 0, 0]
    assert C.neighbour_counts(codes, 4, 0)[:, 0].tolist() == [2, 1, 2, 2, 1]
