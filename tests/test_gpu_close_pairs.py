"""GPU: the close-pairs pass (sct_allpairs_close_pairs, Barcodes.close_pairs / neighbour_counts)
against its numpy contract (tests/close_pairs_reference.py), by exact integer equality.

The sizes sit on the kernel's seams: the 32-code group and the 64-code group pair, the 256-row
block, the column chunk (1024 codes up to 16 bases, 512 above), the diagonal and tail masks and the
work queue's 16-item pull (5000 codes at 16 bases are 60 items).  Random 15..32-base sets hold next
to no close pair, so copies with 0..4 substituted bases are planted across those seams, plus one
code with about 40 neighbours; the 1- and 4-base sets are dense multisets."""

import ctypes
import functools

import numpy as np
import pytest

import close_pairs_reference as C
from sctools_amd import _lib, barcode, synthetic

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 33, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 5000]
WIDTHS = [1, 4, 15, 16, 17, 32]
CANARY = 64


def _substitute(rng, code, L, s):
    """`code` with min(s, L) distinct bases replaced by other bases"""
    code = int(code)
    for p in rng.choice(L, size=min(s, L), replace=False):
        code ^= int(rng.integers(1, 4)) << (2 * int(p))
    return code


@functools.lru_cache(maxsize=None)
def make_set(n, L):
    """n codes of L bases; from 15 bases up with neighbours planted across the kernel's seams"""
    rng = np.random.default_rng(1000 * L + n)
    if L <= 4:
        return rng.integers(0, 4 ** L, size=n).astype(np.uint64)
    codes = [int(rng.integers(0, 1 << 62)) & (4 ** L - 1) | (int(rng.integers(0, 4)) << (2 * L - 2)) for _ in range(n)]
    if n < 2:
        return np.array(codes, dtype=np.uint64)
    seams = [(0, 1), (31, 32), (63, 64), (255, 256), (511, 512), (1023, 1024), (0, n - 1)]
    seams = [(a, b) for a, b in seams if b < n and a != b]
    used = {p for ab in seams for p in ab} | {n - 2, n - 1}
    free = [p for p in rng.permutation(n).tolist() if p not in used]
    for k, (a, b) in enumerate(seams):
        s = k % 4  # 0..3 bases apart, and a decoy one base further than that
        codes[b] = _substitute(rng, codes[a], L, s)
        if free:
            codes[free.pop()] = _substitute(rng, codes[a], L, s + 1)
    if n >= 3:
        codes[n - 2] = _substitute(rng, codes[n - 1], L, 1)
    if len(free) > 60:  # one code with about 40 neighbours, 0..4 bases away
        hub = free.pop()
        for k in range(40):
            codes[free.pop()] = _substitute(rng, codes[hub], L, k % 5)
    return np.array(codes, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def reference(n, L):
    """the contract at the largest threshold the set is run at; lower ones are its prefix in dist"""
    i, j, dist = C.close_pairs(make_set(n, L), 2 * L, min(3, L))
    for a in (i, j, dist):
        a.setflags(write=False)
    return i, j, dist


def expected(n, L, max_d):
    i, j, dist = reference(n, L)
    keep = dist <= max_d
    return i[keep], j[keep], dist[keep]


def degrees(n, max_d, i, j, dist):
    out = np.zeros((n, max_d + 1), dtype=np.int64)
    np.add.at(out, (i, dist), 1)
    np.add.at(out, (j, dist), 1)
    return out


class Device:
    """a SUBSETS plan over a set, and one close-pairs call into canary-guarded buffers"""

    def __init__(self, codes, L, scheme=_lib.SCHEME_SUBSETS):
        import torch
        self.torch = torch
        self.n = codes.size
        self.d_codes = torch.from_numpy(codes.view(np.int64).copy()).cuda()
        self.plan = _lib.AllPairsPlan(self.d_codes.data_ptr(), self.n, 2 * L, scheme=scheme)
        if scheme != _lib.SCHEME_SPECTRAL:  # (a refused call reads no table)
            self.plan.build()

    def run(self, max_d, room, begin=0, end=None):
        torch = self.torch
        d_i = torch.full((room + CANARY,), -7, dtype=torch.int32, device="cuda")
        d_j = torch.full((room + CANARY,), -7, dtype=torch.int32, device="cuda")
        d_dist = torch.full((room + CANARY,), 0xAB, dtype=torch.uint8, device="cuda")
        d_stats = torch.full((6 + 2,), -7, dtype=torch.int64, device="cuda")
        d_deg = torch.full((self.n * (max_d + 1) + CANARY,), -7, dtype=torch.int32, device="cuda")
        self.plan.close_pairs(max_d, d_stats.data_ptr(), d_i.data_ptr(), d_j.data_ptr(), d_dist.data_ptr(), room,
                              d_deg.data_ptr(), begin, end)
        torch.cuda.synchronize()
        i, j, dist, stats, deg = (t.cpu().numpy() for t in (d_i, d_j, d_dist, d_stats, d_deg))
        # nothing past `room`, the six stats or the n * (max_d + 1) degrees is written
        assert (i[room:] == -7).all() and (j[room:] == -7).all() and (dist[room:] == 0xAB).all()
        assert (stats[6:] == -7).all() and (deg[self.n * (max_d + 1):] == -7).all()
        stored = int(stats[1])
        assert 0 <= stored <= room
        return i[:stored], j[:stored], dist[:stored], stats[:6], deg[:self.n * (max_d + 1)].reshape(self.n, max_d + 1)

    def close(self):
        self.plan.close()


def check_whole(dev, n, L, max_d):
    wi, wj, wd = expected(n, L, max_d)
    i, j, dist, stats, deg = dev.run(max_d, wi.size + 3)
    per_d = np.bincount(wd, minlength=4)
    assert stats.tolist() == [wi.size, wi.size] + per_d.tolist(), (n, L, max_d)
    assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(dist, wd), (n, L, max_d)
    assert np.array_equal(deg, degrees(n, max_d, wi, wj, wd)), (n, L, max_d)


@pytest.mark.parametrize("L", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_every_seam_against_the_contract(n, L):
    pytest.importorskip("torch")
    dev = Device(make_set(n, L), L)
    try:
        assert (dev.plan.items > 0) == (n >= 2)
        for max_d in range(0, min(3, L) + 1):
            check_whole(dev, n, L, max_d)
        if L >= 15 and n >= 33:  # the planting put something at every threshold, and a decoy past the last
            ref = np.bincount(reference(n, L)[2], minlength=4)
            assert (ref[:4] > 0).all(), ref
    finally:
        dev.close()


@pytest.mark.parametrize("n,L", [(5000, 16), (2049, 4), (2049, 32), (1025, 17), (2049, 1)])
def test_item_ranges_concatenate_and_add(n, L):
    """Three disjoint item ranges cover [0, items): their pairs concatenated and re-sorted, their stats
    and degrees added, are the whole-range call's."""
    pytest.importorskip("torch")
    dev = Device(make_set(n, L), L)
    try:
        items = dev.plan.items
        cuts = [0, items // 3, 2 * items // 3 + 1, items]
        assert cuts == sorted(cuts) and items >= 3
        for max_d in (min(1, L), min(3, L)):
            wi, wj, wd = expected(n, L, max_d)
            parts = [dev.run(max_d, wi.size, b, e) for b, e in zip(cuts[:-1], cuts[1:])]
            words = np.concatenate([(p[0].astype(np.int64) << 33) | (p[1].astype(np.int64) << 2) | p[2] for p in parts])
            for p in parts:  # each part alone is in order
                assert np.array_equal(np.lexsort((p[1], p[0])), np.arange(p[0].size))
            words.sort()
            assert np.array_equal(words >> 33, wi) and np.array_equal((words >> 2) & (2 ** 31 - 1), wj)
            assert np.array_equal(words & 3, wd)
            stats = sum(p[3] for p in parts)
            assert stats.tolist() == [wi.size, wi.size] + np.bincount(wd, minlength=4).tolist()
            assert np.array_equal(sum(p[4].astype(np.int64) for p in parts), degrees(n, max_d, wi, wj, wd))
    finally:
        dev.close()


@pytest.mark.parametrize("n,L,max_d", [(5000, 16, 3), (1025, 4, 2), (2049, 32, 1), (257, 1, 1)])
def test_short_room_keeps_the_counts_exact(n, L, max_d):
    """room short of found (half of it, and 0): found, the per-distance totals and the degrees stay
    exact, stored == room, every stored pair is a pair of the contract and none repeats."""
    pytest.importorskip("torch")
    dev = Device(make_set(n, L), L)
    try:
        wi, wj, wd = expected(n, L, max_d)
        want = dict(zip(zip(wi.tolist(), wj.tolist()), wd.tolist()))
        assert wi.size >= 8
        for room in (wi.size // 2, 0):
            i, j, dist, stats, deg = dev.run(max_d, room)
            assert stats.tolist() == [wi.size, room] + np.bincount(wd, minlength=4).tolist()
            assert np.array_equal(deg, degrees(n, max_d, wi, wj, wd))
            got = list(zip(i.tolist(), j.tolist()))
            assert len(got) == room and len(set(got)) == room
            assert all(want.get(p) == d for p, d in zip(got, dist.tolist()))
    finally:
        dev.close()


def test_other_schemes_and_thresholds_are_refused():
    torch = pytest.importorskip("torch")
    codes = make_set(2049, 16)
    d_stats = torch.zeros(6, dtype=torch.int64, device="cuda")
    lib = _lib.lib()

    def call(dev, max_d):
        return lib.sct_allpairs_close_pairs(dev.plan._h, 0, dev.plan.items, max_d, None, None, None, 0,
                                            ctypes.c_void_p(d_stats.data_ptr()), None, None)

    for scheme in (_lib.SCHEME_MOMENTS, _lib.SCHEME_SPECTRAL):
        dev = Device(codes, 16, scheme=scheme)
        try:
            assert dev.plan.scheme == scheme
            assert call(dev, 1) == _lib.SCT_E_INVALID
            assert "SUBSETS" in _lib.last_error()
        finally:
            dev.close()
    dev = Device(codes, 16)
    try:
        assert call(dev, 4) == _lib.SCT_E_RANGE and call(dev, -1) == _lib.SCT_E_RANGE
        assert call(dev, 3) == _lib.SCT_OK
        torch.cuda.synchronize()
        assert int(d_stats[0].item()) == expected(2049, 16, 3)[0].size
    finally:
        dev.close()
    # the one-shot host form: the same refusals, and fewer than two codes are no pair
    with pytest.raises(ValueError):
        _lib.close_pairs(codes, 32, max_d=4)
    for few in (codes[:0], codes[:1]):
        i, j, dist, stats, deg = _lib.close_pairs(few, 32, max_d=2, room=4, degree=True)
        assert i.size == j.size == dist.size == 0 and stats.tolist() == [0] * 6 and deg.shape == (few.size, 3)


def _planted_keys(n, seed):
    """about n distinct 16-base codes, some of them 1..4 bases away from others"""
    rng = np.random.default_rng(seed)
    codes = synthetic.whitelist_codes(n, 16, seed=seed).tolist()
    for k in range(200):
        a, b = (int(v) for v in rng.choice(n, size=2, replace=False))
        codes[b] = _substitute(rng, codes[a], 16, 1 + k % 4)
    hub = int(rng.integers(0, n))
    for k in range(40):
        codes[int(rng.integers(0, n))] = _substitute(rng, codes[hub], 16, 1 + k % 4)
    return list(dict.fromkeys(codes))


def test_barcodes_close_pairs_and_neighbour_counts():
    pytest.importorskip("torch")
    keys = _planted_keys(20_000, 17)
    bc = barcode.Barcodes(dict.fromkeys(keys, 1), 16)
    codes = bc.codes_array()
    assert codes.tolist() == keys
    i, j, dist = bc.close_pairs(3)
    assert i.dtype == np.int32 and j.dtype == np.int32 and dist.dtype == np.uint8
    wi, wj, wd = C.close_pairs(codes, 32, 3)
    assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(dist, wd)
    # the headline histogram (through the MOMENTS path) counts the same pairs
    hist = bc.hamming_histogram()[:4]
    assert np.bincount(dist, minlength=4).tolist() == hist.tolist() and int(hist[1:].min()) > 0
    # neighbour counts = the pair list's bincount at both ends
    deg = bc.neighbour_counts(3)
    assert deg.dtype == np.int64 and np.array_equal(deg, degrees(len(keys), 3, i, j, dist))
    assert int(deg.sum(axis=1).max()) >= 20  # the hub
    # the default threshold, and a first room too small for the pairs: one more sweep
    one = dist <= 1
    for room in (None, 5, 0):
        i1, j1, d1 = bc.close_pairs(room=room) if room is not None else bc.close_pairs()
        assert np.array_equal(i1, i[one]) and np.array_equal(j1, j[one]) and np.array_equal(d1, dist[one])
    assert np.array_equal(bc.neighbour_counts(), deg[:, :2])


def test_barcodes_negative_keys_and_refusals():
    pytest.importorskip("torch")
    keys = _planted_keys(3000, 23)
    want = C.close_pairs(np.array(keys, dtype=np.uint64), 32, 2)
    neg = barcode.Barcodes({~k: 1 for k in keys}, 16)  # all negative: the XORs within the set are the same
    got = neg.close_pairs(2)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and want[0].size > 50
    assert np.array_equal(neg.neighbour_counts(2), C.neighbour_counts(np.array(keys, dtype=np.uint64), 32, 2))
    small = barcode.Barcodes({5: 1, 6: 1, 1 << 20: 2}, 16)
    for bad in (4, -1, 1.5):
        with pytest.raises(ValueError, match="max_distance in 0..3"):
            small.close_pairs(bad)
        with pytest.raises(ValueError, match="max_distance in 0..3"):
            small.neighbour_counts(bad)
    wide = barcode.Barcodes({1 << 70: 1, 5: 1}, 40)
    with pytest.raises(ValueError, match="below 2\\*\\*64"):
        wide.close_pairs()
    with pytest.raises(ValueError, match="below 2\\*\\*64"):
        wide.neighbour_counts()
    with pytest.raises(ValueError):  # mixed signs, as everywhere
        barcode.Barcodes({-5: 1, 6: 1}, 16).close_pairs()
    assert [a.tolist() for a in small.close_pairs(1)] == [[0], [1], [1]]
    assert small.neighbour_counts(1).tolist() == [[0, 1], [0, 1], [0, 0]]
