"""Counting on the device (sctools_amd/csrc/count.hip): DeviceCounter against collections.Counter
-- which is literally what the reference calls (barcode.py:102) -- and WhitelistCorrector.count
against np.bincount over nearest() of the same corrector.  Every comparison is exact equality of
integers and of order; there is no tolerance anywhere.  All shapes are small."""

import ctypes
from collections import Counter

import numpy as np
import pytest

from sctools_amd import _lib, barcode, counting, synthetic

pytestmark = pytest.mark.gpu

PREAGG = [0, 1, 2]  # SCT_TUNE_COUNT_PREAGG: none, wave merge, LDS table (none changes a result)


def _same_as_counter(dc, codes):
    want = Counter(codes.tolist())
    got = dc.counter()
    assert list(got.items()) == list(want.items())
    assert all(type(k) is int and type(v) is int for k, v in got.items())
    keys, counts, first = dc.arrays()
    assert dc.total == codes.size
    assert int(counts.sum()) == codes.size
    assert len(dc) == len(want) == keys.size
    return keys, counts, first


@pytest.mark.parametrize("preagg", PREAGG)
@pytest.mark.parametrize("n", [0, 1, 5000])
def test_tiny_inputs(n, preagg):
    """Nothing, one code, and 5,000 copies of one code (one slot, maximal contention)."""
    codes = np.full(n, 0x1234_5678_9ABC, dtype=np.uint64)
    with _lib.tuning(count_preagg=preagg), counting.DeviceCounter() as dc:
        dc.update(codes)
        keys, counts, first = _same_as_counter(dc, codes)
        assert first.tolist() == ([0] if n else [])


def _family(name, n, rng):
    if name == "arange":
        return np.arange(n, dtype=np.uint64)
    if name == "mult32":  # only high bits differ: hard on a hash that looks at the low ones
        return np.arange(n, dtype=np.uint64) << np.uint64(32)
    keys = np.unique(rng.integers(0, 2 ** 64, size=2 * n, dtype=np.uint64, endpoint=False))
    return rng.permutation(keys)[:n]


@pytest.mark.parametrize("preagg", PREAGG)
@pytest.mark.parametrize("family", ["arange", "mult32", "random"])
def test_forced_growth(family, preagg):
    """capacity_hint=64 and 3,000 distinct codes, each 1-4 times, shuffled: the table has to grow
    at least four times on the way, and the result is Counter's, order included."""
    rng = np.random.default_rng(17)
    keys = _family(family, 3000, rng)
    assert np.unique(keys).size == 3000
    codes = rng.permutation(np.repeat(keys, rng.integers(1, 5, size=keys.size)))
    with _lib.tuning(count_preagg=preagg), counting.DeviceCounter(capacity_hint=64) as dc:
        assert dc.info()["capacity"] == 64
        dc.update(codes)
        _same_as_counter(dc, codes)
        cap = dc.info()["capacity"]
        assert cap >= 64 * 2 ** 4 and cap & (cap - 1) == 0
        assert 4 * 3000 <= 3 * cap  # (never above the 3/4 load the growth rule allows)


@pytest.mark.parametrize("preagg", PREAGG)
def test_sentinel_and_edges(preagg):
    """0, 2^64 - 1 (the table's empty mark: several times, first seen mid-stream), 2^63 and 1; and
    an int64 array with negative values, whose keys come back negative."""
    top = 2 ** 64 - 1
    codes = np.array([5, 0, 1, 0, top, 2 ** 63, top, 7, top, 1, 2 ** 63, 0, top - 1], dtype=np.uint64)
    with _lib.tuning(count_preagg=preagg), counting.DeviceCounter(capacity_hint=64) as dc:
        dc.update(codes)
        keys, counts, first = _same_as_counter(dc, codes)
        assert keys.dtype == np.uint64
        assert dc.counter()[top] == 3 and first[keys.tolist().index(top)] == 4
        dc.update(codes)  # the side slot keeps counting across batches
        assert list(dc.counter().items()) == list(Counter(codes.tolist() * 2).items())
    signed = np.array([-1, 3, -(2 ** 63), -1, 0, -7, 3, -1, 2 ** 63 - 1], dtype=np.int64)
    with _lib.tuning(count_preagg=preagg), counting.DeviceCounter(capacity_hint=64) as dc:
        dc.update(signed)
        keys, counts, first = _same_as_counter(dc, signed)
        assert keys.dtype == np.int64 and keys.tolist() == [-1, 3, -(2 ** 63), 0, -7, 2 ** 63 - 1]


@pytest.mark.parametrize("preagg", PREAGG)
def test_streaming_equals_one_shot(preagg):
    """200,000 codes over 300 distinct values, skewed, fed as batches of 1, 70,001 and the rest:
    the same rows as one update, and first = np.unique's first indices in global positions."""
    rng = np.random.default_rng(23)
    values = rng.integers(0, 2 ** 48, size=300, dtype=np.uint64)
    codes = values[np.minimum((rng.pareto(1.2, size=200_000) * 8).astype(np.int64), 299)]
    with _lib.tuning(count_preagg=preagg):
        with counting.DeviceCounter(capacity_hint=256) as one:
            one.update(codes)
            k1, c1, f1 = _same_as_counter(one, codes)
        with counting.DeviceCounter(capacity_hint=256) as dc:
            for piece in (codes[:1], codes[1:70_002], codes[70_002:]):
                dc.update(piece)
            k2, c2, f2 = _same_as_counter(dc, codes)
    for a, b in ((k1, k2), (c1, c2), (f1, f2)):
        assert np.array_equal(a, b)
    uk, ui, uc = np.unique(codes, return_index=True, return_counts=True)
    order = np.argsort(ui)
    assert np.array_equal(k2, uk[order])
    assert np.array_equal(f2, ui[order])
    assert np.array_equal(c2.astype(np.int64), uc[order])


def test_device_resident_path():
    """update_device on a tensor's pointer and sct_counter_fetch into tensors = the host path."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(29)
    codes = rng.integers(0, 5000, size=150_000, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    d = torch.from_numpy(codes.view(np.int64)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    with counting.DeviceCounter(capacity_hint=1024) as dc, counting.DeviceCounter(capacity_hint=1024) as host:
        dc.update_device(d.data_ptr(), 100_000, stream=s)
        dc.update_device(d.data_ptr() + 8 * 100_000, 50_000, stream=s)
        n = len(dc)
        out = [torch.zeros(n + 3, dtype=torch.int64, device="cuda") for _ in range(3)]
        dc.fetch_device(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), n + 3, stream=s)
        torch.cuda.synchronize()
        keys, counts, first = (t.cpu().numpy() for t in out)
        host.update(codes)
        hk, hc, hf = _same_as_counter(host, codes)
        assert np.array_equal(keys[:n].view(np.uint64), hk)
        assert np.array_equal(counts[:n].view(np.uint64), hc)
        assert np.array_equal(first[:n], hf)
        assert not keys[n:].any() and not counts[n:].any() and not first[n:].any()  # rows past nunique untouched
        assert dc.total == codes.size


def test_counter_destroy_waits_for_enqueued_work():
    """A counter closed right after an update was enqueued on a side stream returns only once that
    work has completed (compare test_plan_destroy_waits_for_enqueued_work)."""
    torch = pytest.importorskip("torch")
    side = torch.cuda.Stream()
    d = torch.arange(4_000_000, dtype=torch.int64, device="cuda") % 1000
    torch.cuda.synchronize()
    dc = counting.DeviceCounter(capacity_hint=1 << 22)
    dc.update_device(d.data_ptr(), d.numel(), stream=side.cuda_stream)
    ev = torch.cuda.Event()
    ev.record(side)
    dc.close()
    assert ev.query(), "counter destroy returned before its enqueued update finished"


def test_fetch_with_too_little_room():
    codes = np.array([9, 8, 9, 7, 8, 9], dtype=np.uint64)
    with counting.DeviceCounter(capacity_hint=64) as dc:
        dc.update(codes)
        with pytest.raises(ValueError):
            dc.arrays(room=2)
        assert "room" in _lib.last_error()
        _same_as_counter(dc, codes)  # still usable, and right
        dc.update(codes[:2])
        _same_as_counter(dc, np.concatenate([codes, codes[:2]]))


def test_barcodes_from_encoded_array():
    rng = np.random.default_rng(31)
    codes = rng.choice(synthetic.whitelist_codes(3000, 16), size=20_000)
    got = barcode.Barcodes.from_encoded_array(codes, 16)
    want = barcode.Barcodes.from_iterable_encoded(codes.tolist(), 16)
    assert dict(got._data) == dict(want._data)
    assert list(got) == list(want)
    assert got.summarize_hamming_distances() == want.summarize_hamming_distances()
    assert np.array_equal(got.base_frequency(), want.base_frequency())
    obs = barcode.ObservedBarcodeSet.from_encoded_array(codes, 16)
    assert type(obs) is barcode.ObservedBarcodeSet and list(obs) == list(want)
    q = codes[:50]
    assert np.array_equal(got.nearest(q)[0], want.nearest(q)[0])  # indices follow iteration order


_Q = {}


def _queries(wl3, nq, seed):
    """config4_queries (exact, one substitution, one N, random) as a host uint64 array."""
    torch = pytest.importorskip("torch")
    key = (wl3.tobytes(), nq, seed)
    if key not in _Q:
        q, _, _ = synthetic.config4_queries(wl3, nq, seed=seed, device="cuda")
        _Q[key] = q.cpu().numpy().view(np.uint64)
    return _Q[key]


def _check_count(wc, q):
    idx, _ = wc.nearest(q)
    idx = np.asarray(idx)
    counts, n_none, n_tie = wc.count(q)
    assert counts.dtype == np.int64 and counts.shape == (wc.size,)
    assert np.array_equal(counts, np.bincount(idx[idx >= 0], minlength=wc.size))
    assert n_none == int((idx == -1).sum()) and n_tie == int((idx == -2).sum())
    assert int(counts.sum()) + n_none + n_tie == q.size
    return counts, n_none, n_tie


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_whitelist_corrector_count(devices):
    rng = np.random.default_rng(37)
    wl3 = rng.permutation(synthetic.two_to_three(synthetic.whitelist_codes(1000, 16, seed=3)))
    q = _queries(wl3, 50_000, 4)
    wc = barcode.WhitelistCorrector(wl3, devices=devices)
    try:
        counts, n_none, n_tie = _check_count(wc, q)
        assert n_none > 0 and counts.max() > 1
        # two batches into one accumulator = their sum
        acc = wc.count(q[:20_001])
        acc = wc.count(q[20_001:], out=acc)
        assert np.array_equal(acc[0], counts) and acc[1:] == (n_none, n_tie)
        only = np.zeros(wc.size, dtype=np.int64)
        got = wc.count(q, out=only)
        assert got[0] is only and np.array_equal(only, counts)
        assert wc.count(q[:0])[1:] == (0, 0)
    finally:
        wc.close()


def test_whitelist_corrector_count_ties_and_distance_two():
    rng = np.random.default_rng(41)
    wl3 = rng.permutation(synthetic.two_to_three(synthetic.whitelist_codes(1000, 16, seed=3)))
    q = _queries(wl3, 50_000, 4)
    dup = np.concatenate([wl3, wl3[:3]])  # a whitelist holding duplicate codes: their reads tie
    wc = barcode.WhitelistCorrector(dup)
    try:
        counts, n_none, n_tie = _check_count(wc, q)
        assert n_tie > 0
    finally:
        wc.close()
    wc = barcode.WhitelistCorrector(wl3, max_distance=2)  # not the half-key scheme
    try:
        _check_count(wc, q[:20_000])
    finally:
        wc.close()


def test_index_tally_refuses_out_of_range_index():
    """An index equal to nw (or below -2) makes the call SCT_E_RANGE and is never stored through:
    the words behind counts[nw - 1] stay zero, the valid entries are counted."""
    torch = pytest.importorskip("torch")
    nw = 10
    lib = _lib.lib()
    vp = ctypes.c_void_p
    for bad in (nw, nw + 5, -3, np.iinfo(np.int32).min, np.iinfo(np.int32).max):
        idx = np.array([0, 1, bad, 2, -1, -2, nw - 1, 1], dtype=np.int32)
        d_idx = torch.from_numpy(idx).cuda()
        d_counts = torch.zeros(nw + 64, dtype=torch.int64, device="cuda")
        d_tally = torch.zeros(2, dtype=torch.int64, device="cuda")
        rc = lib.sct_index_tally(vp(d_idx.data_ptr()), idx.size, nw, vp(d_counts.data_ptr()), vp(d_tally.data_ptr()),
                                 None)
        assert rc == _lib.SCT_E_RANGE
        with pytest.raises(ValueError):
            _lib.check(rc)
        torch.cuda.synchronize()
        counts = d_counts.cpu().numpy()
        assert not counts[nw:].any()
        valid = idx[(idx >= 0) & (idx < nw)]
        assert counts[:nw].tolist() == np.bincount(valid, minlength=nw).tolist()
        assert d_tally.cpu().tolist() == [1, 1]
    # and a clean batch accumulates into what is there
    idx = np.array([3, 3, -1, 9], dtype=np.int32)
    d_idx = torch.from_numpy(idx).cuda()
    d_counts = torch.ones(nw, dtype=torch.int64, device="cuda")
    d_tally = torch.zeros(2, dtype=torch.int64, device="cuda")
    _lib.check(lib.sct_index_tally(vp(d_idx.data_ptr()), idx.size, nw, vp(d_counts.data_ptr()),
                                   vp(d_tally.data_ptr()), None))
    torch.cuda.synchronize()
    assert d_counts.cpu().tolist() == [1, 1, 1, 3, 1, 1, 1, 1, 1, 2] and d_tally.cpu().tolist() == [1, 0]
