"""Counting molecules on the device (sctools_amd/csrc/molecules.hip): MoleculeCounter against
tests/molecules_reference.py, the contract in plain Python.  Every comparison is exact equality of
integers and of order; there is no tolerance anywhere.  All shapes are small, and every case runs
under each pre-aggregation form of the insert (SCT_TUNE_COUNT_PREAGG), none of which may change a
number."""

import math

import numpy as np
import pytest

import molecules_reference as R
from sctools_amd import _lib, barcode, counting, synthetic

pytestmark = pytest.mark.gpu

PREAGG = [0, 1, 2]  # none, wave merge, LDS table


def _same(mc, ref):
    """counts(), pairs(), info(), len() and saturation() of the device counter = the reference's."""
    reads, molecules, n_none, n_amb, n_bad = mc.counts()
    assert reads.dtype == np.int64 and molecules.dtype == np.int64 and reads.shape == molecules.shape == (ref.nw,)
    assert all(type(v) is int for v in (n_none, n_amb, n_bad))
    assert (reads.tolist(), molecules.tolist(), n_none, n_amb, n_bad) == ref.counts()
    index, umi = mc.pairs()
    assert index.dtype == np.int32 and umi.dtype == np.uint64
    assert list(zip(index.tolist(), umi.tolist())) == ref.pairs()
    info = mc.info()
    assert info["nmolecules"] == len(ref.seen) == len(mc) == int(molecules.sum())
    assert info["total"] == ref.total
    sat = mc.saturation()
    assert type(sat) is float and (sat == ref.saturation() or (math.isnan(sat) and math.isnan(ref.saturation())))
    return info


def _pair(nw, L, encoding, **kw):
    kind = {"ThreeBit": 3, "TwoBit": 2}[encoding]
    return counting.MoleculeCounter(nw, L, encoding=encoding, **kw), R.Molecules(nw, kind, L)


def _good_umis3(rng, n, L):
    """n ThreeBit UMI codes of L bases over C 1, A 2, G 3, T 4."""
    digits = rng.integers(1, 5, size=(n, L)).astype(np.uint64)
    return (digits << (np.uint64(3) * np.arange(L, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)


@pytest.mark.parametrize("preagg", PREAGG)
@pytest.mark.parametrize("n", [0, 1, 5000])
def test_tiny_inputs(n, preagg):
    """Nothing, one read, and 5,000 copies of one read: one molecule, one slot under maximal
    contention."""
    index = np.full(n, 7, dtype=np.int32)
    umis = np.full(n, int("1234", 8), dtype=np.uint64)
    with _lib.tuning(count_preagg=preagg):
        mc, ref = _pair(10, 4, "ThreeBit")
        with mc:
            assert mc.update(index, umis) is mc
            _same(mc, ref.update(index, umis))
            reads, molecules = mc.counts()[:2]
            assert reads[7] == n and molecules[7] == min(n, 1)


@pytest.mark.parametrize("preagg", PREAGG)
def test_key_separation(preagg):
    """One UMI under 50 barcodes and 50 UMIs under one barcode in one batch, key 0, and the 63-bit
    corner with its neighbours one bit away in the index or in the UMI."""
    nw, L = 2 ** 15, 24  # TwoBit: 15 + 48 = 63 key bits
    top = 2 ** 48 - 1
    reads = [(b, 0xABCDEF) for b in range(100, 150)] + [(9, u) for u in range(1000, 1050)]
    reads += [(0, 0), (0, 0), (0, 1), (1, 0)]
    reads += [(32767, top), (32767, top)]
    reads += [(32767 ^ (1 << b), top) for b in range(15)] + [(32767, top ^ (1 << b)) for b in range(48)]
    rng = np.random.default_rng(5)
    reads = [reads[i] for i in rng.permutation(len(reads))] * 2
    index = np.array([r[0] for r in reads], dtype=np.int32)
    umis = np.array([r[1] for r in reads], dtype=np.uint64)
    with _lib.tuning(count_preagg=preagg):
        mc, ref = _pair(nw, L, "TwoBit", capacity_hint=64)
        with mc:
            mc.update(index, umis)
            _same(mc, ref.update(index, umis))
            assert len(mc) == 50 + 50 + 3 + 1 + 15 + 48
            i, u = mc.pairs()
            assert (int(i[0]), int(u[0])) == (0, 0) and (int(i[-1]), int(u[-1])) == (32767, top)


def _family(name, n, rng):
    """n distinct (index, umi) molecules under nw = 37 and TwoBit L = 28 (56 UMI bits)."""
    if name == "arange":  # consecutive keys
        k = np.arange(n, dtype=np.uint64)
        return (k % np.uint64(37)).astype(np.int32), k // np.uint64(37)
    if name == "high_bits":  # only the UMI's high bits differ: hard on a hash that looks at the low ones
        return np.full(n, 36, dtype=np.int32), np.arange(n, dtype=np.uint64) << np.uint64(40)
    umis = np.unique(rng.integers(0, 2 ** 56, size=2 * n, dtype=np.uint64))
    return rng.integers(0, 37, size=n).astype(np.int32), rng.permutation(umis)[:n]


@pytest.mark.parametrize("preagg", PREAGG)
@pytest.mark.parametrize("family", ["arange", "high_bits", "random"])
def test_forced_growth(family, preagg):
    """capacity_hint=64 and 3,000 distinct molecules, each 1-4 times, shuffled, in three batches: the
    table grows at least four times, every batch leaves the reference's numbers, and the rehash adds
    nothing to molecules."""
    rng = np.random.default_rng(17)
    index, umis = _family(family, 3000, rng)
    assert len(set(zip(index.tolist(), umis.tolist()))) == 3000
    order = rng.permutation(np.repeat(np.arange(3000), rng.integers(1, 5, size=3000)))
    index, umis = index[order], umis[order]
    with _lib.tuning(count_preagg=preagg):
        mc, ref = _pair(37, 28, "TwoBit", capacity_hint=64)
        with mc:
            assert mc.info()["capacity"] == 64
            for lo, hi in ((0, 1), (1, 2501), (2501, order.size)):
                mc.update(index[lo:hi], umis[lo:hi])
                info = _same(mc, ref.update(index[lo:hi], umis[lo:hi]))
                assert int(mc.counts()[1].sum()) == info["nmolecules"]
                cap = info["capacity"]
                assert cap & (cap - 1) == 0 and 4 * info["nmolecules"] <= 3 * cap
            assert info["nmolecules"] == 3000 and cap >= 64 * 2 ** 4


@pytest.mark.parametrize("preagg", PREAGG)
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2048, 4097])
def test_tile_seams(n, preagg):
    """Every molecule twice, its two reads d apart for d in {1, 63, 64, 255, 256, 1023, 1024}: the
    duplicates fall inside a wave, across waves, across the LDS tile's edge and across grid strides
    (a read whose partner would lie past the end of the batch stays single).  The same batch again
    doubles reads and changes nothing else."""
    L = 10
    rng = np.random.default_rng(n)
    with _lib.tuning(count_preagg=preagg):
        for d in (1, 63, 64, 255, 256, 1023, 1024):
            mol = np.full(n, -1, dtype=np.int64)  # molecule number per read
            nxt = 0
            for i in range(n):
                if mol[i] >= 0:
                    continue
                mol[i] = nxt
                if i + d < n and mol[i + d] < 0:
                    mol[i + d] = nxt
                nxt += 1
            # molecule m: barcode m % 300, and a UMI spelling m in base 4 (distinct by construction)
            number = rng.permutation(4 ** L)[:nxt].astype(np.uint64)
            pool_i = (number % np.uint64(300)).astype(np.int32)
            pool_u = np.zeros(nxt, dtype=np.uint64)
            for p in range(L):
                pool_u |= (((number >> np.uint64(2 * p)) & np.uint64(3)) + np.uint64(1)) << np.uint64(3 * p)
            index, umis = pool_i[mol], pool_u[mol]
            mc, ref = _pair(300, L, "ThreeBit", capacity_hint=64)
            with mc:
                mc.update(index, umis)
                _same(mc, ref.update(index, umis))
                reads1, molecules1 = mc.counts()[:2]
                pairs1 = mc.pairs()
                mc.update(index, umis)
                _same(mc, ref.update(index, umis))
                reads2, molecules2 = mc.counts()[:2]
                assert np.array_equal(reads2, 2 * reads1) and np.array_equal(molecules2, molecules1)
                assert all(np.array_equal(a, b) for a, b in zip(mc.pairs(), pairs1))


def _with_triplet(umi, pos, value):
    return (int(umi) & ~(7 << (3 * pos))) | (value << (3 * pos))


@pytest.mark.parametrize("preagg", PREAGG)
def test_tallies(preagg):
    """4,000 ThreeBit L = 10 reads: -1 and -2 answers, UMIs with N and with the triplets 0 / 5 / 7 at
    the first, a middle and the last position, a zero UMI, a UMI with bit umi_bits set, and bad
    UMIs under -1, which count as no match and not as bad."""
    L, nw, n = 10, 50, 4000
    rng = np.random.default_rng(3)
    index = rng.integers(0, nw, size=n).astype(np.int32)
    umis = _good_umis3(rng, 400, L)[rng.integers(0, 400, size=n)]
    index[rng.random(n) < 0.1] = -1
    index[rng.random(n) < 0.05] = -2
    k = 0
    for value in (6, 0, 5, 7):
        for pos in (L - 1, L // 2, 0):  # first base = the high triplet
            for _ in range(5):
                umis[k] = _with_triplet(umis[k], pos, value)
                index[k] = k % nw
                k += 1
    umis[k], index[k] = 0, 3
    umis[k + 1], index[k + 1] = int(umis[k + 1]) | (1 << (3 * L)), 4
    umis[k + 2], index[k + 2] = 2 ** 64 - 1, 5
    for j in range(k + 3, k + 13):  # bad UMIs without a barcode
        umis[j], index[j] = _with_triplet(umis[j], 2, 6), -1 if j % 2 else -2
    perm = rng.permutation(n)
    index, umis = index[perm], umis[perm]
    with _lib.tuning(count_preagg=preagg):
        mc, ref = _pair(nw, L, "ThreeBit", capacity_hint=64)
        with mc:
            mc.update(index, umis)
            _same(mc, ref.update(index, umis))
            reads, _, n_none, n_amb, n_bad = mc.counts()
            assert n_bad == 60 + 3 and n_none >= 5 and n_amb >= 5
            assert int(reads.sum()) + n_none + n_amb + n_bad == n


@pytest.mark.parametrize("preagg", PREAGG)
def test_out_of_range_index(preagg):
    """One nw and one -3 in a batch of 2,000: ValueError (SCT_E_RANGE), every other read counted,
    nothing stored through the bad ones, and the counter goes on working."""
    L, nw, n = 8, 40, 2000
    rng = np.random.default_rng(11)
    index = rng.integers(-2, nw, size=n).astype(np.int32)
    umis = _good_umis3(rng, 300, L)[rng.integers(0, 300, size=n)]
    index[700], index[1300] = nw, -3
    with _lib.tuning(count_preagg=preagg):
        mc, ref = _pair(nw, L, "ThreeBit", capacity_hint=64)
        with mc:
            with pytest.raises(ValueError):
                mc.update(index, umis)
            assert "outside" in _lib.last_error()
            with pytest.raises(ValueError):
                ref.update(index, umis)
            _same(mc, ref)
            assert mc.info()["total"] == n
            mc.update(index[:700], umis[:700])  # a good batch afterwards is no error
            _same(mc, ref.update(index[:700], umis[:700]))


@pytest.mark.parametrize("preagg", PREAGG)
def test_pairs_with_too_little_room(preagg):
    index = np.array([2, 1, 2, 0, 1, 2], dtype=np.int32)
    umis = np.array([9, 9, 9, 10, 11, 12], dtype=np.uint64)
    mc, ref = _pair(3, 2, "TwoBit", capacity_hint=64)
    with _lib.tuning(count_preagg=preagg), mc:
        mc.update(index, umis)
        ref.update(index, umis)
        with pytest.raises(ValueError):
            mc.pairs(room=len(mc) - 1)
        assert "room" in _lib.last_error()
        _same(mc, ref)  # still usable, and right
        i, u = mc.pairs(room=len(mc) + 5)
        assert list(zip(i.tolist(), u.tolist())) == ref.pairs()
        mc.update(index[:2], umis[:2])
        _same(mc, ref.update(index[:2], umis[:2]))


@pytest.mark.parametrize("preagg", PREAGG)
def test_device_form(preagg):
    """update_device from torch tensors on a side stream, then update from host arrays on the
    library's own stream (which has to wait for the first), then the device forms of counts and
    fetch: the reference on the concatenation."""
    torch = pytest.importorskip("torch")
    L, nw = 10, 500
    rng = np.random.default_rng(29)
    index = rng.integers(-2, nw, size=30_000).astype(np.int32)
    umis = _good_umis3(rng, 2000, L)[rng.integers(0, 2000, size=30_000)]
    umis[::97] |= np.uint64(6)  # some N
    d_index, d_umi = torch.from_numpy(index[:20_000]).cuda(), torch.from_numpy(umis[:20_000].view(np.int64)).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _lib.tuning(count_preagg=preagg):
        mc, ref = _pair(nw, L, "ThreeBit", capacity_hint=1024)
        with mc:
            mc.update_device(d_index.data_ptr(), d_umi.data_ptr(), 20_000, stream=side.cuda_stream)
            mc.update(index[20_000:], umis[20_000:])
            info = _same(mc, ref.update(index, umis))
            n = info["nmolecules"]
            out_i = torch.full((n + 3,), -7, dtype=torch.int32, device="cuda")
            out_u = torch.zeros(n + 3, dtype=torch.int64, device="cuda")
            d_counts = torch.zeros(2 * nw + 3, dtype=torch.int64, device="cuda")
            s = side.cuda_stream
            mc.fetch_device(out_i.data_ptr(), out_u.data_ptr(), n + 3, stream=s)
            _lib.check(mc._lib.sct_molecules_counts(mc._h, d_counts.data_ptr(), d_counts.data_ptr() + 8 * nw,
                                                    d_counts.data_ptr() + 16 * nw, s))
            torch.cuda.synchronize()
            got = list(zip(out_i[:n].cpu().tolist(), out_u[:n].cpu().numpy().view(np.uint64).tolist()))
            assert got == ref.pairs()
            assert out_i[n:].cpu().tolist() == [-7] * 3 and not out_u[n:].any()  # rows past nmolecules untouched
            c = d_counts.cpu().tolist()
            assert (c[:nw], c[nw:2 * nw], c[2 * nw], c[2 * nw + 1], c[2 * nw + 2]) == ref.counts()


_E2E = {}


def _end_to_end_input():
    """(index of WhitelistCorrector.correct, count_corrected's result, umis, which UMIs hold an N),
    computed once for every form of the insert."""
    if not _E2E:
        n, nw, L = 20_000, 200, 10
        rng = np.random.default_rng(41)
        wl3 = rng.permutation(synthetic.two_to_three(synthetic.whitelist_codes(nw, 16, seed=3)))
        q, _, _ = synthetic.config4_queries(wl3, n, seed=4, device="cuda")
        q = q.cpu().numpy().view(np.uint64)
        qual = rng.integers(35, 74, size=(n, 16)).astype(np.uint8)
        umis = _good_umis3(rng, 3000, L)[rng.integers(0, 3000, size=n)]
        with_n = rng.random(n) < 0.02
        umis[with_n] = [_with_triplet(u, int(p), 6)
                        for u, p in zip(umis[with_n], rng.integers(0, L, size=int(with_n.sum())))]
        wc = barcode.WhitelistCorrector(wl3)
        try:
            index, _ = wc.correct(q, qual)
            _E2E["input"] = (np.array(index), wc.count_corrected(q, qual), umis, with_n)
        finally:
            wc.close()
    return _E2E["input"]


@pytest.mark.parametrize("preagg", PREAGG)
def test_end_to_end_with_the_corrector(preagg):
    """200 barcodes, 20,000 reads (exact, one substitution, one N, random), 10-base UMIs from 3,000
    molecules, some with N: WhitelistCorrector.correct, then MoleculeCounter.update, against the
    reference fed correct's own index; and reads = count_corrected's counts less the bad-UMI reads."""
    pytest.importorskip("torch")
    n, nw, L = 20_000, 200, 10
    index, (corrected, c_none, c_amb), umis, with_n = _end_to_end_input()
    mc, ref = _pair(nw, L, "ThreeBit")
    with _lib.tuning(count_preagg=preagg), mc:
        mc.update(index, umis)
        _same(mc, ref.update(index, umis))
        reads, molecules, n_none, n_amb, n_bad = mc.counts()
    assert int(reads.sum()) + n_none + n_amb + n_bad == n
    assert (n_none, n_amb) == (c_none, c_amb) and n_bad > 0 and n_none > 0
    bad_per_barcode = np.bincount(index[(index >= 0) & with_n], minlength=nw)
    assert np.array_equal(reads, corrected - bad_per_barcode)
    assert 0 < int(molecules.sum()) < int(reads.sum())
