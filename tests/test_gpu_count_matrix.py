"""The barcode x feature count matrix on the device (sctools_amd/csrc/molecules.hip): a
MoleculeCounter(features=nf) against tests/count_matrix_reference.py, the contract in plain Python.
Every comparison is exact equality of integers and of order; there is no tolerance anywhere.  All
shapes are at most a few thousand reads (one of about 20,000), and a case's input and reference are
computed once for the pre-aggregation forms of the insert (SCT_TUNE_COUNT_PREAGG) it runs under."""

import ctypes
import functools

import numpy as np
import pytest

import count_matrix_reference as M
from sctools_amd import _lib, counting

pytestmark = pytest.mark.gpu

PREAGG = [0, 1, 2]  # none, wave merge, LDS table
ENC = {3: "ThreeBit", 2: "TwoBit"}
C, A, G, T, N = 1, 2, 3, 4, 6


def umi3(*bases):
    """A ThreeBit code written first base first (the first base in the high triplet)."""
    code = 0
    for b in bases:
        code = (code << 3) | b
    return code


def _all_umis3(L):
    """Every good ThreeBit code of L bases, ascending."""
    codes = np.zeros(1, dtype=np.uint64)
    for _ in range(L):
        codes = (codes[:, None] << np.uint64(3) | np.arange(1, 5, dtype=np.uint64)[None, :]).reshape(-1)
    return codes


def _good_umis(rng, n, kind, L):
    lo = 1 if kind == 3 else 0
    d = rng.integers(lo, lo + 4, size=(n, L)).astype(np.uint64)
    return (d << (np.uint64(kind) * np.arange(L, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)


def _mix(n, nw, nf, kind, L, seed):
    """n reads that meet every rule: molecules drawn from a pool of about n / 3 (duplicates inside a
    wave and tiles apart), and index -1, -2, UMIs with N (or a bit too many), features -1 and -2."""
    rng = np.random.default_rng(seed)
    pool = max(1, n // 3)
    pi, pf, pu = rng.integers(0, nw, pool), rng.integers(0, nf, pool), _good_umis(rng, pool, kind, L)
    pick = rng.integers(0, pool, n)
    pick[1::2] = pick[::2][:pick[1::2].size]  # neighbours in a wave share a molecule
    index, feature, umi = pi[pick].astype(np.int32), pf[pick].astype(np.int32), pu[pick].copy()
    what = rng.integers(0, 20, n)
    index[what == 0] = -1
    index[what == 1] = -2
    umi[what == 2] |= np.uint64(6) if kind == 3 else np.uint64(1) << np.uint64(kind * L)
    feature[what == 3] = -1
    feature[what == 4] = -2
    both = what == 5  # a bad UMI and no feature: a bad UMI
    umi[both] |= np.uint64(6) if kind == 3 else np.uint64(1) << np.uint64(kind * L)
    feature[both] = -1
    return index, feature, umi


def _snap(ref):
    """Everything the device counter is compared with, taken from the reference as it stands."""
    return {"counts": ref.counts(), "no_feature": ref.n_no_feature, "pairs": ref.pairs(), "total": ref.total,
            "matrix": ref.matrix(), "collapse": ref.collapse()}


def _matrix_lists(got):
    return tuple(a.tolist() for a in got)


def _same(mc, snap, nw, counted):
    """counts(), n_no_feature, info(), pairs() with and without the feature column, matrix() in every
    form (twice) and collapse() of the device counter = the reference's."""
    reads, molecules, n_none, n_amb, n_bad = mc.counts()
    assert (reads.tolist(), molecules.tolist(), n_none, n_amb, n_bad) == snap["counts"]
    assert mc.n_no_feature == snap["no_feature"]
    rows = snap["pairs"]
    info = mc.info()
    assert info["nmolecules"] == len(rows) == len(mc) and info["total"] == snap["total"]
    three = mc.pairs(features=True)
    assert [a.dtype for a in three] == [np.int32, np.int32, np.uint64]
    assert list(zip(*(a.tolist() for a in three))) == [r[:3] for r in rows]
    two = mc.pairs()  # the same rows without the feature column
    assert list(zip(*(a.tolist() for a in two))) == [(r[0], r[2]) for r in rows]
    indptr, feature, mol, rds, col = snap["matrix"]
    got = mc.matrix()
    assert [a.dtype for a in got] == [np.int64, np.int32, np.int64]
    assert got[0].shape == (nw + 1,) and got[1].shape == got[2].shape == (len(feature),)
    assert _matrix_lists(got) == (indptr, feature, mol)
    assert _matrix_lists(mc.matrix()) == (indptr, feature, mol)  # it reads only
    if not counted:
        return info
    five = mc.pairs(features=True, reads=True, parents=True)
    assert [a.dtype for a in five] == [np.int32, np.int32, np.uint64, np.int64, np.uint64]
    assert list(zip(*(a.tolist() for a in five))) == rows
    four = mc.pairs(reads=True, parents=True)
    assert list(zip(*(a.tolist() for a in four))) == [(r[0],) + r[2:] for r in rows]
    assert _matrix_lists(mc.matrix(reads=True)) == (indptr, feature, mol, rds)
    assert _matrix_lists(mc.matrix(collapsed=True)) == (indptr, feature, mol, col)
    full = mc.matrix(reads=True, collapsed=True)
    assert [a.dtype for a in full] == [np.int64, np.int32, np.int64, np.int64, np.int64]
    assert _matrix_lists(full) == (indptr, feature, mol, rds, col)
    collapsed, n_corrected = mc.collapse()
    assert (collapsed.tolist(), n_corrected) == snap["collapse"]
    # the invariant: the matrix's row sums are the per-barcode vectors
    for values, per_barcode in ((full[2], molecules), (full[3], reads), (full[4], collapsed)):
        sums = np.add.reduceat(np.append(values, 0), full[0][:-1])
        sums[full[0][:-1] == full[0][1:]] = 0
        assert sums.tolist() == per_barcode.tolist()
    return info


def _run(nw, nf, kind, L, batches, snaps, counted, hint=64, preagg=1):
    """Feed the batches, comparing with the snapshot after each; returns the last info()."""
    info = None
    with _lib.tuning(count_preagg=preagg):
        with counting.MoleculeCounter(nw, L, ENC[kind], capacity_hint=hint, read_counts=counted, features=nf) as mc:
            assert mc.features == nf
            for (index, feature, umi), snap in zip(batches, snaps):
                mc.update(index, umi, features=feature)
                info = _same(mc, snap, nw, counted)
    return info


def _reference(nw, nf, kind, L, batches):
    ref = M.FeatureMolecules(nw, nf, kind, L)
    snaps = []
    for index, feature, umi in batches:
        ref.update(index, umi, feature)
        snaps.append(_snap(ref))
    return snaps


# ---- reads per update: the wave, workgroup and LDS-tile seams of the insert

SIZES = [0, 1, 63, 64, 65, 255, 257, 1023, 1024, 1025, 4097]


@functools.lru_cache(maxsize=None)
def _sized_case(n):
    nw, nf, kind, L = 37, 11, 3, 5
    batches = [_mix(n, nw, nf, kind, L, seed=n + 1)]
    return nw, nf, kind, L, batches, _reference(nw, nf, kind, L, batches)


@pytest.mark.parametrize("preagg", PREAGG)
@pytest.mark.parametrize("n", SIZES)
def test_reads_per_update(n, preagg):
    nw, nf, kind, L, batches, snaps = _sized_case(n)
    _run(nw, nf, kind, L, batches, snaps, counted=True, preagg=preagg)
    if n >= 255:  # the mix held every rule
        reads, molecules, n_none, n_amb, n_bad = snaps[-1]["counts"]
        assert min(n_none, n_amb, n_bad, snaps[-1]["no_feature"]) > 0 and sum(molecules) < sum(reads)


@pytest.mark.parametrize("counted", [False, True])
def test_plain_feature_counter_and_two_bit(counted):
    nw, nf, kind, L = 5, 3, 2, 4
    batches = [_mix(700, nw, nf, kind, L, seed=3), _mix(300, nw, nf, kind, L, seed=4)]
    _run(nw, nf, kind, L, batches, _reference(nw, nf, kind, L, batches), counted=counted)


# ---- widths

def test_one_bit_each():
    nw, nf, kind, L = 1, 1, 3, 3
    batches = [_mix(500, nw, nf, kind, L, seed=5)]
    snaps = _reference(nw, nf, kind, L, batches)
    assert snaps[-1]["matrix"][0] == [0, 1]
    _run(nw, nf, kind, L, batches, snaps, counted=True)


def test_feature_that_fits_the_bits_but_not_nf():
    """nf = 3 has two feature bits: feature 3 packs without touching the index, and must be
    SCT_E_RANGE with no key left behind, as must nf itself and -3, after the rest was counted."""
    nw, nf, kind, L = 4, 3, 3, 2
    AA, AC = umi3(A, A), umi3(A, C)
    index = np.array([0, 1, 2, 3, 3], dtype=np.int32)
    umi = np.array([AA, AA, AC, AC, AC], dtype=np.uint64)
    for bad in (3, -3, 2 ** 31 - 1, -2 ** 31):
        feature = np.array([2, bad, 0, 1, 1], dtype=np.int32)
        ref = M.FeatureMolecules(nw, nf, kind, L)
        with pytest.raises(ValueError):
            ref.update(index, umi, feature)
        with counting.MoleculeCounter(nw, L, capacity_hint=64, read_counts=True, features=nf) as mc:
            with pytest.raises(ValueError, match="feature outside"):
                mc.update(index, umi, features=feature)
            assert mc._lib.sct_molecules_update_features_host(mc._h, _lib._ptr(index), _lib._ptr(feature),
                                                              _lib._ptr(umi), 5) == _lib.SCT_E_RANGE
            ref.total += 5  # the second call: the same reads again
            for k in list(ref.mreads):
                ref.mreads[k] *= 2
            ref.reads = [2 * r for r in ref.reads]
            _same(mc, _snap(ref), nw, True)
            assert len(mc) == 3 and mc.counts()[0].tolist() == [2, 0, 2, 4]
            # an index out of range with a good feature: the message names both ranges
            with pytest.raises(ValueError, match=r"index outside \[-2, 4\) or feature outside \[-2, 3\)"):
                mc.update([4], [AA], features=[0])


def test_key_of_63_bits():
    """1 + 2 + 60 bits: the largest index, feature and UMI present, and their neighbours."""
    nw, nf, kind, L = 2, 4, 2, 30
    top = 2 ** 60 - 1
    rows = [(1, 3, top), (1, 3, top), (1, 3, top - 1), (1, 3, 0), (1, 0, top), (0, 3, top), (0, 0, 0), (1, 2, top ^ (3 << 58))]
    batches = [tuple(np.array([r[k] for r in rows], dtype=t) for k, t in ((0, np.int32), (1, np.int32), (2, np.uint64)))]
    snaps = _reference(nw, nf, kind, L, batches)
    assert M.key(1, 3, top, nf, kind, L) == 2 ** 63 - 1
    for preagg in PREAGG:
        _run(nw, nf, kind, L, batches, snaps, counted=True, preagg=preagg)
    with pytest.raises(ValueError):
        counting.MoleculeCounter(3, L, "TwoBit", features=nf)  # 64 bits


# ---- growth

def test_growth_from_64_slots():
    """capacity_hint = 64 fed about 5,000 molecules in three batches: the table rehashes several
    times, and the matrix is taken before and after each."""
    nw, nf, kind, L = 50, 20, 3, 6
    rng = np.random.default_rng(17)
    batches = []
    for n in (40, 2000, 3000):
        index = rng.integers(0, nw, n).astype(np.int32)
        feature = rng.integers(0, nf, n).astype(np.int32)
        batches.append((index, feature, _good_umis(rng, n, kind, L)))
    snaps = _reference(nw, nf, kind, L, batches)
    assert 4500 < len(snaps[-1]["pairs"]) <= 5040
    info = _run(nw, nf, kind, L, batches, snaps, counted=True, hint=64)
    assert info["capacity"] >= 8192


# ---- shapes the run pass can get wrong

def _from_rows(rows):
    return (np.array([r[0] for r in rows], dtype=np.int32), np.array([r[1] for r in rows], dtype=np.int32),
            np.array([r[2] for r in rows], dtype=np.uint64))


def test_empty_counter():
    with counting.MoleculeCounter(7, 4, features=5, read_counts=True, capacity_hint=64) as mc:
        for got in (mc.matrix(), mc.matrix(reads=True, collapsed=True), mc.matrix(room=0)):
            assert got[0].tolist() == [0] * 8 and all(a.size == 0 for a in got[1:])
        assert mc.n_no_feature == 0 and mc.pairs(features=True)[1].size == 0
        mc.update([-1, 0], [umi3(A, A, A, A), umi3(A, A, A, N)], features=[0, 0])  # nothing stored
        assert mc.matrix()[0].tolist() == [0] * 8


@pytest.mark.parametrize("filled", [[3], [0], [6], [1, 2, 4, 5], [0, 6], [0, 1, 2, 3, 4, 5, 6]])
def test_empty_barcodes_at_the_start_middle_and_end(filled):
    """nw = 7: one molecule alone in the middle, barcode 0 or nw - 1 the only one filled, both ends
    empty, and every barcode filled."""
    nw, nf, kind, L = 7, 4, 3, 2
    rows = []
    for i in filled:
        rows += [(i, (i + k) % nf, umi3(A, C + (k % 4))) for k in range(1 if len(filled) == 1 and i == 3 else 3)]
        rows.append(rows[-1])
    batches = [_from_rows(rows)]
    snaps = _reference(nw, nf, kind, L, batches)
    _run(nw, nf, kind, L, batches, snaps, counted=True)


def test_one_entry_of_4096_molecules():
    """Every ThreeBit UMI of 6 bases under one (barcode, feature): one entry over 64 wave tiles, whose
    values arrive as one add per tile; every molecule has all 18 neighbours."""
    nw, nf, kind, L = 3, 2, 3, 6
    umis = _all_umis3(L)
    assert umis.size == 4096
    reads = np.repeat(umis, 1 + (np.arange(4096) % 3))  # 1, 2 or 3 reads
    index = np.full(reads.size, 1, dtype=np.int32)
    feature = np.full(reads.size, 1, dtype=np.int32)
    batches = [(index, feature, reads)]
    snaps = _reference(nw, nf, kind, L, batches)
    assert snaps[0]["matrix"][:3] == ([0, 0, 1, 1], [1], [4096])
    _run(nw, nf, kind, L, batches, snaps, counted=True)


def test_3000_entries_of_one_molecule():
    nw, nf, kind, L = 100, 64, 3, 4
    rng = np.random.default_rng(23)
    cells = rng.permutation(nw * nf)[:3000]
    batches = [((cells // nf).astype(np.int32), (cells % nf).astype(np.int32), _good_umis(rng, 3000, kind, L))]
    snaps = _reference(nw, nf, kind, L, batches)
    assert snaps[0]["matrix"][2] == [1] * 3000
    _run(nw, nf, kind, L, batches, snaps, counted=True)


@pytest.mark.parametrize("sizes", [(256, 768, 100), (64, 192, 768, 1), (63, 1, 192, 767, 1, 65), (1024, 1024, 1)])
def test_entry_boundaries_on_tile_seams(sizes):
    """Entries whose first sorted row is row 64, 256 or 1,024 exactly (and one row either side)."""
    nw, nf, kind, L = 4, 3, 3, 6
    umis = _all_umis3(L)
    rng = np.random.default_rng(sum(sizes))
    rows_i, rows_f, rows_u = [], [], []
    for e, size in enumerate(sizes):  # entry e = (e // nf, e % nf): ascending key order
        pick = np.sort(rng.permutation(4096)[:size])
        rows_i.append(np.full(size, e // nf)), rows_f.append(np.full(size, e % nf)), rows_u.append(umis[pick])
    index, feature, umi = np.concatenate(rows_i), np.concatenate(rows_f), np.concatenate(rows_u)
    perm = rng.permutation(index.size)
    perm = np.concatenate([perm, perm[::5]])  # some molecules twice
    batches = [(index[perm].astype(np.int32), feature[perm].astype(np.int32), umi[perm])]
    snaps = _reference(nw, nf, kind, L, batches)
    assert snaps[0]["matrix"][2] == list(sizes)
    _run(nw, nf, kind, L, batches, snaps, counted=True)


def test_room():
    """room == nnz is taken; room == nnz - 1 is refused with nnz reported and the counter as it was."""
    nw, nf, kind, L = 9, 5, 3, 4
    index, feature, umi = _mix(2000, nw, nf, kind, L, seed=31)
    ref = M.FeatureMolecules(nw, nf, kind, L).update(index, umi, feature)
    snap = _snap(ref)
    nnz = len(snap["matrix"][1])
    assert 1 < nnz < len(snap["pairs"])
    with counting.MoleculeCounter(nw, L, capacity_hint=64, read_counts=True, features=nf) as mc:
        mc.update(index, umi, features=feature)
        assert _matrix_lists(mc.matrix(reads=True, collapsed=True, room=nnz)) == snap["matrix"]
        with pytest.raises(ValueError, match="the matrix has %d" % nnz):
            mc.matrix(room=nnz - 1)
        indptr = np.full(nw + 1, -5, dtype=np.int64)
        feat = np.full(nnz, -5, dtype=np.int32)
        mol = np.full(nnz, 77, dtype=np.uint64)
        got = ctypes.c_int64(-1)
        for room in (nnz - 1, 0):
            rc = mc._lib.sct_molecules_matrix_host(mc._h, _lib._ptr(indptr), _lib._ptr(feat), _lib._ptr(mol), None, None,
                                                   room, ctypes.byref(got))
            assert rc == _lib.SCT_E_INVALID and got.value == nnz
            assert (indptr == -5).all() and (feat == -5).all() and (mol == 77).all()
        _same(mc, snap, nw, True)


# ---- invariants on a larger random case, the device forms, and the host grouping

@functools.lru_cache(maxsize=None)
def _random_case():
    nw, nf, kind, L = 300, 40, 3, 8
    index, feature, umi = _mix(20_000, nw, nf, kind, L, seed=41)
    # mutate some UMIs by one base so that the collapse has work
    rng = np.random.default_rng(43)
    hit = rng.random(umi.size) < 0.1
    pos = rng.integers(0, L, umi.size).astype(np.uint64) * np.uint64(3)
    good = (umi & np.uint64(6 << 0)) != np.uint64(6)  # leave the N reads alone
    flip = hit & good
    old = (umi >> pos) & np.uint64(7)
    new = (old % np.uint64(4)) + np.uint64(1)
    umi = np.where(flip, (umi & ~(np.uint64(7) << pos)) | (new << pos), umi)
    batches = [(index, feature, umi)]
    return nw, nf, kind, L, batches, _reference(nw, nf, kind, L, batches)


def test_random_case_invariants_and_host_grouping():
    nw, nf, kind, L, batches, snaps = _random_case()
    index, feature, umi = batches[0]
    assert snaps[0]["collapse"][1] > 50  # molecules do move
    with counting.MoleculeCounter(nw, L, capacity_hint=1 << 12, read_counts=True, features=nf) as mc:
        mc.update(index, umi, features=feature)
        _same(mc, snaps[0], nw, True)  # row sums against counts() and collapse(), matrix() twice
        # pairs(features=True) grouped on the host gives the same matrix
        pi, pf, pu, pr = mc.pairs(features=True, reads=True)
        cell = pi.astype(np.int64) * nf + pf
        uniq, start, count = np.unique(cell, return_index=True, return_counts=True)
        indptr, mfeat, mol, rds = mc.matrix(reads=True)
        assert (uniq % nf).tolist() == mfeat.tolist() and count.tolist() == mol.tolist()
        assert np.add.reduceat(pr, start).tolist() == rds.tolist()
        assert np.searchsorted(uniq // nf, np.arange(nw + 1)).tolist() == indptr.tolist()


def test_device_forms():
    """update_device with feature_ptr on a side stream and matrix_device into torch tensors."""
    torch = pytest.importorskip("torch")
    nw, nf, kind, L, batches, snaps = _random_case()
    index, feature, umi = batches[0]
    d_index, d_feature = torch.from_numpy(index).cuda(), torch.from_numpy(feature).cuda()
    d_umi = torch.from_numpy(umi.view(np.int64)).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    indptr, mfeat, mol, rds, col = snaps[0]["matrix"]
    nnz = len(mfeat)
    with counting.MoleculeCounter(nw, L, capacity_hint=1 << 10, read_counts=True, features=nf) as mc:
        n = index.size
        mc.update_device(d_index.data_ptr(), d_umi.data_ptr(), n // 2, stream=side.cuda_stream,
                         feature_ptr=d_feature.data_ptr())
        mc.update_device(d_index.data_ptr() + 4 * (n // 2), d_umi.data_ptr() + 8 * (n // 2), n - n // 2,
                         feature_ptr=d_feature.data_ptr() + 4 * (n // 2))
        room = nnz + 5
        o_indptr = torch.full((nw + 1,), -1, dtype=torch.int64, device="cuda")
        o_feat = torch.full((room,), -7, dtype=torch.int32, device="cuda")
        o_val = torch.full((3, room), -7, dtype=torch.int64, device="cuda")
        got = mc.matrix_device(o_indptr.data_ptr(), o_feat.data_ptr(), o_val[0].data_ptr(), o_val[1].data_ptr(),
                               o_val[2].data_ptr(), room, stream=side.cuda_stream)
        torch.cuda.synchronize()
        assert got == nnz
        assert o_indptr.cpu().tolist() == indptr and o_feat[:nnz].cpu().tolist() == mfeat
        assert o_val[:, :nnz].cpu().tolist() == [mol, rds, col]
        assert (o_feat[nnz:] == -7).all() and (o_val[:, nnz:] == -7).all()  # nothing past nnz
        # only the molecules, no reads and no collapsed
        o_val.fill_(-7)
        assert mc.matrix_device(o_indptr.data_ptr(), o_feat.data_ptr(), o_val[0].data_ptr(), None, 0, nnz) == nnz
        torch.cuda.synchronize()
        assert o_val[0, :nnz].cpu().tolist() == mol and (o_val[1:] == -7).all()
        with pytest.raises(ValueError):
            mc.update_device(d_index.data_ptr(), d_umi.data_ptr(), 1)  # no feature_ptr


# ---- counted

def test_chains_under_two_features_do_not_interact():
    """The header's AA x 1, AC x 2, GC x 5 under feature 0, and AA x 1, AC x 2 under feature 2 of the
    same barcode, and the first chain again under another barcode."""
    nw, nf, kind, L = 3, 3, 3, 2
    AA, AC, GC = umi3(A, A), umi3(A, C), umi3(G, C)
    rows = [(1, 0, AA)] + [(1, 0, AC)] * 2 + [(1, 0, GC)] * 5 + [(1, 2, AA)] + [(1, 2, AC)] * 2
    rows += [(2, 0, AA)] + [(2, 0, AC)] * 2 + [(2, 0, GC)] * 5
    batches = [_from_rows(rows)]
    snaps = _reference(nw, nf, kind, L, batches)
    assert snaps[0]["matrix"] == ([0, 0, 2, 3], [0, 2, 0], [3, 2, 3], [8, 3, 8], [2, 1, 2])
    assert snaps[0]["collapse"] == ([0, 3, 2], 5)
    for preagg in PREAGG:
        _run(nw, nf, kind, L, batches, snaps, counted=True, preagg=preagg)


def test_reads_and_collapsed_need_read_counts():
    with counting.MoleculeCounter(5, 4, features=3, capacity_hint=64) as mc:
        mc.update([0, 1], [umi3(A, A, A, A)] * 2, features=[1, 2])
        before = _matrix_lists(mc.matrix())
        for kw in ({"reads": True}, {"collapsed": True}):
            with pytest.raises(ValueError, match="read_counts"):
                mc.matrix(**kw)
        with pytest.raises(ValueError, match="read_counts"):
            mc.pairs(features=True, reads=True)
        buf = np.zeros(8, dtype=np.uint64)
        nnz = ctypes.c_int64(-1)
        p = _lib._ptr(buf)
        assert mc._lib.sct_molecules_matrix_host(mc._h, p, p, None, p, None, 8, ctypes.byref(nnz)) == _lib.SCT_E_INVALID
        assert mc._lib.sct_molecules_matrix_host(mc._h, p, p, None, None, p, 8, ctypes.byref(nnz)) == _lib.SCT_E_INVALID
        assert mc._lib.sct_molecules_fetch_features_host(mc._h, p, p, p, p, None, 8) == _lib.SCT_E_INVALID
        assert nnz.value == -1 and not buf.any()
        assert _matrix_lists(mc.matrix()) == before == ([0, 1, 2, 2, 2, 2], [1, 2], [1, 1])


# ---- merge

@pytest.mark.parametrize("rows_route", [0, 1])
@pytest.mark.parametrize("counted", [False, True])
def test_merge_of_alternate_pieces(counted, rows_route):
    """Two feature counters fed alternate pieces, merged with the table read in place and through
    the compacted rows (the route between two devices), give the one counter's matrix."""
    nw, nf, kind, L, batches, snaps = _random_case()
    index, feature, umi = (a[:6000] for a in batches[0])
    whole = M.FeatureMolecules(nw, nf, kind, L).update(index, umi, feature)
    make = lambda: counting.MoleculeCounter(nw, L, capacity_hint=64, read_counts=counted, features=nf)  # noqa: E731
    with make() as a, make() as b, _lib.tuning(merge_rows=rows_route):
        for piece in range(0, 6000, 1000):
            target = a if (piece // 1000) % 2 == 0 else b
            s = slice(piece, piece + 1000)
            target.update(index[s], umi[s], features=feature[s])
        b_before = _matrix_lists(b.matrix())
        assert a.merge(b) is a
        _same(a, _snap(whole), nw, counted)
        assert _matrix_lists(b.matrix()) == b_before  # the source is unchanged


def test_merge_needs_equal_nf():
    AAAA = umi3(A, A, A, A)
    with counting.MoleculeCounter(5, 4, features=3, capacity_hint=64) as a, \
            counting.MoleculeCounter(5, 4, features=4, capacity_hint=64) as b, \
            counting.MoleculeCounter(5, 4, capacity_hint=64) as plain:
        a.update([0, 1], [AAAA] * 2, features=[1, 2])
        b.update([0], [AAAA], features=[3])
        plain.update([0], [AAAA])
        before = (_matrix_lists(a.matrix()), a.info(), a.counts()[0].tolist())
        for other in (b, plain):
            with pytest.raises(ValueError, match="features"):
                a.merge(other)
            assert a._lib.sct_molecules_merge(a._h, other._h, None) == _lib.SCT_E_INVALID
            assert "nf differ" in _lib.last_error()
            assert plain._lib.sct_molecules_merge(other._h, a._h, None) == _lib.SCT_E_INVALID
        assert (_matrix_lists(a.matrix()), a.info(), a.counts()[0].tolist()) == before
        assert len(b) == 1 and len(plain) == 1


# ---- the update form must be the counter's

def test_wrong_update_form_changes_nothing():
    AAAA = umi3(A, A, A, A)
    index, feature = np.array([0, 1], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    umi = np.array([AAAA, AAAA], dtype=np.uint64)
    with counting.MoleculeCounter(5, 4, features=3, capacity_hint=64) as mc, \
            counting.MoleculeCounter(5, 4, capacity_hint=64) as plain:
        with pytest.raises(ValueError, match="features"):
            mc.update(index, umi)
        with pytest.raises(ValueError, match="features"):
            plain.update(index, umi, features=feature)
        with pytest.raises(ValueError, match="differ in length"):
            mc.update(index, umi, features=feature[:1])
        lib, p = mc._lib, _lib._ptr
        assert lib.sct_molecules_update_host(mc._h, p(index), p(umi), 2) == _lib.SCT_E_INVALID
        assert "feature" in _lib.last_error()
        assert lib.sct_molecules_update_features_host(plain._h, p(index), p(feature), p(umi), 2) == _lib.SCT_E_INVALID
        assert "no features" in _lib.last_error()
        nnz = ctypes.c_int64(0)
        assert lib.sct_molecules_matrix_host(plain._h, p(index), p(feature), None, None, None, 2,
                                             ctypes.byref(nnz)) == _lib.SCT_E_INVALID
        with pytest.raises(ValueError):
            plain.matrix()
        with pytest.raises(ValueError):
            plain.pairs(features=True)
        for c in (mc, plain):
            assert c.info()["total"] == 0 and len(c) == 0 and c.counts()[0].sum() == 0
        assert plain.features is None and plain.n_no_feature == 0 and mc.features == 3
