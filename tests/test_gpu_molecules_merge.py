"""Merging molecule counters on the device (sct_molecules_merge, MoleculeCounter.merge): after
a.merge(b), a is the counter that was fed a's reads and then b's, so the expected result is
tests/molecules_reference.py / tests/umi_collapse_reference.py fed the concatenation.  Every
comparison is exact equality of integers and of order; there is no tolerance anywhere.  All shapes
are a few thousand reads, and a case's input and reference are computed once for its forms."""

import functools

import numpy as np
import pytest

import test_gpu_molecules as M
import umi_collapse_reference as U
from sctools_amd import _lib, counting

pytestmark = pytest.mark.gpu

PREAGG = [0, 1, 2]  # the feeding updates: none, wave merge, LDS table
ENC = {3: "ThreeBit", 2: "TwoBit"}
C, A, G, T = 1, 2, 3, 4


def umi3(*bases):
    """A ThreeBit code written first base first (the first base in the high triplet)."""
    code = 0
    for b in bases:
        code = (code << 3) | b
    return code


def _arrays(reads):
    return (np.array([r[0] for r in reads], dtype=np.int32), np.array([r[1] for r in reads], dtype=np.uint64))


def _ref(nw, kind, L, *batches):
    ref = U.CountedMolecules(nw, kind, L)
    for index, umis in batches:
        ref.update(index, umis)
    return ref


def _snap(ref, parents=True):
    """Everything a counter is compared with, taken from the reference as it stands.  parents=False
    leaves the parents and the collapse out (the reference walks 3 * L neighbours per molecule in
    Python): rows are then (index, umi, reads)."""
    if parents:
        rows, collapse = ref.pairs_counted(), ref.collapse()
    else:
        rows, collapse = [(i, u, ref.mreads[(i, u)]) for (i, u) in sorted(ref.mreads)], None
    return {"counts": ref.counts(), "rows": rows, "collapse": collapse, "total": ref.total}


def _same(mc, snap):
    """counts(), pairs(), info() and, for a counter with read counts, pairs(reads, parents) and
    collapse() of the device counter = the reference's."""
    reads, molecules, n_none, n_amb, n_bad = mc.counts()
    assert (reads.tolist(), molecules.tolist(), n_none, n_amb, n_bad) == snap["counts"]
    rows = snap["rows"]
    index, umi = mc.pairs()
    assert list(zip(index.tolist(), umi.tolist())) == [r[:2] for r in rows]
    info = mc.info()
    assert info["nmolecules"] == len(rows) == len(mc) == int(molecules.sum()) and info["total"] == snap["total"]
    if mc.read_counts and snap["collapse"] is None:
        assert list(zip(*(a.tolist() for a in mc.pairs(reads=True)))) == rows
    elif mc.read_counts:
        four = mc.pairs(reads=True, parents=True)
        assert list(zip(*(a.tolist() for a in four))) == rows
        collapsed, n_corrected = mc.collapse()
        assert (collapsed.tolist(), n_corrected) == snap["collapse"]
    return info


def _state(mc):
    """What a counter shows, as plain Python values (to compare a counter with itself later)."""
    reads, molecules, n_none, n_amb, n_bad = mc.counts()
    out = [reads.tolist(), molecules.tolist(), n_none, n_amb, n_bad, mc.info()]
    out.append([a.tolist() for a in (mc.pairs(reads=True) if mc.read_counts else mc.pairs())])
    return out


def _counter(nw, kind, L, counted, batches=(), **kw):
    mc = counting.MoleculeCounter(nw, L, encoding=ENC[kind], read_counts=counted, **kw)
    for index, umis in batches:
        mc.update(index, umis)
    return mc


@functools.lru_cache(maxsize=None)
def _overlap():
    """ThreeBit L = 4 under 7 barcodes: 900 molecules, a third fed to `a` only, a third to `b` only, a
    third to both (their reads split at random), 1-8 reads each; no-match, ambiguous and bad-UMI reads
    on both sides.  (nw, kind, L, a's reads, b's reads, snapshot of a alone, of b alone, of both)."""
    nw, kind, L = 7, 3, 4
    rng = np.random.default_rng(2024)
    codes = rng.permutation(4 ** L * nw)[:900]
    mol_i = (codes % nw).astype(np.int32)
    mol_u = np.zeros(900, dtype=np.uint64)
    for p in range(L):
        mol_u |= ((((codes // nw) >> (2 * p)) & 3) + 1).astype(np.uint64) << np.uint64(3 * p)
    rows = np.repeat(np.arange(900), rng.integers(1, 9, size=900))
    rows = rng.permutation(rows)
    side = np.where(rows % 3 == 0, 0, np.where(rows % 3 == 1, 1, rng.integers(0, 2, size=rows.size)))
    index, umis = mol_i[rows].copy(), mol_u[rows].copy()
    extra = rng.random(rows.size)
    index[extra < 0.04] = -1
    index[(extra >= 0.04) & (extra < 0.06)] = -2
    umis[(extra >= 0.06) & (extra < 0.08)] |= np.uint64(6)  # an N in the last base
    in_a = side == 0
    a, b = (index[in_a], umis[in_a]), (index[~in_a], umis[~in_a])
    ra, rb, rab = _ref(nw, kind, L, a), _ref(nw, kind, L, b), _ref(nw, kind, L, a, b)
    only_a, only_b, both = ra.seen - rb.seen, rb.seen - ra.seen, ra.seen & rb.seen
    assert 3500 <= rows.size <= 4500 and min(len(only_a), len(only_b), len(both)) >= 200
    assert sum(rab.molecules) < sum(ra.molecules) + sum(rb.molecules)  # adding molecules[] up would be wrong
    assert all(t > 0 for t in ra.tally + rb.tally)
    return nw, kind, L, a, b, _snap(ra), _snap(rb), _snap(rab)


@pytest.mark.parametrize("preagg", PREAGG)
@pytest.mark.parametrize("counted", [False, True])
def test_overlap(counted, preagg):
    """Molecules only in dst, only in src and in both: counts() and pairs() after the merge are the
    reference's on all reads, and with read counts so are every molecule's reads, its parent and the
    collapse.  merge returns the counter it was called on."""
    nw, kind, L, a, b, snap_a, snap_b, snap_ab = _overlap()
    with _lib.tuning(count_preagg=preagg):
        with _counter(nw, kind, L, counted, [a], capacity_hint=64) as ca, \
                _counter(nw, kind, L, counted, [b], capacity_hint=64) as cb:
            _same(ca, snap_a)
            assert ca.merge(cb) is ca
            _same(ca, snap_ab)
            _same(cb, snap_b)


@pytest.mark.parametrize("counted", [False, True])
def test_compacted_rows_give_the_same(counted):
    """SCT_TUNE_MERGE_ROWS 1: the source's occupied rows are compacted and copied into scratch first,
    the route two devices always take, here on one; every number as with the table read in place,
    and an empty source on that route."""
    nw, kind, L, a, b, snap_a, snap_b, snap_ab = _overlap()
    assert _lib.tune_get("merge_rows") == -1  # every other test runs the default
    with _lib.tuning(merge_rows=1):
        with _counter(nw, kind, L, counted, [a], capacity_hint=64) as ca, \
                _counter(nw, kind, L, counted, [b], capacity_hint=64) as cb, _counter(nw, kind, L, counted) as empty:
            ca.merge(empty).merge(cb)
            _same(ca, snap_ab)
            _same(cb, snap_b)
            _same(empty.merge(cb), snap_b)


def test_a_parent_flips_by_merge():
    """dst holds AC x 2 and GC x 1, so GC collapses into AC; src brings GC x 5 and AA x 1, after which
    AC collapses into GC and AA into AC: the collapse is valid across shards only because mreads add."""
    dst_reads = [(0, umi3(A, C))] * 2 + [(0, umi3(G, C))]
    src_reads = [(0, umi3(G, C))] * 5 + [(0, umi3(A, A))]
    with _counter(1, 3, 2, True, [_arrays(dst_reads)], capacity_hint=64) as dst, \
            _counter(1, 3, 2, True, [_arrays(src_reads)], capacity_hint=64) as src:
        before = dict(zip(dst.pairs(reads=True, parents=True)[1].tolist(), dst.pairs(reads=True, parents=True)[3].tolist()))
        assert before == {umi3(A, C): umi3(A, C), umi3(G, C): umi3(A, C)}
        assert dst.collapse()[0].tolist() == [1] and dst.collapse()[1] == 1
        dst.merge(src)
        index, umi, mreads, parent = dst.pairs(reads=True, parents=True)
        got = {u: (r, p) for u, r, p in zip(umi.tolist(), mreads.tolist(), parent.tolist())}
        assert got == {umi3(A, A): (1, umi3(A, C)), umi3(A, C): (2, umi3(G, C)), umi3(G, C): (6, umi3(G, C))}
        collapsed, n_corrected = dst.collapse()
        assert collapsed.tolist() == [2] and n_corrected == 2
        _same(dst, _snap(_ref(1, 3, 2, _arrays(dst_reads), _arrays(src_reads))))


@functools.lru_cache(maxsize=None)
def _growth():
    """TwoBit L = 28 under 37 barcodes: `few` = 10 molecules (five of them also among the many), `many` =
    about 5,000 distinct molecules of the arange, high_bits and random families, 1-3 reads each."""
    nw, kind, L = 37, 2, 28
    rng = np.random.default_rng(77)
    parts = [M._family("arange", 2000, rng), M._family("high_bits", 1500, rng), M._family("random", 1500, rng)]
    mol_i, mol_u = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    rows = rng.permutation(np.repeat(np.arange(mol_i.size), rng.integers(1, 4, size=mol_i.size)))
    many = (mol_i[rows], mol_u[rows])
    few = (np.concatenate([mol_i[:5], np.arange(5, dtype=np.int32)]),
           np.concatenate([mol_u[:5], np.arange(2 ** 55, 2 ** 55 + 5, dtype=np.uint64)]))
    r_few, r_many = _ref(nw, kind, L, few), _ref(nw, kind, L, many)
    assert len(r_few.seen) == 10 and 4900 <= len(r_many.seen) <= 5000 and len(r_few.seen & r_many.seen) == 5
    # (the parents of 5,000 molecules with 84 neighbours each are test_overlap's subject, on fewer)
    return (nw, kind, L, few, many, _snap(_ref(nw, kind, L, few, many), parents=False),
            _snap(_ref(nw, kind, L, many, few), parents=False))


@pytest.mark.parametrize("counted", [False, True])
def test_growth(counted):
    """A 64-slot counter of 10 molecules takes in about 5,000: it is grown first, by at least four
    doublings, to a load of at most 1/2, and the rehash adds nothing to molecules.  src's table is
    larger than dst's there; then smaller (a roomy dst does not grow), and the other way round."""
    nw, kind, L, few, many, snap_few_many, snap_many_few = _growth()
    nmol = len(snap_few_many["rows"])
    with _counter(nw, kind, L, counted, [many], capacity_hint=64) as src:
        src_cap = src.info()["capacity"]
        with _counter(nw, kind, L, counted, [few], capacity_hint=64) as dst:
            assert dst.info()["capacity"] == 64 < src_cap
            info = _same(dst.merge(src), snap_few_many)
            cap = info["capacity"]
            assert cap >= 64 * 2 ** 4 and cap & (cap - 1) == 0 and 2 * nmol <= cap < 4 * nmol
            assert int(dst.counts()[1].sum()) == len(dst) == nmol
        with _counter(nw, kind, L, counted, [few], capacity_hint=1 << 17) as dst:
            assert dst.info()["capacity"] == 1 << 17 > src_cap
            assert _same(dst.merge(src), snap_few_many)["capacity"] == 1 << 17
        with _counter(nw, kind, L, counted, [few], capacity_hint=64) as small:  # the large one takes the small one
            assert _same(src.merge(small), snap_many_few)["capacity"] == src_cap
            assert int(src.counts()[1].sum()) == len(src) == nmol


@pytest.mark.parametrize("counted", [False, True])
def test_corners(counted):
    """Key 0 (index 0, the all-A TwoBit UMI) and the 63-bit key (TwoBit L = 24, nw = 32768, index
    32767, the all-T UMI) present only in src; an empty src, an empty dst, both empty; and a src that
    holds tallies and no molecule, whose tallies and total still add."""
    nw, kind, L = 2 ** 15, 2, 24
    top = 2 ** 48 - 1
    mid = _arrays([(5, 77), (5, 77), (32767, top - 1), (0, 1), (-1, 3)])
    ends = _arrays([(0, 0), (32767, top), (32767, top), (5, 77), (-2, 0)])
    tallies = _arrays([(-1, 5), (-2, 6), (-2, 7), (3, 2 ** 48), (4, 2 ** 63)])  # the last two: bad UMIs
    with _counter(nw, kind, L, counted, [mid], capacity_hint=64) as dst, \
            _counter(nw, kind, L, counted, [ends], capacity_hint=64) as src:
        _same(dst.merge(src), _snap(_ref(nw, kind, L, mid, ends)))
        index, umi = dst.pairs()
        assert (int(index[0]), int(umi[0])) == (0, 0) and (int(index[-1]), int(umi[-1])) == (32767, top)
        with _counter(nw, kind, L, counted) as empty, _counter(nw, kind, L, counted) as empty2:
            _same(dst.merge(empty), _snap(_ref(nw, kind, L, mid, ends)))  # an empty src changes nothing
            _same(empty.merge(empty2), _snap(_ref(nw, kind, L)))  # both empty
            _same(empty2, _snap(_ref(nw, kind, L)))
            _same(empty.merge(src), _snap(_ref(nw, kind, L, ends)))  # an empty dst becomes src
        with _counter(nw, kind, L, counted, [tallies], capacity_hint=64) as only_tallies:
            assert len(only_tallies) == 0 and only_tallies.counts()[2:] == (1, 2, 2)
            snap = _snap(_ref(nw, kind, L, mid, ends, tallies))
            assert snap["counts"][2:] == (2, 3, 2) and snap["total"] == 15
            _same(dst.merge(only_tallies), snap)


@pytest.mark.parametrize("counted", [False, True])
def test_src_is_untouched_and_merges_compose(counted):
    """src shows the same counts(), pairs and info() before and after; merging it twice doubles reads,
    mreads, the tallies and total and leaves molecules alone; both counters take further updates and
    stay right; and (a <- b) <- c equals a <- (b <- c)."""
    nw, kind, L, a, b, snap_a, snap_b, snap_ab = _overlap()
    c = (a[0][::3].copy(), a[1][::3] ^ np.uint64(1 << 3))  # a's every third read, a bit of its last-but-one base flipped: new molecules, and bad UMIs
    with _counter(nw, kind, L, counted, [a], capacity_hint=64) as ca, \
            _counter(nw, kind, L, counted, [b], capacity_hint=64) as cb:
        before = _state(cb)
        ca.merge(cb)
        assert _state(cb) == before
        _same(ca.merge(cb), _snap(_ref(nw, kind, L, a, b, b)))
        assert _state(cb) == before
        reads1, molecules1 = snap_ab["counts"][:2]
        reads2, molecules2, n_none, n_amb, n_bad = ca.counts()
        assert molecules2.tolist() == molecules1
        assert reads2.tolist() == [x + y for x, y in zip(reads1, snap_b["counts"][0])]
        assert (n_none, n_amb, n_bad) == tuple(x + y for x, y in zip(snap_ab["counts"][2:], snap_b["counts"][2:]))
        assert ca.info()["total"] == snap_ab["total"] + snap_b["total"]
        if counted:
            once = {r[:2]: r[2] for r in snap_ab["rows"]}
            twice = dict(zip(zip(*(x.tolist() for x in ca.pairs())), ca.pairs(reads=True)[2].tolist()))
            in_b = {r[:2]: r[2] for r in snap_b["rows"]}
            assert twice == {k: v + in_b.get(k, 0) for k, v in once.items()}
        _same(ca.update(*c), _snap(_ref(nw, kind, L, a, b, b, c)))
        _same(cb.update(*c), _snap(_ref(nw, kind, L, b, c)))
    with _counter(nw, kind, L, counted, [a], capacity_hint=64) as left, \
            _counter(nw, kind, L, counted, [b], capacity_hint=64) as mid, \
            _counter(nw, kind, L, counted, [c], capacity_hint=64) as right, \
            _counter(nw, kind, L, counted, [a], capacity_hint=64) as left2:
        left.merge(mid).merge(right)  # (a <- b) <- c
        left2.merge(mid.merge(right))  # a <- (b <- c)
        assert _state(left)[:5] == _state(left2)[:5] and _state(left)[6] == _state(left2)[6]
        assert left.info()["nmolecules"] == left2.info()["nmolecules"] and left.info()["total"] == left2.info()["total"]
        _same(left, _snap(_ref(nw, kind, L, a, b, c)))


def test_errors_leave_dst_as_it_was():
    """Self-merge, another nw, kind, L, read counts against none, a closed counter and something that
    is no counter: ValueError (TypeError for the last) whose message names what differs, from the C
    entry point too, and dst's counts() and pairs() stay."""
    nw, kind, L, a, b, snap_a, _, _ = _overlap()
    lib = _lib.lib()
    with _counter(nw, kind, L, False, [a], capacity_hint=64) as dst:
        before = _state(dst)
        others = {"whitelist_size": (_counter(nw + 1, kind, L, False), "nw"),
                  "encoding": (_counter(nw, 2, L, False), "kind"),
                  "umi_length": (_counter(nw, kind, L + 1, False), "L differ"),
                  "read_counts": (_counter(nw, kind, L, True), "read counts")}
        try:
            for word, (other, c_word) in others.items():
                other.update(*_arrays([(1, 0)]))
                with pytest.raises(ValueError, match=word):
                    dst.merge(other)
                assert lib.sct_molecules_merge(dst._h, other._h, None) == _lib.SCT_E_INVALID
                assert c_word in _lib.last_error(), _lib.last_error()
                assert _state(dst) == before
        finally:
            for other, _ in others.values():
                other.close()
        with pytest.raises(ValueError, match="itself"):
            dst.merge(dst)
        assert lib.sct_molecules_merge(dst._h, dst._h, None) == _lib.SCT_E_INVALID and "itself" in _lib.last_error()
        assert lib.sct_molecules_merge(dst._h, None, None) == _lib.SCT_E_INVALID and "NULL" in _lib.last_error()
        assert lib.sct_molecules_merge(None, dst._h, None) == _lib.SCT_E_INVALID
        closed = _counter(nw, kind, L, False, [b])
        closed.close()
        with pytest.raises(ValueError, match="closed"):
            dst.merge(closed)
        with pytest.raises(ValueError, match="closed"):
            closed.merge(dst)
        for thing in (None, 7, [dst], "counter", (a[0], a[1])):
            with pytest.raises(TypeError):
                dst.merge(thing)
        assert _state(dst) == before
        _same(dst, snap_a)


@pytest.mark.parametrize("counted", [False, True])
def test_ordering_across_streams(counted):
    """src is fed through update_device on one torch stream and merged on another with no
    synchronisation in between; then src is fed again on the first stream straight after the merge,
    which has to wait for the merge's reads of src."""
    torch = pytest.importorskip("torch")
    nw, kind, L, a, b, snap_a, snap_b, snap_ab = _overlap()
    d_index, d_umi = torch.from_numpy(b[0]).cuda(), torch.from_numpy(b[1].view(np.int64)).cuda()
    one, two = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with _counter(nw, kind, L, counted, [a], capacity_hint=64) as dst, _counter(nw, kind, L, counted) as src:
        src.update_device(d_index.data_ptr(), d_umi.data_ptr(), b[0].size, stream=one.cuda_stream)
        assert dst.merge_device(src, stream=two.cuda_stream) is dst
        src.update_device(d_index.data_ptr(), d_umi.data_ptr(), b[0].size, stream=one.cuda_stream)
        _same(dst, snap_ab)
        _same(src, _snap(_ref(nw, kind, L, b, b)))
        torch.cuda.synchronize()


def test_an_explicit_device():
    """MoleculeCounter(device=0) is the default counter on a one-GPU box, the current device stays
    what it was through every call, and a device that does not exist is a ValueError."""
    torch = pytest.importorskip("torch")
    nw, kind, L, a, b, snap_a, snap_b, snap_ab = _overlap()
    current = torch.cuda.current_device()
    with counting.MoleculeCounter(nw, L, capacity_hint=64, read_counts=True, device=0) as ca, \
            counting.MoleculeCounter(nw, L, capacity_hint=64, read_counts=True) as cb:
        assert ca.device == 0 and cb.device is None
        ca.update(*a)
        cb.update(*b)
        _same(ca.merge(cb), snap_ab)
        assert torch.cuda.current_device() == current
    with pytest.raises(ValueError, match="device"):
        counting.MoleculeCounter(nw, L, device=_lib.device_count())
    with pytest.raises(ValueError):
        counting.MoleculeCounter(nw, L, device=-1)
    h = counting._vp()
    assert _lib.lib().sct_molecules_create_ex(nw, kind, L, 64, 2, -1, counting.ctypes.byref(h)) == _lib.SCT_E_INVALID
    assert "flags" in _lib.last_error() and not h


@pytest.mark.parametrize("counted", [False, True])
def test_two_devices(counted):
    """A counter on device 0 and one on device 1, merged in both directions, whichever of the two
    devices is current; the current device after every call is the one before it."""
    torch = pytest.importorskip("torch")
    if _lib.device_count() < 2:
        pytest.skip("needs two devices")
    nw, kind, L, a, b, snap_a, snap_b, snap_ab = _overlap()
    snap_ba = _snap(_ref(nw, kind, L, b, a))
    for current in (0, 1):
        with torch.cuda.device(current):
            def same_device(result=None):
                assert torch.cuda.current_device() == current
                return result
            with same_device(_counter(nw, kind, L, counted, capacity_hint=64, device=0)) as c0, \
                    same_device(_counter(nw, kind, L, counted, capacity_hint=64, device=1)) as c1:
                same_device(c0.update(*a))
                same_device(c1.update(*b))
                _same(c0, snap_a)
                _same(c1, snap_b)
                same_device()
                same_device(c0.merge(c1))  # 1 -> 0
                _same(c0, snap_ab)
                _same(c1, snap_b)
                same_device()
                with _counter(nw, kind, L, counted, [a], capacity_hint=64, device=0) as again:
                    same_device(c1.merge(again))  # 0 -> 1
                    _same(c1, snap_ba)
                    _same(again, snap_a)
                same_device()
