"""Removing swapped molecules on the device (sct_molecules_swapped, counting.remove_swapped and
MoleculeCounter.remove_swapped_device) against tests/swapped_reference.py, the contract in plain
Python, applied to the references of the counters themselves.  Every comparison is exact equality of
integers and of order; there is no tolerance anywhere.  A case is a few thousand reads (the heavy
molecules: about 200,000, two small batches), and its input and references are computed once."""

import ctypes
import functools

import numpy as np
import pytest

import count_matrix_reference as CM
import downsample_reference as D
import molecules_reference as R
import swapped_reference as S
import test_gpu_count_matrix as F
import test_gpu_downsample as DS
import test_gpu_molecules_merge as MM
import test_swapped_reference_host as H
from sctools_amd import _lib, counting

pytestmark = pytest.mark.gpu

ENC = MM.ENC
FRACTIONS = H.FRACTIONS


def _counter(ref, batches=(), hint=64):
    return MM._counter(ref.nw, ref.kind, ref.L, True, batches, capacity_hint=hint)


def _close(counters):
    for c in counters:
        c.close()


def _check(sources, refs, num, den):
    """remove_swapped of the device counters = the reference's, sample by sample: counts, rows with
    reads and parents, info with total, both collapses, the tally; the sources as they were; and the
    README's identities.  Returns the cleaned references."""
    before = [MM._state(c) for c in sources]
    want, want_tally = H.cleaned(list(refs), num, den)
    cleaned, tally = counting.remove_swapped(sources, min_fraction=(num, den))
    try:
        assert tally.dtype == np.int64 and tally.shape == (len(sources), 3) and tally.tolist() == want_tally
        assert len(cleaned) == len(sources)
        for got, src, ref in zip(cleaned, sources, want):
            assert got is not src and got.read_counts and got.features is None
            assert (got.size, got.kind, got.umi_length, got.device) == (src.size, src.kind, src.umi_length, src.device)
            info = DS._same(got, DS._snap(ref))
            assert info["capacity"] == DS.merge_capacity(64, 0, len(ref.mreads))
        assert [MM._state(c) for c in sources] == before
        assert sum(int(c.counts()[0].sum()) for c in cleaned) + int(tally[:, 2].sum()) == \
            sum(int(c.counts()[0].sum()) for c in sources)
        keys = [set(zip(*(a.tolist() for a in c.pairs()))) for c in cleaned]
        assert sum(len(k) for k in keys) == len(set().union(*keys))  # a key is stored in at most one
    finally:
        _close(cleaned)
    return want


# ---- the base case: the two overlapping halves of test_gpu_molecules_merge, 227 keys in both


@pytest.fixture(scope="module")
def base_counters():
    (a, b), (ra, rb) = H.base()
    with _counter(ra, [a]) as ca, _counter(rb, [b]) as cb:
        yield ca, cb


@pytest.mark.parametrize("num,den", FRACTIONS)
def test_base_case(base_counters, num, den):
    _, refs = H.base()
    want = _check(list(base_counters), refs, num, den)
    both = set(refs[0].mreads) & set(refs[1].mreads)
    kept = [len(both & set(w.mreads)) for w in want]
    if (num, den) == (4, 5):
        assert kept == [10, 18]
    if (num, den) == (1, 1):
        assert kept == [0, 0] and all(len(w.mreads) > 200 for w in want)


# ---- s = 1, 3 and 16


@functools.lru_cache(maxsize=None)
def _dealt(s):
    """The base case's reads dealt over s samples at random, and six more molecules forced into every
    sample: three with (13, 1, 1, ...) reads and three with (60, 1, 1, ...), each heavy in another
    sample -- at s = 16 the first kind is dropped by all and the second sits at 60 / 75 = 4 / 5."""
    (a, b), (ra, rb) = H.base()
    index, umis = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    rng = np.random.default_rng(100 + s)
    side = rng.integers(0, s, size=index.size)
    unused = [(i, MM.umi3(MM.T, x, y, z)) for i in range(ra.nw) for x in (1, 2, 3, 4) for y in (1, 2, 3, 4)
              for z in (1, 2, 3, 4)]
    forced = [k for k in unused if k not in ra.mreads and k not in rb.mreads][::7][:6]
    assert len(forced) == 6
    batches = []
    for t in range(s):
        extra = []
        for j, (i, u) in enumerate(forced):
            heavy = (13 if j < 3 else 60) if t == (5 * j) % s else 1
            extra += [(i, u)] * heavy
        ei, eu = MM._arrays(extra)
        batches.append((np.concatenate([index[side == t], ei]), np.concatenate([umis[side == t], eu])))
    refs = [H.fed(ra.nw, ra.kind, ra.L, batch) for batch in batches]
    for i, u in forced:
        assert all((i, u) in r.mreads for r in refs)
    return batches, refs, forced


@pytest.mark.parametrize("s", [1, 3, 16])
def test_samples(s):
    """One sample is a copy; with 3 and 16 `others` sums over many tables, for keys stored in all."""
    batches, refs, _ = _dealt(s)
    sources = [_counter(r, [batch]) for r, batch in zip(refs, batches)]
    try:
        want = _check(sources, refs, 4, 5)
        if s == 1:
            assert H.shown(want[0]) == H.shown(refs[0])
        else:
            most = max(sum(k in r.mreads for r in refs) for k in refs[0].mreads)
            assert most == s
    finally:
        _close(sources)


def test_sixteen_samples_at_equality():
    """(60, 1, 1, ...) over 16 samples: 60 * 1 >= 4 * 15 keeps, in the heavy sample only; (13, 1, ...)
    keeps nowhere."""
    _, refs, forced = _dealt(16)
    want, _ = H.cleaned(refs, 4, 5)
    assert [sum(k in w.mreads for w in want) for k in forced] == [0, 0, 0, 1, 1, 1]


# ---- table shapes


def test_tables_of_64_slots_beside_grown_ones():
    """A sample in the smallest table (64 slots, one wave) beside one that grew to at least two
    workgroups' worth of slots and one made large: find runs under three masks in one launch."""
    (a, b), (ra, rb) = H.base()
    few = (np.concatenate([a[0][:12], b[0][:12]]), np.concatenate([a[1][:12], b[1][:12]]))
    rf = H.fed(ra.nw, ra.kind, ra.L, few)
    assert set(rf.mreads) & set(ra.mreads) and set(rf.mreads) & set(rb.mreads)
    with _counter(ra, [a]) as fed, _counter(ra) as ca, _counter(rf, [few]) as cf, \
            _counter(rb, [b], hint=1 << 14) as cb:
        ca.merge(fed)  # grown by merge's rule: 563 molecules take 2048 slots
        caps = [c.info()["capacity"] for c in (ca, cf, cb)]
        assert caps == [2048, 64, 1 << 14]
        _check([ca, cf, cb], [ra, rf, rb], 4, 5)
        _check([cf, cb, ca], [rf, rb, ra], 2, 3)


def test_a_table_at_a_load_just_under_a_half():
    """b cut to 508 molecules and merged into a 64-slot counter: 1024 slots at a load of 0.496.  Two of
    the keys a probes there share a home slot, so one hit is displaced, and a key of a that is not
    stored there has the home slot of one that is, so a miss walks a chain to an EMPTY slot."""
    (a, b), (ra, rb) = H.base()
    both = sorted(set(ra.mreads) & set(rb.mreads))
    chosen = set(both + sorted(set(rb.mreads) - set(ra.mreads))[:508 - len(both)])
    assert len(chosen) == 508
    keep = np.array([i < 0 or (i, u) in chosen or R.umi_is_bad(u, rb.kind, rb.L)
                     for i, u in zip(b[0].tolist(), b[1].tolist())])
    cut = (b[0][keep], b[1][keep])
    rc = H.fed(rb.nw, rb.kind, rb.L, cut)
    assert set(rc.mreads) == chosen

    def home(k):
        return D.mix64(R.key(k[0], k[1], rb.kind, rb.L)) & 1023
    homes = [home(k) for k in both]
    assert len(set(homes)) < len(homes)  # two probed and stored keys with one home: one is displaced
    stored_homes = {home(k) for k in chosen}
    assert any(home(k) in stored_homes for k in set(ra.mreads) - chosen)  # a miss that meets a chain
    with _counter(ra, [a]) as ca, _counter(rc, [cut]) as fed, _counter(rc) as cc:
        cc.merge(fed)
        info = cc.info()
        assert info["capacity"] == 1024 and info["nmolecules"] == 508
        _check([ca, cc], [ra, rc], 4, 5)
        _check([cc, ca], [rc, ra], 2, 3)


# ---- heavy and light


def test_heavy_and_light():
    """100,000 reads in one sample against 1 in the other, both ways round, and 100,000 against
    25,000, which is equality at 4/5."""
    nw, kind, L = 7, 3, 4
    k1, k2, k3 = (2, MM.umi3(MM.A, MM.C, MM.G, MM.T)), (5, MM.umi3(MM.T, MM.G, MM.C, MM.A)), (0, MM.umi3(MM.C, MM.C, MM.C, MM.C))
    x = MM._arrays([k1] * 100000 + [k2] + [k3] * 100000)
    y = MM._arrays([k1] + [k2] * 100000 + [k3] * 25000)
    rx, ry = H.fed(nw, kind, L, x), H.fed(nw, kind, L, y)
    with _counter(rx, [x]) as cx, _counter(ry, [y]) as cy:
        want = _check([cx, cy], [rx, ry], 4, 5)
        assert want[0].mreads == {k1: 100000, k3: 100000} and want[1].mreads == {k2: 100000}
        want = _check([cx, cy], [rx, ry], 1, 1)
        assert not want[0].mreads and not want[1].mreads
        want = _check([cy, cx], [ry, rx], 5, 6)
        assert want[0].mreads == {k2: 100000} and want[1].mreads == {k1: 100000}


# ---- what is added to


def test_into_counters_that_hold_overlapping_molecules():
    """into[0] holds b's molecules and into[1] a's: the kept shared keys are there already, so mreads
    add and no molecule counts twice; the table is what merge's rule gives for the target's molecules
    plus the survivors.  Twice the same call: the same reads again and no molecule."""
    (a, b), (ra, rb) = H.base()
    nw, kind, L = ra.nw, ra.kind, ra.L
    into_refs = [H.fed(nw, kind, L, b), H.fed(nw, kind, L, a)]
    sizes = [len(r.mreads) for r in into_refs]
    clean, _ = H.cleaned([ra, rb], 4, 5)
    want_tally = [S.remove_swapped([ra, rb], k, 4, 5, into_refs[k]) for k in range(2)]
    assert any(k in rb.mreads for k in clean[0].mreads) and any(k in ra.mreads for k in clean[1].mreads)
    with _counter(ra, [a]) as ca, _counter(rb, [b]) as cb, _counter(rb, [b]) as ia, _counter(ra, [a]) as ib:
        before = [MM._state(c) for c in (ca, cb)]
        caps = [c.info()["capacity"] for c in (ia, ib)]
        got, tally = counting.remove_swapped([ca, cb], (4, 5), into=[ia, ib])
        assert got[0] is ia and got[1] is ib and tally.tolist() == want_tally
        for c, ref, cap, size, cl in zip((ia, ib), into_refs, caps, sizes, clean):
            assert DS._same(c, DS._snap(ref))["capacity"] == DS.merge_capacity(cap, size, len(cl.mreads))
        for k in range(2):
            S.remove_swapped([ra, rb], k, 4, 5, into_refs[k])
        molecules = [c.counts()[1].tolist() for c in (ia, ib)]
        assert ca.remove_swapped_device([cb], ia, 4, 5).tolist() == want_tally[0]
        assert cb.remove_swapped_device([ca], ib, 4, 5).tolist() == want_tally[1]
        for c, ref, m in zip((ia, ib), into_refs, molecules):
            DS._same(c, DS._snap(ref))
            assert c.counts()[1].tolist() == m
        assert [MM._state(c) for c in (ca, cb)] == before


# ---- other counter kinds


def test_feature_counter():
    """features=5: the reads of a feature case dealt over two samples, and one (index, UMI) under
    feature 1 in one sample and feature 2 in the other, which is not shared; under feature 4 in both
    it is."""
    ref, (index, feature, umi) = DS._features()
    nw, nf, kind, L = ref.nw, ref.nf, ref.kind, ref.L
    rng = np.random.default_rng(3)
    side = rng.integers(0, 2, size=index.size)
    u = int(umi[(index >= 0) & (feature >= 0) & ~np.array([R.umi_is_bad(int(x), kind, L) for x in umi])][0])
    extra = [(np.array([3] * 10, np.int32), np.array([1] * 9 + [4], np.int32), np.array([u] * 10, np.uint64)),
             (np.array([3] * 2, np.int32), np.array([2, 4], np.int32), np.array([u] * 2, np.uint64))]
    parts, refs = [], []
    for t in range(2):
        part = tuple(np.concatenate([x[side == t], e]) for x, e in zip((index, feature, umi), extra[t]))
        parts.append(part)
        refs.append(CM.FeatureMolecules(nw, nf, kind, L).update(part[0], part[2], part[1]))
    assert all(r.n_no_feature > 0 for r in refs)
    want, want_tally = H.cleaned(refs, 4, 5)
    sources = [counting.MoleculeCounter(nw, L, ENC[kind], capacity_hint=64, read_counts=True, features=nf)
               for _ in range(2)]
    try:
        for c, (i, f, m) in zip(sources, parts):
            c.update(i, m, features=f)
        before = [MM._state(c) for c in sources]
        cleaned, tally = counting.remove_swapped(sources)
        try:
            assert tally.tolist() == want_tally and 0 < want_tally[0][1] < want_tally[0][0]
            for got, w in zip(cleaned, want):
                assert got.features == nf
                F._same(got, F._snap(w), nw, True)
            if (3, 1, u) not in refs[1].mreads and (3, 2, u) not in refs[0].mreads:
                assert (3, 1, u) in want[0].mreads and (3, 2, u) in want[1].mreads
        finally:
            _close(cleaned)
        assert [MM._state(c) for c in sources] == before
    finally:
        _close(sources)


def test_twobit():
    ref, (index, umis) = DS._twobit()
    side = np.random.default_rng(4).integers(0, 2, size=index.size)
    batches = [(index[side == t], umis[side == t]) for t in range(2)]
    refs = [H.fed(ref.nw, ref.kind, ref.L, batch) for batch in batches]
    assert len(set(refs[0].mreads) & set(refs[1].mreads)) > 100
    with _counter(refs[0], [batches[0]]) as c0, _counter(refs[1], [batches[1]]) as c1:
        for num, den in ((4, 5), (2, 3)):
            want = _check([c0, c1], refs, num, den)
            assert all(0 < len(w.mreads) < len(r.mreads) for w, r in zip(want, refs))


# ---- ordering


def test_ordering_across_streams():
    """The other sample is fed through update_device on one torch stream and probed by the removal on
    another with no synchronisation in between; then it is fed again on the first stream straight
    after the call, which has to wait for the removal's reads of it."""
    torch = pytest.importorskip("torch")
    (a, b), (ra, rb) = H.base()
    d_index, d_umi = torch.from_numpy(b[0]).cuda(), torch.from_numpy(b[1].view(np.int64)).cuda()
    one, two = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    want = H.empty_like(ra)
    want_tally = S.remove_swapped([ra, rb], 0, 4, 5, want)
    with _counter(ra, [a]) as ca, _counter(rb) as cb, _counter(ra) as into:
        cb.update_device(d_index.data_ptr(), d_umi.data_ptr(), b[0].size, stream=one.cuda_stream)
        tally = ca.remove_swapped_device([cb], into, 4, 5, stream=two.cuda_stream)
        cb.update_device(d_index.data_ptr(), d_umi.data_ptr(), b[0].size, stream=one.cuda_stream)
        assert tally.tolist() == want_tally
        DS._same(into, DS._snap(want))
        DS._same(cb, DS._snap(H.fed(rb.nw, rb.kind, rb.L, b, b)))
        torch.cuda.synchronize()


# ---- errors


def _call(src, k, dst, num=4, den=5, s=None, tally=None):
    """sct_molecules_swapped through the C ABI on a list of counters (None: a NULL element)."""
    handles = (ctypes.c_void_p * max(1, len(src)))(*[c._h if c is not None else None for c in src])
    return _lib.lib().sct_molecules_swapped(handles, len(src) if s is None else s, k,
                                            dst._h if dst is not None else None, num, den, tally, None)


def test_errors_leave_every_counter_as_it_was():
    (a, b), (ra, rb) = H.base()
    nw, kind, L = ra.nw, ra.kind, ra.L
    lib = _lib.lib()
    with _counter(ra, [a]) as ca, _counter(rb, [b]) as cb, \
            _counter(ra, [(a[0][:50], a[1][:50])]) as dst:
        held = (ca, cb, dst)
        before = [MM._state(c) for c in held]

        def invalid(rc, word):
            assert rc == _lib.SCT_E_INVALID and word in _lib.last_error(), (rc, _lib.last_error())
            assert [MM._state(c) for c in held] == before

        invalid(lib.sct_molecules_swapped(None, 2, 0, dst._h, 4, 5, None, None), "NULL")
        invalid(_call([ca, None], 0, dst), "NULL")
        invalid(_call([ca, cb], 0, None), "NULL")
        invalid(_call([ca, cb], 0, dst, s=0), "samples")
        invalid(_call([ca] * 17, 0, dst), "samples")
        invalid(_call([ca, cb], -1, dst), "outside")
        invalid(_call([ca, cb], 2, dst), "outside")
        invalid(_call([ca, cb, ca], 1, dst), "same counter")
        invalid(_call([ca, dst], 0, dst), "target")
        for num, den in ((1, 2), (0, 1), (0, 0), (5, 4), (2 ** 32 + 1, 2 ** 32 + 1), (2 ** 31, 2 ** 32)):
            invalid(_call([ca, cb], 0, dst, num, den), "fraction")
            with pytest.raises(ValueError, match="min_fraction"):
                counting.remove_swapped([ca, cb], (num, den))
        for bad in (0.8, (4, 5.0), (4,), "45", None, (True, 1)):
            with pytest.raises(ValueError, match="min_fraction"):
                counting.remove_swapped([ca, cb], bad)
        others = {"whitelist_size": (MM._counter(nw + 1, kind, L, True), "nw"),
                  "encoding": (MM._counter(nw, 2, L, True), "kind"),
                  "umi_length": (MM._counter(nw, kind, L + 1, True), "L differ"),
                  "read_counts": (MM._counter(nw, kind, L, False), "read counts"),
                  "features": (counting.MoleculeCounter(nw, L, ENC[kind], read_counts=True, features=5), "nf differ")}
        try:
            for word, (other, c_word) in others.items():
                invalid(_call([ca, other], 0, dst), c_word)
                invalid(_call([ca, other], 1, dst), c_word)
                invalid(_call([ca, cb], 0, other), c_word)
                with pytest.raises(ValueError, match=word):
                    counting.remove_swapped([ca, other])
                with pytest.raises(ValueError, match=word):
                    counting.remove_swapped([ca, cb], into=[dst, other])
                with pytest.raises(ValueError, match=word):
                    ca.remove_swapped_device([cb], other, 4, 5)
        finally:
            for other, _ in others.values():
                other.close()
        if _lib.device_count() >= 2:
            with MM._counter(nw, kind, L, True, [b], device=1) as far:
                invalid(_call([ca, far], 0, dst), "on one device first")
                with pytest.raises(ValueError, match="on one device first"):
                    counting.remove_swapped([ca, far])
        closed = _counter(rb, [b])
        closed.close()
        for call in (lambda: counting.remove_swapped([ca, closed]), lambda: counting.remove_swapped([closed, ca]),
                     lambda: counting.remove_swapped([ca, cb], into=[dst, closed]),
                     lambda: ca.remove_swapped_device([cb], closed, 4, 5)):
            with pytest.raises(ValueError, match="closed"):
                call()
        for call in (lambda: counting.remove_swapped([ca, ca]), lambda: counting.remove_swapped([ca, cb], into=[dst, dst]),
                     lambda: counting.remove_swapped([ca, cb], into=[dst, ca]),
                     lambda: ca.remove_swapped_device([cb], ca, 4, 5),
                     lambda: ca.remove_swapped_device([cb, cb], dst, 4, 5)):
            with pytest.raises(ValueError, match="repeated"):
                call()
        with pytest.raises(ValueError, match="into="):
            counting.remove_swapped([ca, cb], into=[dst])
        with pytest.raises(ValueError, match="1 to 16"):
            counting.remove_swapped([])
        for thing in (None, 7, "counter", (a[0], a[1])):
            with pytest.raises(TypeError):
                counting.remove_swapped([ca, thing])
            with pytest.raises(TypeError):
                ca.remove_swapped_device([cb], thing, 4, 5)
        assert [MM._state(c) for c in held] == before


def test_counters_made_by_a_failing_call_are_closed(monkeypatch):
    """The second sample's removal fails: the counter made for the first, which was filled already,
    and the one made for the second are closed before the error leaves."""
    (a, b), (ra, rb) = H.base()
    made = []
    real = counting.MoleculeCounter.remove_swapped_device

    def failing(self, others, into, num, den, stream=0):
        made.append(into)
        if len(made) == 2:
            raise RuntimeError("the second sample fails")
        return real(self, others, into, num, den, stream)

    with _counter(ra, [a]) as ca, _counter(rb, [b]) as cb:
        monkeypatch.setattr(counting.MoleculeCounter, "remove_swapped_device", failing)
        with pytest.raises(RuntimeError, match="second sample"):
            counting.remove_swapped([ca, cb])
        assert len(made) == 2 and not any(c._h for c in made)
        monkeypatch.undo()
        DS._same(ca, DS._snap(ra))
