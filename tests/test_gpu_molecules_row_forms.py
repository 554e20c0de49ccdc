"""The row forms of the molecule counter (sctools_amd/csrc/molecules.hip): every way of reading a
table back -- pairs() in its five forms, the three device fetch entry points, matrix() and collapse()
-- runs one sorted-rows stage, one emit kernel and one collapse pass, so they must agree with each
other on the columns they share, and with the contract in plain Python (tests/molecules_reference.py,
tests/umi_collapse_reference.py, tests/count_matrix_reference.py).

One counted feature counter (nw = 7, nf = 5, ThreeBit, UMI length 4) and one plain counter fed the
same reads, both from capacity_hint = 0: the tables start at 64 slots and grow, so the rehash kernel
runs with and without read counts.  M distinct molecules, M in {0, 1, 63, 64, 65, 1025}: the seams of
the 64-row wave tile, the smallest sorts, at least two growth steps.  A molecule is a distinct
(index, UMI) with one feature, read 1 to 4 times, the reads shuffled with a fixed seed.  Every
comparison is exact equality of integers and of order."""

import ctypes
import functools
from collections import Counter

import numpy as np
import pytest

import count_matrix_reference as M
import molecules_reference as R
import umi_collapse_reference as U
from sctools_amd import _lib, counting

pytestmark = pytest.mark.gpu

NW, NF, KIND, L = 7, 5, 3, 4
SIZES = [0, 1, 63, 64, 65, 1025]
FORMS = [dict(), dict(reads=True), dict(reads=True, parents=True), dict(features=True),
         dict(features=True, reads=True, parents=True)]


@functools.lru_cache(maxsize=None)
def _case(m):
    """(index, feature, umi) reads of m molecules and the three references fed with them."""
    rng = np.random.default_rng(1000 + m)
    which = rng.choice(NW * 4 ** L, size=m, replace=False)  # distinct (index, UMI)
    mi, digits = which // 4 ** L, which % 4 ** L
    mu = np.zeros(m, dtype=np.uint64)
    for p in range(L):
        mu |= ((digits // 4 ** p % 4 + 1).astype(np.uint64)) << np.uint64(3 * p)
    mf = rng.integers(0, NF, m)
    reads = np.repeat(np.arange(m), rng.integers(1, 5, m))
    rng.shuffle(reads)
    index, feature, umi = mi[reads].astype(np.int32), mf[reads].astype(np.int32), mu[reads]
    refs = (R.Molecules(NW, KIND, L).update(index, umi), U.CountedMolecules(NW, KIND, L).update(index, umi),
            M.FeatureMolecules(NW, NF, KIND, L).update(index, umi, feature))
    return index, feature, umi, refs


def _counters(m, upto=None, frm=0):
    index, feature, umi, _ = _case(m)
    sl = slice(frm, upto)
    fc = counting.MoleculeCounter(NW, L, capacity_hint=0, read_counts=True, features=NF)
    pc = counting.MoleculeCounter(NW, L, capacity_hint=0)
    fc.update(index[sl], umi[sl], features=feature[sl])
    pc.update(index[sl], umi[sl])
    return fc, pc


def _rows(cols):
    return list(zip(*(c.tolist() for c in cols)))


def _expected(m, form):
    """The feature reference's rows with the columns of `form`."""
    rows = _case(m)[3][2].pairs()
    keep = [0] + ([1] if form.get("features") else []) + [2] + ([3] if form.get("reads") else []) \
        + ([4] if form.get("parents") else [])
    return [tuple(r[k] for k in keep) for r in rows]


@pytest.mark.parametrize("m", SIZES)
def test_host_forms_agree(m):
    _, _, _, (plain_ref, counted_ref, _) = _case(m)
    fc, pc = _counters(m)
    with fc, pc:
        assert len(fc) == len(pc) == m
        got = {}
        for i, form in enumerate(FORMS):
            cols = fc.pairs(**form)
            assert all(c.shape == (m,) for c in cols)
            got[i] = _rows(cols)
            assert got[i] == _expected(m, form), form
        # a molecule's (index, UMI) is distinct here, so the feature column only reorders within a barcode
        assert Counter(pc.pairs()[0].tolist()) == Counter(fc.pairs(features=True)[0].tolist())
        assert sorted((r[0], r[2]) for r in got[3]) == _rows(pc.pairs()) == plain_ref.pairs()
        assert sorted((r[0], r[2], r[3]) for r in got[4]) == [r[:3] for r in counted_ref.pairs_counted()]
        if m >= 65:
            assert fc.info()["capacity"] > 64 and pc.info()["capacity"] > 64  # both rehash forms ran


def _device_rows(torch, call, m, room, want):
    """call(index_ptr, feature_ptr, umi_ptr, mreads_ptr, parent_ptr, room) into tensors of `room`
    rows filled with -7; `want` names the columns given (the others are passed as None)."""
    dt = {"index": torch.int32, "feature": torch.int32, "umi": torch.int64, "mreads": torch.int64, "parent": torch.int64}
    out = {k: torch.full((max(room, 1),), -7, dtype=dt[k], device="cuda") for k in want}
    torch.cuda.synchronize()
    call(*[out[k].data_ptr() if k in out else None for k in dt], room)
    torch.cuda.synchronize()
    for k in want:
        assert (out[k][m:] == -7).all(), "the tail of %s was written" % k
    return list(zip(*(out[k][:m].cpu().tolist() for k in dt if k in out)))


@pytest.mark.parametrize("m", SIZES)
def test_device_forms_equal_host_forms(m):
    torch = pytest.importorskip("torch")
    lib, vp = _lib.lib(), ctypes.c_void_p
    fc, pc = _counters(m)
    with fc, pc:
        for room in (m, m + 3):
            got = _device_rows(torch, lambda i, f, u, r, p, n: pc.fetch_device(i, u, n), m, room, ("index", "umi"))
            assert got == _rows(pc.pairs())
            got = _device_rows(torch, lambda i, f, u, r, p, n: fc.fetch_device(i, u, n), m, room, ("index", "umi"))
            assert got == _expected(m, {})
            for want, form in ((("index", "umi", "mreads"), dict(reads=True)),
                               (("index", "umi", "mreads", "parent"), dict(reads=True, parents=True))):
                got = _device_rows(torch, lambda i, f, u, r, p, n: fc.fetch_counted_device(i, u, r, p, n), m, room, want)
                assert got == _expected(m, form)
            for extra in ((), ("mreads",), ("parent",), ("mreads", "parent")):
                def call(i, f, u, r, p, n):
                    _lib.check(lib.sct_molecules_fetch_features(fc._h, vp(i), vp(f), vp(u), vp(r), vp(p), n, None))
                got = _device_rows(torch, call, m, room, ("index", "feature", "umi") + extra)
                form = dict(features=True, reads="mreads" in extra, parents="parent" in extra)
                full = _expected(m, dict(features=True, reads=True, parents=True))
                keep = [0, 1, 2] + ([3] if form["reads"] else []) + ([4] if form["parents"] else [])
                assert got == [tuple(r[k] for k in keep) for r in full]


def _group(rows):
    """pairs(features=True, reads=True, parents=True) grouped by (index, feature): the CSR matrix."""
    entries = {}
    for i, f, u, r, p in rows:
        e = entries.setdefault((i, f), [0, 0, set()])
        e[0] += 1
        e[1] += r
        e[2].add(p)
    order = sorted(entries)
    indptr = np.zeros(NW + 1, dtype=np.int64)
    for i, _ in order:
        indptr[i + 1:] += 1
    return (indptr.tolist(), [f for _, f in order], [entries[k][0] for k in order], [entries[k][1] for k in order],
            [len(entries[k][2]) for k in order])


def _matrix_and_collapse_agree(fc, m):
    rows = _rows(fc.pairs(features=True, reads=True, parents=True))
    full = tuple(a.tolist() for a in fc.matrix(reads=True, collapsed=True))
    assert full == _group(rows)
    collapsed, n_corrected = fc.collapse()
    per_row = [sum(full[4][full[0][i]:full[0][i + 1]]) for i in range(NW)]
    assert collapsed.tolist() == per_row
    assert n_corrected == sum(r[2] != r[4] for r in rows)
    return full, (collapsed.tolist(), n_corrected)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("m", SIZES)
def test_matrix_and_collapse(m, form):
    ref = _case(m)[3][2]
    fc, pc = _counters(m)
    with fc, pc, _lib.tuning(collapse_form=form):
        full, collapse = _matrix_and_collapse_agree(fc, m)
        assert full == ref.matrix() and collapse == ref.collapse()
        for kw, keep in ((dict(), (0, 1, 2)), (dict(reads=True), (0, 1, 2, 3)), (dict(collapsed=True), (0, 1, 2, 4))):
            assert tuple(a.tolist() for a in fc.matrix(**kw)) == tuple(full[k] for k in keep)


@pytest.mark.parametrize("merge_rows", [0, 1])
@pytest.mark.parametrize("m", SIZES)
def test_merge_of_two_halves(m, merge_rows):
    index = _case(m)[0]
    half = index.size // 2
    whole_f, whole_p = _counters(m)
    a_f, a_p = _counters(m, upto=half)
    b_f, b_p = _counters(m, frm=half)
    with whole_f, whole_p, a_f, a_p, b_f, b_p, _lib.tuning(merge_rows=merge_rows):
        a_f.merge(b_f)
        a_p.merge(b_p)
        assert len(a_f) == len(a_p) == m
        for form in FORMS:
            assert _rows(a_f.pairs(**form)) == _rows(whole_f.pairs(**form)) == _expected(m, form)
        assert _rows(a_p.pairs()) == _rows(whole_p.pairs())
        for kw in (dict(), dict(reads=True, collapsed=True)):
            assert [a.tolist() for a in a_f.matrix(**kw)] == [a.tolist() for a in whole_f.matrix(**kw)]
        assert [c.tolist() for c in a_f.counts()[:2]] == [c.tolist() for c in whole_f.counts()[:2]]
        _matrix_and_collapse_agree(a_f, m)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 1025])
def test_too_little_room(m):
    torch = pytest.importorskip("torch")
    lib, vp = _lib.lib(), ctypes.c_void_p
    message = "room for %d molecules, the counter holds %d" % (m - 1, m)
    fc, pc = _counters(m)
    with fc, pc:
        buf = torch.zeros((5, m), dtype=torch.int64, device="cuda")
        i, f, u, r, p = (buf[k].data_ptr() for k in range(5))
        calls = [lambda: pc.pairs(room=m - 1), lambda: pc.fetch_device(i, u, m - 1)]
        calls += [functools.partial(fc.pairs, room=m - 1, **form) for form in FORMS]
        calls += [lambda: fc.fetch_device(i, u, m - 1), lambda: fc.fetch_counted_device(i, u, r, None, m - 1),
                  lambda: fc.fetch_counted_device(i, u, r, p, m - 1)]
        calls += [lambda r_=r_, p_=p_: _lib.check(lib.sct_molecules_fetch_features(
            fc._h, vp(i), vp(f), vp(u), vp(r_), vp(p_), m - 1, None)) for r_ in (None, r) for p_ in (None, p)]
        for call in calls:
            with pytest.raises(ValueError) as err:
                call()
            assert message in str(err.value)
        torch.cuda.synchronize()
        assert (buf == 0).all()  # a refused call writes nothing
        for form in FORMS:
            assert _rows(fc.pairs(**form)) == _expected(m, form)
        assert _rows(pc.pairs()) == _case(m)[3][0].pairs()


@pytest.mark.parametrize("n", [0, 1, 64, 65])
@pytest.mark.parametrize("side", [False, True])
def test_device_counter_rows(n, side):
    """DeviceCounter.arrays() and fetch_device through the shared sorted-rows stage (rows sorted by
    first position, the side slot's key 2^64 - 1 among them): collections.Counter's order."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(n)
    distinct = rng.choice(1 << 40, size=n, replace=False).astype(np.uint64)
    if side and n:
        distinct[n // 2] = np.uint64(2 ** 64 - 1)
    codes = distinct[rng.integers(0, max(n, 1), 3 * n)] if n else distinct
    codes = np.concatenate([codes, distinct])  # every code at least once
    want = Counter(codes.tolist())
    first = {}
    for pos, c in enumerate(codes.tolist()):
        first.setdefault(c, pos)
    with counting.DeviceCounter(capacity_hint=0) as dc:
        dc.update(codes)
        keys, counts, firsts = dc.arrays()
        assert keys.tolist() == list(want) and counts.tolist() == list(want.values())
        assert firsts.tolist() == [first[k] for k in want]
        room = n + 2
        out = torch.full((3, room), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        dc.fetch_device(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), room)
        torch.cuda.synchronize()
        assert (out[:, n:] == -7).all()
        got = out[:, :n].cpu().numpy()
        assert got[0].view(np.uint64).tolist() == list(want) and got[1].tolist() == list(want.values())
        assert got[2].tolist() == firsts.tolist()
