"""Resolving features on the device (sctools_amd/csrc/molecules.hip, "resolving features" in
include/sctools_hip.h): MoleculeCounter.resolve and matrix(resolved=True) against
tests/feature_resolve_reference.py, the contract in plain Python.  Every comparison is exact equality
of integers; there is no tolerance anywhere.  The run pass can go wrong at the 64-row wave tile, at the
workgroup's 256 rows and past them, so the shapes put a group's first row, a collapsed molecule's rows
and a whole group on those seams; tables start at capacity_hint=64 unless a test says otherwise."""

import ctypes
import functools
import random

import numpy as np
import pytest

import count_matrix_reference as M
import feature_resolve_reference as F
import umi_collapse_reference as U
import umi_directional_reference as D
from sctools_amd import _lib, counting

pytestmark = pytest.mark.gpu

ENC = {3: "ThreeBit", 2: "TwoBit"}


def umi_of(kind, *digits):
    """A good code of the digits 0..3, written first base first (the first base in the high digit)."""
    code = 0
    for d in digits:
        code = (code << kind) | (d + (1 if kind == 3 else 0))
    return code


def nth_umi(kind, L, n):
    """The n-th good code of L bases in ascending order."""
    return umi_of(kind, *[(n >> (2 * p)) & 3 for p in reversed(range(L))])


def reference(nw, nf, kind, L, mreads):
    """The FeatureMolecules that holds {(index, feature, umi): reads} (no read is walked)."""
    fm = M.FeatureMolecules(nw, nf, kind, L)
    fm.mreads = dict(mreads)
    for (i, _, _), r in mreads.items():
        fm.reads[i] += r
        fm.molecules[i] += 1
    fm.total = sum(mreads.values())
    return fm


def reads_of(mreads, seed=0):
    """(index int32, feature int32, umi uint64): every molecule's reads, shuffled."""
    keys = np.array(list(mreads.keys()), dtype=np.int64).reshape(-1, 3)
    each = np.repeat(np.arange(len(mreads)), np.array(list(mreads.values()), dtype=np.int64))
    np.random.default_rng(seed).shuffle(each)
    return keys[each, 0].astype(np.int32), keys[each, 1].astype(np.int32), keys[each, 2].astype(np.uint64)


def counter(nw, nf, kind, L, mreads=None, hint=64, arrays=None):
    mc = counting.MoleculeCounter(nw, L, ENC[kind], capacity_hint=hint, read_counts=True, features=nf)
    index, feature, umi = arrays if arrays is not None else reads_of(mreads)
    return mc.update(index, umi, features=feature)


def device_answer(mc, method):
    """(resolve(method), matrix with every column the method has) as plain lists."""
    resolved = mc.resolve(method=method)
    matrix = mc.matrix(reads=True, collapsed=method != "none", resolved=True, method=method)
    return (resolved[0].tolist(),) + resolved[1:], [a.tolist() for a in matrix]


def reference_answer(fm, method):
    return F.answer(fm, method), [c for c in F.matrix_resolved(fm, method) if c is not None]


def check(mc, fm, methods=F.METHODS):
    """resolve() and matrix(resolved=True) of the device counter = the reference's, for every method,
    and the header's invariants on what the device gave."""
    for method in methods:
        got, want = device_answer(mc, method), reference_answer(fm, method)
        assert got[0] == want[0], method
        assert got[1] == want[1], method
        (resolved, n_shared, n_lost, n_tied, _), matrix = got
        indptr, bound, kept = matrix[0], matrix[-2] if method != "none" else matrix[2], matrix[-1]
        assert sum(resolved) + n_lost + n_tied == sum(bound)
        assert [sum(kept[indptr[i]:indptr[i + 1]]) for i in range(fm.nw)] == resolved
        assert all(k <= b for k, b in zip(kept, bound))
        if n_shared == 0:
            assert kept == bound and got[0][2:] == (0, 0, 0)


# ---- the cases worked by hand

def small_cases(kind):
    a, a2, u = umi_of(kind, 1, 1, 0), umi_of(kind, 1, 1, 2), umi_of(kind, 2, 3, 0)
    return {
        "worked": (1, 3, {(0, 1, a): 1, (0, 1, a2): 3, (0, 2, a2): 3}),
        "kept_and_lost": (2, 4, {(1, 0, u): 5, (1, 2, u): 3, (1, 3, u): 3}),
        "tied": (2, 4, {(1, 0, u): 3, (1, 2, u): 3, (1, 3, u): 1}),
        "alone": (2, 4, {(0, 3, umi_of(kind, 0, 0, 0)): 2, (1, 1, umi_of(kind, 3, 3, 3)): 1}),
    }


@pytest.mark.parametrize("kind", [3, 2])
def test_the_worked_case(kind):
    """Collapse comes first: A' ties 3 : 3 without it, and carries 4 reads against 3 with it."""
    nw, nf, mreads = small_cases(kind)["worked"]
    with counter(nw, nf, kind, 3, mreads) as mc:
        assert device_answer(mc, "none") == (([1], 1, 0, 2, 6), [[0, 2], [1, 2], [2, 1], [4, 3], [1, 0]])
        for method in ("one_step", "directional"):
            assert device_answer(mc, method) == (([1], 1, 1, 0, 3), [[0, 2], [1, 2], [2, 1], [4, 3], [1, 1], [1, 0]])
        check(mc, reference(nw, nf, kind, 3, mreads))


@pytest.mark.parametrize("kind", [3, 2])
@pytest.mark.parametrize("name,want", [("kept_and_lost", ([0, 1], 1, 2, 0, 6)), ("tied", ([0, 0], 1, 0, 3, 7)),
                                       ("alone", ([1, 1], 0, 0, 0, 0))])
def test_small_cases(kind, name, want):
    nw, nf, mreads = small_cases(kind)[name]
    with counter(nw, nf, kind, 3, mreads) as mc:
        for method in F.METHODS:
            assert device_answer(mc, method)[0] == want
        check(mc, reference(nw, nf, kind, 3, mreads))


# ---- seams of the run pass

def fillers(k, L):
    """k molecules of one read under barcode 0, feature 0: the sorted rows 0 .. k - 1."""
    return {(0, 0, nth_umi(3, L, n)): 1 for n in range(k)}


@pytest.mark.parametrize("k", [0, 62, 63, 64, 255, 256, 257])
def test_group_start_on_a_seam(k):
    """The group's first row is sorted row k; its top lies on the first member, the last, or the first
    row of the next wave tile, and in one variant the first and the last tie."""
    nw, nf, L = 2, 256, 6
    u = nth_umi(3, L, 1234)
    past = 64 - k % 64  # the member on the first row past the seam
    for size in (2, 3, 64, 65, 130):
        tops = [[0], [size - 1], [0, size - 1]] + ([[past]] if past < size else [])
        for top in tops:
            mreads = fillers(k, L)
            mreads.update({(1, f, u): 5 if f in top else 2 for f in range(size)})
            fm = reference(nw, nf, 3, L, mreads)
            want = F.answer(fm, "none")
            assert want[0][1] == (len(top) == 1) and want[1] == 1  # (the input is what it is meant to be)
            with counter(nw, nf, 3, L, mreads) as mc:
                check(mc, fm, methods=("none",))


@pytest.mark.parametrize("start", [60, 250])
@pytest.mark.parametrize("other", [-1, 0, 1])
def test_collapsed_molecule_across_a_seam(start, other):
    """A parent and its 18 one-base children under feature 3 are one collapsed molecule of 19 rows that
    starts at sorted row `start`; the parent's UMI alone under feature 9 has one read fewer than, as
    many as, or one more than the family."""
    nw, nf, L = 2, 16, 6
    parent = nth_umi(3, L, 2000)
    family = {(1, 3, parent): 10}
    family.update({(1, 3, v): 1 for v in U.neighbours(parent, 3, L)})
    assert len(family) == 19
    mreads = fillers(start, L)
    mreads.update(family)
    mreads[(1, 9, parent)] = sum(family.values()) + other
    fm = reference(nw, nf, 3, L, mreads)
    # barcode 1's kept molecules and the tally (the fillers of barcode 0 share nothing)
    want = {-1: (1, 1, 1, 0, 27), 0: (0, 1, 0, 2, 56), 1: (1, 1, 1, 0, 28)}[other]
    with counter(nw, nf, 3, L, mreads) as mc:
        got = device_answer(mc, "one_step")[0]
        assert (got[0][1],) + got[1:] == want
        check(mc, fm)


@functools.lru_cache(maxsize=None)
def snake_case():
    nw, nf, L = 2, 4, 10
    path = D.snake(3, L, 130, random.Random(7))
    mreads = {(1, 1, u): 1 for u in path}
    root = max(path)  # mutually joined 1-read UMIs: the largest code
    return nw, nf, L, mreads, root


@pytest.mark.parametrize("reads", [129, 130, 131])
def test_molecule_longer_than_two_tiles(reads):
    """130 one-read UMIs in a line are one directional cluster of 130 rows under feature 1; the root's
    UMI alone under feature 2 loses to it, ties with it, beats it."""
    nw, nf, L, snake, root = snake_case()
    mreads = dict(snake)
    mreads[(1, 2, root)] = reads
    fm = reference(nw, nf, 3, L, mreads)
    want = {129: ([0, 1], 1, 1, 0, 129), 130: ([0, 0], 1, 0, 2, 260), 131: ([0, 1], 1, 1, 0, 130)}[reads]
    assert F.answer(fm, "directional") == want
    with counter(nw, nf, 3, L, mreads) as mc:
        got = device_answer(mc, "directional")
        assert got[0] == want
        assert got[1][-1] == {129: [1, 0], 130: [0, 0], 131: [0, 1]}[reads]
        check(mc, fm)


@pytest.mark.parametrize("two_at_the_top", [False, True])
def test_whole_panel_group(two_at_the_top):
    """One (barcode, UMI) under all 4,096 features with 1 .. 4,096 reads: one lane walks the group."""
    nw, nf, L = 2, 4096, 6
    u = nth_umi(3, L, 77)
    mreads = {(1, f, u): f + 1 for f in range(nf)}
    if two_at_the_top:
        mreads[(1, 17, u)] = nf
    total = sum(mreads.values())
    want = ([0, 0], 1, 0, nf, total) if two_at_the_top else ([0, 1], 1, nf - 1, 0, total - nf)
    with counter(nw, nf, 3, L, mreads) as mc:
        for method in F.METHODS:
            resolved = mc.resolve(method=method)
            assert (resolved[0].tolist(),) + resolved[1:] == want
        kept = mc.matrix(resolved=True, method="none")[-1].tolist()
        assert kept == [0] * nf if two_at_the_top else kept == [0] * (nf - 1) + [1]


# ---- a random mix

@functools.lru_cache(maxsize=None)
def mix_case():
    nw, nf, kind, L = 5, 6, 3, 6
    index, feature, umi = F.mix(0, n=6000, nw=nw, nf=nf, kind=kind, L=L, hop=0.08, err=0.05, planted=8)
    fm = M.FeatureMolecules(nw, nf, kind, L).update(index, umi, feature)
    arrays = (np.array(index, np.int32), np.array(feature, np.int32), np.array(umi, np.uint64))
    return nw, nf, kind, L, arrays, fm, {m: reference_answer(fm, m) for m in F.METHODS}


@pytest.mark.parametrize("method", F.METHODS)
def test_random_mix(method):
    nw, nf, kind, L, arrays, fm, want = mix_case()
    # a condition on the input, stated on the reference alone: every kind of group is there
    alone, unique, tied = F.group_kinds(F.rows_of(fm, method))
    assert alone >= 5 and unique >= 5 and tied >= 5, (alone, unique, tied)
    with counter(nw, nf, kind, L, arrays=arrays) as mc:
        assert device_answer(mc, method) == want[method]
        assert device_answer(mc, method) == want[method]  # it reads only
        check(mc, fm, methods=(method,))


def test_layout_independence():
    """The same reads shuffled, in a small and a large first table, as two halves merged by both routes,
    and under both forms of the collapse and of the directional sweeps: one answer."""
    nw, nf, kind, L, (index, feature, umi), _, want = mix_case()
    order = np.random.default_rng(3).permutation(index.size)
    shuffled = (index[order], feature[order], umi[order])
    half = index.size // 2

    def answers(mc):
        return {m: device_answer(mc, m) for m in F.METHODS}

    for hint in (64, 1 << 20):
        with counter(nw, nf, kind, L, arrays=shuffled, hint=hint) as mc:
            assert answers(mc) == want
    for route in (0, 1):
        with _lib.tuning(merge_rows=route):
            with counter(nw, nf, kind, L, arrays=tuple(a[:half] for a in shuffled)) as a, \
                    counter(nw, nf, kind, L, arrays=tuple(a[half:] for a in shuffled), hint=4096) as b:
                assert answers(a.merge(b)) == want
    with counter(nw, nf, kind, L, arrays=(index, feature, umi)) as mc:
        for form in (0, 1):
            with _lib.tuning(collapse_form=form):
                assert answers(mc) == want
            with _lib.tuning(directional_form=form):
                assert answers(mc) == want


# ---- the matrix

def gappy_case():
    """nw = 7 with barcodes 0, 3 and 6 empty; barcode 2 loses everything under feature 1."""
    kind, L = 3, 4
    a, b, c = nth_umi(kind, L, 5), nth_umi(kind, L, 90), nth_umi(kind, L, 200)
    mreads = {(1, 0, a): 2, (1, 2, a): 1, (1, 2, b): 4, (2, 1, c): 2, (2, 3, c): 2, (2, 3, a): 1,
              (4, 0, b): 1, (5, 1, a): 3, (5, 0, a): 3, (5, 2, c): 1}
    return 7, 4, kind, L, mreads


def test_matrix_shares_its_layout_and_keeps_explicit_zeros():
    nw, nf, kind, L, mreads = gappy_case()
    fm = reference(nw, nf, kind, L, mreads)
    with counter(nw, nf, kind, L, mreads) as mc:
        check(mc, fm)
        plain = [a.tolist() for a in mc.matrix(reads=True, collapsed=True)]
        for method in F.METHODS:
            full = mc.matrix(reads=True, collapsed=method != "none", resolved=True, method=method)
            assert [a.dtype for a in full] == [np.int64, np.int32] + [np.int64] * (len(full) - 2)
            assert [a.tolist() for a in full[:4]] == plain[:4]  # indptr, feature, molecules, reads
            only = mc.matrix(resolved=True, method=method)  # the new column alone comes last
            assert [a.tolist() for a in only] == plain[:3] + [full[-1].tolist()]
            assert [a.tolist() for a in mc.matrix(reads=True, resolved=True, method=method)][:4] == plain[:4]
        indptr, feature, _, kept = (a.tolist() for a in mc.matrix(resolved=True))
        assert indptr == [0, 0, 2, 4, 4, 5, 8, 8]  # empty barcodes at the start, in the middle and at the end
        entries = [(i, f) for i in range(nw) for f in feature[indptr[i]:indptr[i + 1]]]
        assert dict(zip(entries, kept)) == {(1, 0): 1, (1, 2): 1, (2, 1): 0, (2, 3): 1, (4, 0): 1, (5, 0): 0, (5, 1): 0,
                                            (5, 2): 1}
        assert mc.resolve()[0].tolist() == [0, 2, 1, 0, 1, 1, 0]
        # the existing call gives what it gave
        assert [a.tolist() for a in mc.matrix(reads=True, collapsed=True)] == plain


def test_matrix_room_and_the_empty_counter():
    nw, nf, kind, L, mreads = gappy_case()
    lib = _lib.lib()
    with counter(nw, nf, kind, L, mreads) as mc:
        with pytest.raises(ValueError, match="8"):  # nnz is named
            mc.matrix(resolved=True, room=7)
        assert len(mc.matrix(resolved=True, room=8)[-1]) == 8
        # the C ABI: nnz reported, nothing written, the tally included
        indptr, feature = np.full(nw + 1, -1, np.int64), np.full(8, -7, np.int32)
        values, tally = np.full((4, 8), 99, np.uint64), np.full(4, 99, np.uint64)
        nnz = ctypes.c_int64(-1)
        rc = lib.sct_molecules_matrix_resolved_host(mc._h, 0, _lib._ptr(indptr), _lib._ptr(feature), _lib._ptr(values[0]),
                                                    _lib._ptr(values[1]), _lib._ptr(values[2]), _lib._ptr(values[3]),
                                                    _lib._ptr(tally), 3, ctypes.byref(nnz))
        assert (rc, nnz.value) == (_lib.SCT_E_INVALID, 8)
        assert (indptr == -1).all() and (feature == -7).all() and (values == 99).all() and (tally == 99).all()
        rc = lib.sct_molecules_matrix_resolved_host(mc._h, 0, _lib._ptr(indptr), _lib._ptr(feature), _lib._ptr(values[0]),
                                                    _lib._ptr(values[1]), _lib._ptr(values[2]), _lib._ptr(values[3]),
                                                    _lib._ptr(tally), 8, ctypes.byref(nnz))
        assert (rc, nnz.value) == (_lib.SCT_OK, 8)
        assert tuple(int(t) for t in tally) == mc.resolve()[1:]
        assert values[3].tolist() == mc.matrix(resolved=True)[-1].tolist()
    with counting.MoleculeCounter(nw, L, ENC[kind], capacity_hint=64, read_counts=True, features=nf) as mc:
        for method in F.METHODS:
            resolved = mc.resolve(method=method)
            assert (resolved[0].tolist(),) + resolved[1:] == ([0] * nw, 0, 0, 0, 0)
            got = mc.matrix(resolved=True, method=method)
            assert got[0].tolist() == [0] * (nw + 1) and all(a.size == 0 for a in got[1:])
        tally = np.full(4, 99, np.uint64)
        nnz = ctypes.c_int64(-1)
        indptr = np.full(nw + 1, -1, np.int64)
        rc = lib.sct_molecules_matrix_resolved_host(mc._h, 2, _lib._ptr(indptr), None, None, None, None, None,
                                                    _lib._ptr(tally), 0, ctypes.byref(nnz))
        assert (rc, nnz.value, indptr.tolist(), tally.tolist()) == (_lib.SCT_OK, 0, [0] * (nw + 1), [0] * 4)


def test_device_forms_match_the_host_forms():
    torch = pytest.importorskip("torch")
    nw, nf, kind, L, arrays, _, want = mix_case()
    side = torch.cuda.Stream()
    with counter(nw, nf, kind, L, arrays=arrays) as mc:
        for method in F.METHODS:
            (resolved, *tally), matrix = want[method]
            nnz, room = len(matrix[1]), len(matrix[1]) + 3
            d_resolved = torch.full((nw,), -7, dtype=torch.int64, device="cuda")
            d_tally = torch.full((4,), -7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            mc.resolve_device(d_resolved.data_ptr(), d_tally.data_ptr(), stream=side.cuda_stream, method=method)
            torch.cuda.synchronize()
            assert (d_resolved.cpu().tolist(), d_tally.cpu().tolist()) == (resolved, tally)
            d_resolved.fill_(-7)
            torch.cuda.synchronize()
            mc.resolve_device(d_resolved.data_ptr(), method=method)  # no tally
            torch.cuda.synchronize()
            assert d_resolved.cpu().tolist() == resolved
            o_indptr = torch.full((nw + 1,), -1, dtype=torch.int64, device="cuda")
            o_feat = torch.full((room,), -7, dtype=torch.int32, device="cuda")
            o_val = torch.full((4, room), -7, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            collapsed = o_val[2].data_ptr() if method != "none" else None
            got = mc.matrix_device(o_indptr.data_ptr(), o_feat.data_ptr(), o_val[0].data_ptr(), o_val[1].data_ptr(),
                                   collapsed, room, stream=side.cuda_stream, method=method,
                                   resolved_ptr=o_val[3].data_ptr())
            torch.cuda.synchronize()
            assert got == nnz
            columns = [0, 1, 2, 3] if method != "none" else [0, 1, 3]
            assert [o_indptr.cpu().tolist(), o_feat[:nnz].cpu().tolist()] == matrix[:2]
            assert o_val[columns, :nnz].cpu().tolist() == matrix[2:]
            assert (o_feat[nnz:] == -7).all() and (o_val[:, nnz:] == -7).all()  # nothing past nnz
            if method == "none":
                assert (o_val[2] == -7).all()
            # the resolved column alone
            o_val.fill_(-7)
            torch.cuda.synchronize()
            assert mc.matrix_device(o_indptr.data_ptr(), o_feat.data_ptr(), None, None, None, room, method=method,
                                    resolved_ptr=o_val[3].data_ptr()) == nnz
            torch.cuda.synchronize()
            assert o_val[3, :nnz].cpu().tolist() == matrix[-1] and (o_val[:3] == -7).all()


# ---- errors

def _unchanged(mc, before):
    assert [a.tolist() if hasattr(a, "tolist") else a for a in mc.counts()] == before[0]
    assert [a.tolist() for a in mc.matrix()] == before[1]


def _state(mc):
    return [a.tolist() if hasattr(a, "tolist") else a for a in mc.counts()], [a.tolist() for a in mc.matrix()]


def test_errors_change_nothing():
    nw, nf, kind, L, mreads = gappy_case()
    index, feature, umi = reads_of(mreads)
    lib = _lib.lib()
    out, tally = np.full(nw, 99, np.uint64), np.full(4, 99, np.uint64)
    # a counter that is not counted
    with counting.MoleculeCounter(nw, L, ENC[kind], capacity_hint=64, features=nf) as mc:
        mc.update(index, umi, features=feature)
        before = _state(mc)
        with pytest.raises(ValueError, match="read_counts"):
            mc.resolve()
        with pytest.raises(ValueError, match="read_counts"):
            mc.matrix(resolved=True)
        with pytest.raises(ValueError, match="read_counts"):
            mc.resolve_device(1)
        with pytest.raises(ValueError, match="read_counts"):
            mc.matrix_device(1, 1, None, None, None, 8, resolved_ptr=1)
        assert lib.sct_molecules_resolve_host(mc._h, 0, _lib._ptr(out), _lib._ptr(tally)) == _lib.SCT_E_INVALID
        _unchanged(mc, before)
    # a counter without features
    with counting.MoleculeCounter(nw, L, ENC[kind], capacity_hint=64, read_counts=True) as mc:
        mc.update(index, umi)
        counts = [a.tolist() if hasattr(a, "tolist") else a for a in mc.counts()]
        with pytest.raises(ValueError, match="features"):
            mc.resolve()
        with pytest.raises(ValueError, match="features"):
            mc.matrix(resolved=True)
        assert lib.sct_molecules_resolve_host(mc._h, 0, _lib._ptr(out), _lib._ptr(tally)) == _lib.SCT_E_INVALID
        assert [a.tolist() if hasattr(a, "tolist") else a for a in mc.counts()] == counts
    # unknown methods, and a collapsed column without a collapse
    with counter(nw, nf, kind, L, mreads) as mc:
        before = _state(mc)
        indptr, feat, values = np.full(nw + 1, -1, np.int64), np.full(8, -7, np.int32), np.full((4, 8), 99, np.uint64)
        nnz = ctypes.c_int64(-1)
        for method in (-1, 3):
            assert lib.sct_molecules_resolve_host(mc._h, method, _lib._ptr(out), _lib._ptr(tally)) == _lib.SCT_E_INVALID
            assert "method" in _lib.last_error()
            rc = lib.sct_molecules_matrix_resolved_host(mc._h, method, _lib._ptr(indptr), _lib._ptr(feat),
                                                        _lib._ptr(values[0]), None, None, _lib._ptr(values[3]), None, 8,
                                                        ctypes.byref(nnz))
            assert rc == _lib.SCT_E_INVALID
        rc = lib.sct_molecules_matrix_resolved_host(mc._h, 2, _lib._ptr(indptr), _lib._ptr(feat), _lib._ptr(values[0]),
                                                    None, _lib._ptr(values[2]), _lib._ptr(values[3]), None, 8,
                                                    ctypes.byref(nnz))
        assert rc == _lib.SCT_E_INVALID
        assert (out == 99).all() and (tally == 99).all() and (indptr == -1).all() and (values == 99).all()
        for bad in ("nope", None, 2):
            with pytest.raises(ValueError, match="method"):
                mc.resolve(method=bad)
        with pytest.raises(ValueError):
            mc.matrix(collapsed=True, method="none")
        with pytest.raises(ValueError):
            mc.matrix(collapsed=True, resolved=True, method="none")
        with pytest.raises(ValueError):
            mc.matrix(method="none")  # 'none' is a method of the resolve calls only
        # the calls that take a collapse method go on rejecting 2
        assert lib.sct_molecules_collapse_by_host(mc._h, 2, _lib._ptr(out), None) == _lib.SCT_E_INVALID
        rc = lib.sct_molecules_matrix_by_host(mc._h, 2, _lib._ptr(indptr), _lib._ptr(feat), _lib._ptr(values[0]), None, None,
                                              8, ctypes.byref(nnz))
        assert rc == _lib.SCT_E_INVALID
        with pytest.raises(ValueError):
            counting.collapse_method("none")
        assert counting.resolve_method("none") == 2 and counting.resolve_method("directional") == 1
        _unchanged(mc, before)
