"""The host forms of the nearest index -- query, count, correct, correct_count, each on one
device and split over device slots (sct_nearest_*_host, sct_nearest_multi_*_host) -- pinned
against the brute forces: tests/posterior_reference.py for the correct forms, the C oracle for the
query forms.  Every expected value comes from those two, never from another form of the library.

Covered here and nowhere else: quality rows with a stride above the barcode length, the `+=`
contract of counts / tally / stats, three slots with an uneven split, a slot with an empty range,
and the host argument checks of the eight entry points."""

import functools
from collections import namedtuple

import numpy as np
import pytest

import posterior_reference as R
from oracle import oracle as O
from sctools_amd import _lib
from test_gpu_posterior import W, family, priors_for

pytestmark = pytest.mark.gpu

# 300 codes and 1,257 queries each: five workgroups with a ragged last one, 419 queries per slot
# on three slots; the 8 + 8 digit split with the index pass, and the odd 3 + 2 split without it
CASES = [(3, 16, "shuffled"), (2, 5, "alphabetical")]
DEVICES = [None, [0, 0], [0, 0, 0]]
THRESHOLD = (3, 4)
PAD = {16: 24, 5: 8}  # bytes between padded quality rows

Expected = namedtuple("Expected", "prior ci cd ni nd scored_lo scored_hi")


@functools.lru_cache(maxsize=None)
def expected(case):
    kind, L, _ = case
    wl, queries, quals, scanned = family(*case)
    prior = priors_for(np.random.default_rng(8), wl.size).astype(np.uint32)
    ci, cd = R.decide(L, scanned, quals, prior, W, *THRESHOLD)
    ni, nd = O.c_nearest(kind, wl, queries, 1)
    # scored queries: those with several distance-1 candidates at least, at most all with any
    near = np.array([len(row[1]) if row[0] == "near" else 0 for row in scanned])
    return Expected(prior, np.array(ci, dtype=np.int32), np.array(cd, dtype=np.uint8), ni, nd, near >= 2, near >= 1)


def tallies(index, nw):
    return (np.bincount(index[index >= 0], minlength=nw).astype(np.uint64),
            np.array([(index == -1).sum(), (index == -2).sum()], dtype=np.uint64))


def check_stats(stats, case, sl=slice(None)):
    """stats = (queries scored, those of them given an index), bounded by the reference's rows"""
    e = expected(case)
    nq = np.arange(e.ci.size)[sl].size
    assert int(stats[1]) <= int(stats[0]) <= nq
    assert e.scored_lo[sl].sum() <= int(stats[0]) <= e.scored_hi[sl].sum()
    assert (e.scored_lo[sl] & (e.ci[sl] >= 0)).sum() <= int(stats[1]) <= (e.scored_hi[sl] & (e.ci[sl] >= 0)).sum()


@pytest.fixture(scope="module")
def plans():
    made = {}

    def get(case, devices):
        key = (case, tuple(devices) if devices else None)
        if key not in made:
            kind, L, _ = case
            made[key] = _lib.HostNearestPlan(kind, family(*case)[0], kind * L, 1, devices=devices)
            made[key].set_posterior(expected(case).prior, W, *THRESHOLD)
        return made[key]

    yield get
    for p in made.values():
        p.close()


def c_form(plan, name):
    """the bound C function of a form for this plan: (f, takes quality rows)"""
    lib = _lib.lib()
    stem = "sct_nearest_multi_%s_host" if plan._multi else "sct_nearest_%s_host"
    return getattr(lib, stem % name), name.startswith("correct")


def call_c(plan, name, q, rows, stride, nq, outs):
    f, with_rows = c_form(plan, name)
    args = [plan._h, _lib._ptr(q)] + ([_lib._ptr(rows), stride] if with_rows else []) + [nq]
    return f(*args, *[_lib._ptr(o) for o in outs])


@pytest.mark.parametrize("devices", DEVICES, ids=["one", "two", "three"])
@pytest.mark.parametrize("case", CASES, ids=["3x16", "2x5"])
def test_every_form_matches_the_reference(plans, case, devices):
    wl, queries, quals, _ = family(*case)
    e = expected(case)
    plan = plans(case, devices)
    index, dist = plan.query(queries)
    assert np.array_equal(index, e.ni) and np.array_equal(dist, e.nd)
    counts, tally = np.zeros(wl.size, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    plan.count(queries, counts, tally)
    want = tallies(e.ni, wl.size)
    assert np.array_equal(counts, want[0]) and np.array_equal(tally, want[1])
    index, dist, stats = plan.correct(queries, quals)
    assert index.dtype == np.int32 and dist.dtype == np.uint8
    assert np.array_equal(index, e.ci) and np.array_equal(dist, e.cd)
    check_stats(stats, case)
    counts, tally = np.zeros(wl.size, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    stats2 = plan.correct_count(queries, quals, counts, tally)
    want = tallies(e.ci, wl.size)
    assert np.array_equal(counts, want[0]) and np.array_equal(tally, want[1])
    check_stats(stats2, case)
    # every class of answer is in the input
    assert (e.ci >= 0).any() and (e.ci == -1).any() and (e.ci == -2).any() and (e.ni == -2).any()
    assert (e.ci != e.ni).any()


@pytest.mark.parametrize("devices", DEVICES[:2], ids=["one", "two"])
@pytest.mark.parametrize("case", CASES, ids=["3x16", "2x5"])
def test_padded_quality_rows(plans, case, devices):
    """Rows 24 (8) bytes apart for 16 (5) positions: the strided copy; the padding bytes would
    change the answers if they were read as qualities."""
    L = case[1]
    wl, queries, quals, _ = family(*case)
    e = expected(case)
    padded = np.zeros((queries.size, PAD[L]), dtype=np.uint8)
    padded[:, L:] = 255 - quals[:, :PAD[L] - L]
    padded[:, :L] = quals
    rows = padded[:, :L]
    assert rows.strides == (PAD[L], 1) and not rows.flags.c_contiguous
    plan = plans(case, devices)
    index, dist, stats = plan.correct(queries, rows)
    assert np.array_equal(index, e.ci) and np.array_equal(dist, e.cd)
    check_stats(stats, case)
    counts, tally = np.zeros(wl.size, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    check_stats(plan.correct_count(queries, rows, counts, tally), case)
    want = tallies(e.ci, wl.size)
    assert np.array_equal(counts, want[0]) and np.array_equal(tally, want[1])


@pytest.mark.parametrize("devices", [None, [0, 0, 0]], ids=["one", "three"])
@pytest.mark.parametrize("case", CASES, ids=["3x16", "2x5"])
def test_outputs_accumulate(plans, case, devices):
    """counts, tally and stats are added to, never overwritten: prefilled arrays, in one call and
    in batches of 400 / 1 / 856."""
    L = case[1]
    wl, queries, quals, _ = family(*case)
    e = expected(case)
    plan = plans(case, devices)
    fill_c = (np.arange(wl.size, dtype=np.uint64) * 3 + 7)
    fill_t = np.array([11, 1 << 40], dtype=np.uint64)
    fill_s = np.array([1000, 1 << 33], dtype=np.uint64)
    batches = (slice(0, 400), slice(400, 401), slice(401, None))
    for parts in ((slice(None),), batches):
        counts, tally = fill_c.copy(), fill_t.copy()
        for sl in parts:
            plan.count(queries[sl], counts, tally)
        want = tallies(e.ni, wl.size)
        assert np.array_equal(counts - fill_c, want[0]) and np.array_equal(tally - fill_t, want[1])
        counts, tally, stats = fill_c.copy(), fill_t.copy(), fill_s.copy()
        for sl in parts:
            q, rows = np.ascontiguousarray(queries[sl]), np.ascontiguousarray(quals[sl])
            assert call_c(plan, "correct_count", q, rows, L, q.size, (counts, tally, stats)) == _lib.SCT_OK
        want = tallies(e.ci, wl.size)
        assert np.array_equal(counts - fill_c, want[0]) and np.array_equal(tally - fill_t, want[1])
        check_stats(stats - fill_s, case)
        stats = fill_s.copy()
        index, dist = np.full(queries.size, 77, dtype=np.int32), np.full(queries.size, 77, dtype=np.uint8)
        for sl in parts:
            q, rows = np.ascontiguousarray(queries[sl]), np.ascontiguousarray(quals[sl])
            assert call_c(plan, "correct", q, rows, L, q.size, (index[sl], dist[sl], stats)) == _lib.SCT_OK
        assert np.array_equal(index, e.ci) and np.array_equal(dist, e.cd)
        check_stats(stats - fill_s, case)


@pytest.mark.parametrize("devices", DEVICES[:2], ids=["one", "two"])
def test_empty_batch_touches_nothing(plans, devices):
    case = CASES[0]
    wl, queries, quals, _ = family(*case)
    plan = plans(case, devices)
    q, rows = np.ascontiguousarray(queries[:1]), np.ascontiguousarray(quals[:1])
    index, dist = np.full(1, 77, dtype=np.int32), np.full(1, 77, dtype=np.uint8)
    counts, tally, stats = (np.full(n, 5, dtype=np.uint64) for n in (wl.size, 2, 2))
    for name, outs in (("query", (index, dist)), ("count", (counts, tally)), ("correct", (index, dist, stats)),
                       ("correct_count", (counts, tally, stats))):
        assert call_c(plan, name, q, rows, case[1], 0, outs) == _lib.SCT_OK, name
    assert index[0] == 77 and dist[0] == 77
    assert (counts == 5).all() and (tally == 5).all() and (stats == 5).all()
    # and through the Python forms
    assert [a.size for a in plan.query(queries[:0])] == [0, 0]
    plan.count(queries[:0], counts, tally)
    assert [a.size for a in plan.correct(queries[:0], quals[:0])[:2]] == [0, 0]
    assert plan.correct_count(queries[:0], quals[:0], counts, tally).tolist() == [0, 0]
    assert (counts == 5).all() and (tally == 5).all()


@pytest.mark.parametrize("case", CASES, ids=["3x16", "2x5"])
def test_one_query_on_two_slots(plans, case):
    """nq = 1 on [0, 0]: slot 0 gets the empty range [0, 0), slot 1 the query."""
    wl, queries, quals, _ = family(*case)
    e = expected(case)
    plan = plans(case, [0, 0])
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 60):  # every class of query of family()
        sl = slice(k, k + 1)
        index, dist = plan.query(queries[sl])
        assert (index[0], dist[0]) == (e.ni[k], e.nd[k])
        counts, tally = np.zeros(wl.size, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
        plan.count(queries[sl], counts, tally)
        want = tallies(e.ni[sl], wl.size)
        assert np.array_equal(counts, want[0]) and np.array_equal(tally, want[1])
        index, dist, stats = plan.correct(queries[sl], quals[sl])
        assert (index[0], dist[0]) == (e.ci[k], e.cd[k])
        check_stats(stats, case, sl)
        counts, tally = np.zeros(wl.size, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
        check_stats(plan.correct_count(queries[sl], quals[sl], counts, tally), case, sl)
        want = tallies(e.ci[sl], wl.size)
        assert np.array_equal(counts, want[0]) and np.array_equal(tally, want[1])


@pytest.mark.parametrize("devices", DEVICES[:2], ids=["one", "two"])
def test_other_plans_are_refused(devices):
    """Host argument checks: a max_d = 2 plan and a whitelist with an N have no half-key tables."""
    seqs = ["ACGTACGT", "ACGTACGA", "TTTTACGT"]
    q = np.array([R.encode(3, "ACGTACGC")], dtype=np.uint64)
    quals = np.full((1, 8), 40, dtype=np.uint8)
    with_n = np.array([R.encode(3, s) for s in seqs + ["ACNTACGT"]], dtype=np.uint64)
    for wl, max_d in ((with_n, 1), (with_n[:3], 2)):
        plan = _lib.HostNearestPlan(3, wl, 24, max_d, devices=devices)
        try:
            counts, tally = np.zeros(wl.size, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
            with pytest.raises(ValueError, match="half-key"):
                plan.correct(q, quals)
            with pytest.raises(ValueError, match="half-key"):
                plan.correct_count(q, quals, counts, tally)
            assert not counts.any() and not tally.any()
            index, dist = plan.query(q)  # the plan itself works
            ridx, rdist = O.c_nearest(3, wl, q, max_d)
            assert (index[0], dist[0]) == (ridx[0], rdist[0]) == (-2, 1)
        finally:
            plan.close()


@pytest.mark.parametrize("devices", DEVICES[:2], ids=["one", "two"])
def test_bad_arguments_are_invalid(plans, devices):
    case = CASES[0]
    L = case[1]
    wl, queries, quals, _ = family(*case)
    plan = plans(case, devices)
    q, rows = np.ascontiguousarray(queries[:8]), np.ascontiguousarray(quals[:8])
    index, dist = np.full(8, 77, dtype=np.int32), np.full(8, 77, dtype=np.uint8)
    counts, tally, stats = (np.full(n, 5, dtype=np.uint64) for n in (wl.size, 2, 2))
    # rows closer together than the plan's positions
    assert call_c(plan, "correct", q, rows, L - 1, 8, (index, dist, stats)) == _lib.SCT_E_INVALID
    assert call_c(plan, "correct_count", q, rows, L - 1, 8, (counts, tally, stats)) == _lib.SCT_E_INVALID
    # no counts array for a whitelist that has codes
    assert call_c(plan, "count", q, rows, L, 8, (None, tally)) == _lib.SCT_E_INVALID
    assert call_c(plan, "correct_count", q, rows, L, 8, (None, tally, stats)) == _lib.SCT_E_INVALID
    assert (index == 77).all() and (dist == 77).all()
    assert (counts == 5).all() and (tally == 5).all() and (stats == 5).all()
