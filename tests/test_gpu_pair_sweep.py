"""GPU: the seams of the schedule that allpairs_count_kernel and allpairs_close_kernel share (work-queue
pulls, chunk-major items, the LDS tile restaged at chunk seams, the counter flush), by exact integer
equality at the smallest shapes that have them.

  SUBSETS (2049, 16): 1,024 columns per chunk, chunks of 4, 8 and 8 items (20 items), the last chunk
                      holding one column
  SUBSETS (1025, 17): 512 columns per chunk, chunks of 2, 4 and 4 items (10 items)
  MOMENTS (1025, 16): the triple-layout tile, 512 columns per chunk, the same 10 items

A pull of 3 items starts at every offset against the chunk seams once the item range is split at every
item; allpairs_flush_items=1 adds a counter flush, which uses the tile as scratch, before every pull."""

import functools

import numpy as np
import pytest

import close_pairs_reference as C
import test_gpu_close_pairs as CP
from oracle import oracle as O
from sctools_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

# (scheme, n, L, item count, splits): every split of the first shape, three inside a chunk of the others
COUNT_SHAPES = [
    (_lib.SCHEME_SUBSETS, 2049, 16, 20, range(21)),
    (_lib.SCHEME_SUBSETS, 1025, 17, 10, (1, 4, 8)),
    (_lib.SCHEME_MOMENTS, 1025, 16, 10, (1, 4, 8)),
]
# (n, L, item count, a split inside the middle chunk)
CLOSE_SHAPES = [(2049, 16, 20, 7), (1025, 17, 10, 4)]


@functools.lru_cache(maxsize=None)
def make_codes(n, L):
    """n codes of L bases: distinct seeded codes, then copies of 12 of them spread over the set with
    0, 1, 2 and 3 bases substituted (the copies lie in the last chunk, their sources in every chunk)"""
    base = synthetic.whitelist_codes(n - 12, L, seed=100 * L + n)
    rng = np.random.default_rng(n + L)
    src = base[np.linspace(0, base.size - 1, 12).astype(np.int64)]
    planted = [CP._substitute(rng, s, L, k % 4) for k, s in enumerate(src.tolist())]
    codes = np.concatenate([base, np.array(planted, dtype=np.uint64)])
    codes.setflags(write=False)
    return codes


@functools.lru_cache(maxsize=None)
def oracle_hist(n, L):
    return O.c_hist_rows(make_codes(n, L)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def close_reference(n, L):
    i, j, dist = C.close_pairs(make_codes(n, L), 2 * L, 3)
    for a in (i, j, dist):
        a.setflags(write=False)
    return i, j, dist


@pytest.mark.parametrize("flush", [0, 1])
@pytest.mark.parametrize("scheme,n,L,items,splits", COUNT_SHAPES)
def test_count_ranges_add_up_across_pulls_and_chunk_seams(scheme, n, L, items, splits, flush):
    torch = pytest.importorskip("torch")
    codes = make_codes(n, L)
    d_codes = torch.from_numpy(codes.view(np.int64).copy()).cuda()
    knobs = dict(allpairs_grab=3, allpairs_flush_items=1) if flush else dict(allpairs_grab=3)
    with _lib.tuning(**knobs):
        plan = _lib.AllPairsPlan(d_codes.data_ptr(), n, 2 * L, scheme=scheme)
        try:
            assert plan.scheme == scheme and plan.items == items
            plan.build()

            def counts(begin, end):
                c = torch.zeros(plan.ncounts, dtype=torch.int64, device="cuda")
                plan.count(c.data_ptr(), begin, end)
                torch.cuda.synchronize()
                return c.cpu().numpy()

            whole = counts(0, items)
            assert int(whole[0]) == n * (n - 1) // 2
            moments = torch.zeros(plan.ncounts, dtype=torch.int64, device="cuda")
            plan.moments(moments.data_ptr())  # (adds nothing for SUBSETS)
            hist = plan.counts_to_hist((whole + moments.cpu().numpy()).view(np.uint64)).astype(np.int64)
            ref = oracle_hist(n, L)
            assert hist.tolist() == ref[:plan.nbins].tolist() and ref[plan.nbins:].sum() == 0
            assert hist[0] > 0 and hist[1] > 0
            for b in splits:
                assert np.array_equal(counts(0, b) + counts(b, items), whole), b
        finally:
            plan.close()


@pytest.mark.parametrize("grab", [3, 1])
@pytest.mark.parametrize("n,L,items,split", CLOSE_SHAPES)
def test_close_pairs_across_pulls_and_chunk_seams(n, L, items, split, grab):
    pytest.importorskip("torch")
    ri, rj, rd = close_reference(n, L)
    assert (np.bincount(rd, minlength=4) > 0).all()
    with _lib.tuning(allpairs_grab=grab):
        dev = CP.Device(make_codes(n, L), L)
        try:
            assert dev.plan.items == items
            for max_d in (1, 3):
                keep = rd <= max_d
                wi, wj, wd = ri[keep], rj[keep], rd[keep]
                want_stats = [wi.size, wi.size] + np.bincount(wd, minlength=4).tolist()
                want_deg = CP.degrees(n, max_d, wi, wj, wd)
                i, j, dist, stats, deg = dev.run(max_d, wi.size + 3)
                assert stats.tolist() == want_stats
                assert np.array_equal(i, wi) and np.array_equal(j, wj) and np.array_equal(dist, wd)
                assert np.array_equal(deg, want_deg)
                # two item ranges split inside a chunk: pairs concatenate, stats and degrees add
                parts = [dev.run(max_d, wi.size, 0, split), dev.run(max_d, wi.size, split, items)]
                for p in parts:  # each part alone is in order
                    assert np.array_equal(np.lexsort((p[1], p[0])), np.arange(p[0].size))
                words = np.concatenate([(p[0].astype(np.int64) << 33) | (p[1].astype(np.int64) << 2) | p[2]
                                        for p in parts])
                words.sort()
                assert np.array_equal(words >> 33, wi) and np.array_equal((words >> 2) & (2 ** 31 - 1), wj)
                assert np.array_equal(words & 3, wd)
                assert sum(p[3] for p in parts).tolist() == want_stats
                assert np.array_equal(sum(p[4].astype(np.int64) for p in parts), want_deg)
        finally:
            dev.close()
