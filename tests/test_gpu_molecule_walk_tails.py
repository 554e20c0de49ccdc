"""The tails of the kernels' walks over their items (open_table.h: for_each_item, for_each_wave_tile,
wave_serial): item counts one below, at and one above a wave (64), a workgroup (256) and a trip of a
one-workgroup grid (1024 items give one workgroup and four trips, 1025 two workgroups and three), so
that the last trip has a single live lane, a full wave or none.  The last item is always one whose
loss changes the answer.  MoleculeCounter against tests/molecules_reference.py /
tests/umi_collapse_reference.py and DeviceCounter against collections.Counter, by exact equality of
integers and of order; nw = 3, ThreeBit, a few hundred reads at most, each reference computed once."""

import functools
from collections import Counter

import numpy as np
import pytest

import test_gpu_molecules_merge as MM
from sctools_amd import _lib, counting

pytestmark = pytest.mark.gpu

NW, KIND = 3, 3
SIZES = [1, 63, 64, 65, 255, 256, 257, 1025]
PREAGG = [0, 1, 2]  # none, wave merge, LDS table
LAST = (2, MM.umi3(4, 4, 4, 4))  # the last read's molecule: no other read has a T in the first base


def _umis(rng, n, L, first_bases):
    """n ThreeBit UMIs of L bases, the first base (the high triplet) drawn from `first_bases`."""
    digits = rng.integers(1, 5, size=(n, L)).astype(np.uint64)
    digits[:, L - 1] = rng.choice(first_bases, size=n)
    return (digits << (np.uint64(3) * np.arange(L, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _reads(n):
    """n reads of L = 4 under 3 barcodes from a pool of about n / 3 UMIs (so molecules repeat, within a
    wave and across trips), some no-match, ambiguous and bad-UMI reads, and LAST as the last read alone.
    (index, umis, snapshot of the reference after them)."""
    rng = np.random.default_rng(1000 + n)
    pool = _umis(rng, max(1, n // 3), 4, [1, 2, 3])
    index = rng.integers(0, NW, size=n).astype(np.int32)
    umis = pool[rng.integers(0, pool.size, size=n)]
    what = rng.random(n)
    index[what < 0.05] = -1
    index[(what >= 0.05) & (what < 0.08)] = -2
    umis[(what >= 0.08) & (what < 0.11)] |= np.uint64(6)  # an N in the last base
    index[-1], umis[-1] = LAST
    ref = MM._ref(NW, KIND, 4, (index, umis))
    assert LAST in ref.seen and ref.mreads[LAST] == 1
    return index, umis, MM._snap(ref)


@pytest.mark.parametrize("preagg", PREAGG)
@pytest.mark.parametrize("n", SIZES)
def test_update_tails(n, preagg):
    """update of n reads, plain and counted, in one batch into a table that does not grow: counts,
    rows, every molecule's reads and parent and the collapse are the reference's."""
    index, umis, snap = _reads(n)
    with _lib.tuning(count_preagg=preagg):
        for counted in (False, True):
            with MM._counter(NW, KIND, 4, counted, [(index, umis)], capacity_hint=4096) as mc:
                info = MM._same(mc, snap)
                assert info["capacity"] == 4096 and info["total"] == n


@functools.lru_cache(maxsize=None)
def _merge_case(m):
    """A source of m molecules of L = 5 with 1-3 reads each, LAST's like among them, and a target fed
    reads of the source's first few molecules and of four of its own.  (src reads, dst reads, snapshot
    of the reference fed dst's reads and then src's)."""
    L = 5
    rng = np.random.default_rng(2000 + m)
    last = (2, MM.umi3(4, 4, 4, 4, 4))
    mols = {last}
    while len(mols) < m:
        mols.add((int(rng.integers(0, NW)), int(_umis(rng, 1, L, [1, 2, 3])[0])))
    mols = sorted(mols)
    rows = rng.permutation(np.repeat(np.arange(m), rng.integers(1, 4, size=m)))
    src = (np.array([mols[r][0] for r in rows], dtype=np.int32), np.array([mols[r][1] for r in rows], dtype=np.uint64))
    own = [(int(rng.integers(0, NW)), int(u)) for u in _umis(rng, 4, L, [4])]
    dst_mols = [mol for mol in mols[:5] + own if mol != last] * 2
    dst = (np.array([d[0] for d in dst_mols], dtype=np.int32), np.array([d[1] for d in dst_mols], dtype=np.uint64))
    ref_src = MM._ref(NW, KIND, L, src)
    assert len(ref_src.seen) == m and last in ref_src.seen
    return src, dst, MM._snap(ref_src), MM._snap(MM._ref(NW, KIND, L, dst, src))


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_dense_merge_tails(m, counted):
    """SCT_TUNE_MERGE_ROWS 1: the source's m occupied rows, compacted, are the merge kernel's items."""
    src, dst, snap_src, snap_both = _merge_case(m)
    with MM._counter(NW, KIND, 5, counted, [dst], capacity_hint=64) as cd, \
            MM._counter(NW, KIND, 5, counted, [src], capacity_hint=64) as cs:
        with _lib.tuning(merge_rows=1):
            assert cd.merge(cs) is cd
        MM._same(cd, snap_both)
        MM._same(cs, snap_src)


@functools.lru_cache(maxsize=None)
def _codes(n):
    """n uint64 codes from a pool of about n / 3, the all-ones code (the table's EMPTY, counted in the
    side slot) among them when n allows, and a code of its own as the last.  (codes, keys in
    first-occurrence order, their counts, their first positions)."""
    rng = np.random.default_rng(3000 + n)
    pool = rng.integers(0, 2 ** 62, size=max(1, n // 3), dtype=np.uint64)
    codes = pool[rng.integers(0, pool.size, size=n)]
    if n >= 63:
        codes[[5, 40]] = np.uint64(2 ** 64 - 1)
    codes[-1] = np.uint64(2 ** 63 + 1)
    seen = Counter(codes.tolist())
    first = {}
    for at, c in enumerate(codes.tolist()):
        first.setdefault(c, at)
    assert seen[2 ** 63 + 1] == 1
    return codes, list(seen), list(seen.values()), [first[c] for c in seen]


@pytest.mark.parametrize("preagg", PREAGG)
@pytest.mark.parametrize("n", SIZES)
def test_counter_update_tails(n, preagg):
    """DeviceCounter.update of n codes in one batch: the rows in first-occurrence order, their counts
    and first positions are collections.Counter's."""
    codes, keys, counts, first = _codes(n)
    with _lib.tuning(count_preagg=preagg), counting.DeviceCounter(capacity_hint=4096) as dc:
        dc.update(codes)
        got = dc.arrays()
        assert [a.tolist() for a in got] == [keys, counts, first]
        assert dc.info() == {"nunique": len(keys), "total": n, "capacity": 4096}
