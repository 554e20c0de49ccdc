"""CPU: the downsampling contract's Python restatement (tests/downsample_reference.py) on its own --
the ends of the threshold range, nestedness, independence of the order of updates, the mapping of a
fraction to a threshold, and a statistical sanity check of the draw.  The device is compared with the
reference by exact equality elsewhere (tests/test_gpu_downsample.py); the bounds on z here are a
condition on the draw itself, chosen with margin over what the reference gave (2.04 and 1.55)."""

import math
import random

import numpy as np
import pytest

import count_matrix_reference as C
import downsample_reference as D
import umi_collapse_reference as U
from sctools_amd import counting

TOP = 2 ** 64 - 1


def _reads(seed, n=3000, nw=7, L=4):
    """n ThreeBit reads of about n / 4 molecules, with no-match, ambiguous and bad-UMI reads."""
    rng = random.Random(seed)
    mols = [(rng.randrange(nw), sum(rng.choice((1, 2, 3, 4)) << (3 * p) for p in range(L))) for _ in range(n // 4)]
    out = []
    for _ in range(n):
        i, u = rng.choice(mols)
        x = rng.random()
        out.append((-1, u) if x < 0.04 else (-2, u) if x < 0.06 else (i, u | 6) if x < 0.08 else (i, u))
    return out


def _fed(reads, nw=7, L=4, batches=1):
    ref = U.CountedMolecules(nw, 3, L)
    step = (len(reads) + batches - 1) // batches
    for b in range(0, len(reads), step):
        ref.update([r[0] for r in reads[b:b + step]], [r[1] for r in reads[b:b + step]])
    return ref


def _shown(ref):
    return ref.counts(), sorted(ref.mreads.items()), ref.total


def test_threshold_ends_keep_nothing_and_everything():
    for seed in (0, 1, TOP):
        for key in (0, 2 ** 63 - 1, D.tally_key(0), D.tally_key(3)):
            for r in (0, 1, 5, 300):
                assert D.thin(seed, key, r, 0) == 0
                assert D.thin(seed, key, r, 2 ** 32) == r
    src = _fed(_reads(1))
    assert all(t > 0 for t in src.tally)
    none = D.downsample(src, 0, 9, U.CountedMolecules(7, 3, 4))
    assert _shown(none) == _shown(U.CountedMolecules(7, 3, 4)) and none.total == 0
    everything = D.downsample(src, 2 ** 32, 9, U.CountedMolecules(7, 3, 4))
    assert _shown(everything) == _shown(src) and everything.seen == src.seen
    assert D.curve(src, [0, 2 ** 32], 9) == ([0, sum(src.reads)], [0, sum(src.molecules)])


def test_nested_in_the_threshold_and_monotone_in_the_reads():
    rng = random.Random(3)
    thresholds = sorted(rng.randrange(2 ** 32 + 1) for _ in range(12))
    for _ in range(50):
        seed, key, r = rng.getrandbits(64), rng.getrandbits(63), rng.randrange(1, 40)
        ds = D.draws(seed, key, r)
        assert ds == [D.draw(seed, key, j) for j in range(r)]
        kept = [{j for j in range(r) if ds[j] < T} for T in thresholds]
        assert all(a <= b for a, b in zip(kept, kept[1:]))
        assert [len(s) for s in kept] == [D.thin(seed, key, r, T) for T in thresholds]
        for T in thresholds[::4]:
            by_r = [D.thin(seed, key, n, T) for n in range(r + 1)]
            assert all(0 <= b - a <= 1 for a, b in zip(by_r, by_r[1:]))
    src = _fed(_reads(2))
    reads, molecules = D.curve(src, thresholds, 77)
    assert reads == sorted(reads) and molecules == sorted(molecules)
    for t, T in enumerate(thresholds):
        into = D.downsample(src, T, 77, U.CountedMolecules(7, 3, 4))
        assert (sum(into.reads), sum(into.molecules)) == (reads[t], molecules[t])
        assert into.total == reads[t] + sum(into.tally)
        assert all(v >= 1 for v in into.mreads.values())


def test_the_order_of_updates_changes_nothing():
    reads = _reads(4)
    shuffled = list(reads)
    random.Random(8).shuffle(shuffled)
    a, b, c = _fed(reads), _fed(shuffled, batches=5), _fed(reads[::-1], batches=2)
    assert _shown(a) == _shown(b) == _shown(c)
    for T in (1, 2 ** 29, 2 ** 31, 2 ** 32 - 1):
        thinned = [_shown(D.downsample(x, T, 5, U.CountedMolecules(7, 3, 4))) for x in (a, b, c)]
        assert thinned[0] == thinned[1] == thinned[2]
    # twice the same call: the same reads again, no new molecule
    once = D.downsample(a, 2 ** 31, 5, U.CountedMolecules(7, 3, 4))
    twice = D.downsample(a, 2 ** 31, 5, D.downsample(a, 2 ** 31, 5, U.CountedMolecules(7, 3, 4)))
    assert twice.molecules == once.molecules and twice.reads == [2 * x for x in once.reads]
    assert twice.total == 2 * once.total and twice.tally == [2 * x for x in once.tally]


def test_a_feature_counter_thins_four_tallies_under_its_three_part_keys():
    rng = random.Random(6)
    fm = C.FeatureMolecules(7, 5, 3, 4)
    reads = _reads(5, n=1500)
    fm.update([r[0] for r in reads], [r[1] for r in reads], [rng.choice((-1, 0, 1, 2, 3, 4)) for _ in reads])
    assert fm.n_no_feature > 0
    into = D.downsample(fm, 2 ** 31, 3, C.FeatureMolecules(7, 5, 3, 4))
    assert into.tally == [D.thin_tally(3, k, fm.tally[k], 2 ** 31) for k in range(4)]
    for (i, f, u), m in into.mreads.items():
        assert m == D.thin(3, C.key(i, f, u, 5, 3, 4), fm.mreads[(i, f, u)], 2 ** 31)
    assert into.total == sum(into.reads) + sum(into.tally)


def test_fraction_to_threshold():
    below_one = math.nextafter(1.0, 0.0)
    want = {0: 0, 0.0: 0, 1: 2 ** 32, 1.0: 2 ** 32, 0.5: 2 ** 31, 2.0 ** -33: 0, below_one: 2 ** 32, 0.1: 429496730,
            0.25: 2 ** 30}
    for fraction, threshold in want.items():
        assert counting.downsample_threshold(fraction) == threshold == D.downsample_threshold(fraction), fraction
    for fraction in (-0.1, -2.0 ** -60, math.nextafter(1.0, 2.0), 2, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            counting.downsample_threshold(fraction)
        with pytest.raises(ValueError):
            D.downsample_threshold(fraction)


def _mix64_np(x):
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xff51afd7ed558ccd)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xc4ceb9fe1a85ec53)
    return x ^ (x >> np.uint64(33))


def _draws_np(seed, keys, j):
    """draw(seed, key, j) of every key (and, j an array, of every j of one key), with numpy."""
    with np.errstate(over="ignore"):
        streams = _mix64_np(keys ^ np.uint64(D.mix64(seed ^ D.G)))
        step = (np.asarray(j, dtype=np.uint64) + np.uint64(1)) * np.uint64(D.G)
        return _mix64_np(streams + step) >> np.uint64(32)


def test_the_draw_is_statistically_sane():
    """200,000 keys i | (i // 200) << 30 with 4 reads each, seeds 0, 1 and 12345, thresholds 2^30, 2^31
    and 429496730: the reads kept against the binomial and the molecules that survive against
    1 - (1 - p)^4, |z| <= 4 each; one key with 10^6 reads at p = 0.25 likewise."""
    n, r = 200000, 4
    i = np.arange(n, dtype=np.uint64)
    keys = i | ((i // np.uint64(200)) << np.uint64(30))
    for seed in (0, 1, 12345):
        d = np.stack([_draws_np(seed, keys, j) for j in range(r)])
        for k in (0, 1999, 123456):  # the numpy draw is the reference's
            assert d[:, k].tolist() == D.draws(seed, int(keys[k]), r)
        for T in (2 ** 30, 2 ** 31, 429496730):
            p = T / 2 ** 32
            kept = d < np.uint64(T)
            z_reads = (int(kept.sum()) - n * r * p) / math.sqrt(n * r * p * (1 - p))
            q = 1 - (1 - p) ** r
            z_molecules = (int(kept.any(axis=0).sum()) - n * q) / math.sqrt(n * q * (1 - q))
            assert abs(z_reads) <= 4 and abs(z_molecules) <= 4, (seed, T, z_reads, z_molecules)
    m = 10 ** 6
    d = _draws_np(0, np.uint64(12345), np.arange(m, dtype=np.uint64))
    assert d[:5].tolist() == D.draws(0, 12345, 5)
    z = (int((d < np.uint64(2 ** 30)).sum()) - m * 0.25) / math.sqrt(m * 0.25 * 0.75)
    assert abs(z) <= 4, z
