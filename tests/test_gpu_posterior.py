"""Posterior barcode correction on the device (sctools_amd/csrc/nearest.hip: the deferring query
pass and halves_resolve_kernel) against the brute force of tests/posterior_reference.py: every
index and every distance, exact equality.  All shapes are small; the brute-force scan of a case
is made once and shared by the prior / threshold variants that reuse its inputs."""

import functools

import numpy as np
import pytest

import posterior_reference as R
from sctools_amd import barcode, synthetic

pytestmark = pytest.mark.gpu

ENC = {2: "TwoBit", 3: "ThreeBit"}
ALPHA = "ACGT"
QBYTES = np.array([0, 32, 33, 35, 40, 44, 53, 63, 70, 75, 127, 255], dtype=np.uint8)
W = np.array(R.phred_weights(), dtype=np.uint32)


def codes_of(kind, seqs):
    """(n, L) arrays of base numbers (A C G T = 0..3, alphabetical) -> codes"""
    return np.array([R.encode(kind, "".join(ALPHA[b] for b in s)) for s in seqs], dtype=np.uint64)


def one_off(rng, seq):
    s = seq.copy()
    p = rng.integers(0, s.size)
    s[p] = (s[p] + rng.integers(1, 4)) % 4
    return s


@functools.lru_cache(maxsize=None)
def family(kind, L, order, nq=1257, seed=5):
    """A whitelist of up to 300 L-base codes in which a third of the codes have one to three
    neighbours at distance 1, and queries of every class: exact, one substitution (of a whitelist
    code: distance 1 to it, often to its neighbours too), two substitutions, random, for ThreeBit N
    at the first / the last / a middle base and the invalid triplets 0, 5, 7, and bits above
    kind * L.  Quality bytes include 0, 32, 127 and 255."""
    rng = np.random.default_rng(seed + 100 * L + kind)
    nw = min(300, 4 ** L * 3 // 4)
    pool = {tuple(s) for s in rng.integers(0, 4, size=(nw // 2, L))}
    for s in list(pool)[: nw // 3]:
        for _ in range(int(rng.integers(1, 4))):
            pool.add(tuple(one_off(rng, np.array(s))))
    seqs = sorted(pool)[:nw] if len(pool) > nw else sorted(pool)
    seqs = [np.array(s) for s in seqs]
    if order == "shuffled":
        seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    wl = codes_of(kind, seqs)
    queries = []
    for t in range(nq):
        s = seqs[int(rng.integers(0, len(seqs)))]
        c = t % 8
        if c in (1, 2, 3):
            s = one_off(rng, s)
        elif c == 4:
            s = one_off(rng, one_off(rng, s))
        elif c == 5:
            s = rng.integers(0, 4, size=L)
        q = int(codes_of(kind, [s])[0])
        if kind == 3 and c in (6, 7):  # N or an invalid triplet at the first, last or a middle base
            digit = [L - 1, 0, L // 2][(t // 8) % 3]
            trip = [6, 0, 5, 7][(t // 24) % 4]
            q = (q & ~(7 << (3 * digit))) | (trip << (3 * digit))
            if t % 16 == 7:  # and a second damaged base sometimes: nothing within 1
                q = (q & ~(7 << (3 * ((digit + 1) % L)))) | (6 << (3 * ((digit + 1) % L)))
        if t % 61 == 60:  # bits above the barcode
            q |= 1 << (kind * L + int(rng.integers(0, 64 - kind * L)))
        queries.append(q)
    quals = QBYTES[rng.integers(0, QBYTES.size, size=(nq, L))]
    queries = np.array(queries, dtype=np.uint64)
    return wl, queries, quals, R.scan(kind, L, wl.tolist(), queries.tolist())


def check(wc, L, case, prior, threshold=(39, 40), weights=None, sl=slice(None)):
    wl, queries, quals, scanned = case
    wc.set_prior(prior)
    index, dist = wc.correct(queries[sl], quals[sl], threshold=threshold, quality_weights=weights)
    want_i, want_d = R.decide(L, scanned[sl], quals[sl], prior, W if weights is None else weights, *threshold)
    assert index.dtype == np.int32 and dist.dtype == np.uint8
    bad = np.flatnonzero((index != np.array(want_i, dtype=np.int32)) | (dist != np.array(want_d, dtype=np.uint8)))
    assert bad.size == 0, (bad[:5], index[bad[:5]], np.array(want_i)[bad[:5]], dist[bad[:5]])
    return np.array(want_i)


def priors_for(rng, nw):
    p = rng.integers(1, 1 << 30, size=nw)
    p[rng.random(nw) < 0.25] = 0
    p[rng.random(nw) < 0.25] = 1
    return p


@pytest.mark.parametrize("order", ["alphabetical", "shuffled"])
@pytest.mark.parametrize("L", [2, 5, 16])
@pytest.mark.parametrize("kind", [2, 3])
def test_matches_reference(kind, L, order):
    """1+1 digits, an odd split and the full 8+8; whitelist index = table position, and the
    permuted path; no prior, random priors with zeros, and S{L} quality rows."""
    case = family(kind, L, order)
    wl, queries, quals, _ = case
    rng = np.random.default_rng(L)
    with_prior = priors_for(rng, wl.size)
    wc = barcode.WhitelistCorrector(wl, encoding=ENC[kind], barcode_length=L)
    try:
        assert wc.barcode_length == L
        got = check(wc, L, case, None)
        assert (got >= 0).any() and (got == -2).any() and (got == -1).any()
        check(wc, L, case, with_prior)
        check(wc, L, case, with_prior, threshold=(3, 4))
        check(wc, L, case, None, threshold=(33, 64), weights=np.full(256, 1 << 20, dtype=np.uint32))
        # the rows as fastq.iter_arrays yields them
        as_s = np.ascontiguousarray(quals).view("S%d" % L).reshape(-1)
        wc.set_prior(with_prior)
        a = wc.correct(queries, as_s)
        b = wc.correct(queries, quals)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        wc.close()


@pytest.mark.parametrize("nq", [0, 1])
def test_tiny_batches(nq):
    case = family(3, 16, "shuffled")
    wc = barcode.WhitelistCorrector(case[0], barcode_length=16)
    try:
        for start in (0, 1, 2, 3):
            got = check(wc, 16, case, None, sl=slice(start, start + nq))
            assert got.size == nq
    finally:
        wc.close()


def test_dense_buckets():
    """200 of the 256 four-base codes: every bucket is full of candidates (up to 12 per query)."""
    rng = np.random.default_rng(44)
    for kind, order in ((3, "sorted"), (2, "shuffled")):
        all_seqs = [np.array([a, b, c, d]) for a in range(4) for b in range(4) for c in range(4) for d in range(4)]
        keep = np.sort(rng.permutation(256)[:200])
        if order == "shuffled":
            keep = rng.permutation(keep)
        wl = codes_of(kind, [all_seqs[i] for i in keep])
        queries = codes_of(kind, all_seqs + all_seqs)
        quals = QBYTES[rng.integers(0, QBYTES.size, size=(queries.size, 4))]
        case = (wl, queries, quals, R.scan(kind, 4, wl.tolist(), queries.tolist()))
        wc = barcode.WhitelistCorrector(wl, encoding=ENC[kind], barcode_length=4)
        try:
            got = check(wc, 4, case, None, threshold=(3, 4))
            assert (got == -2).sum() > 20 and (got >= 0).sum() > 200
            check(wc, 4, case, priors_for(rng, 200))
        finally:
            wc.close()


def test_duplicated_code_and_long_bucket():
    """A code at two indices is two candidates (and a tie at distance 0); 300 codes that share their
    first 8 bases make an A bucket of more than 256 entries (no rank table, many 24-entry groups)."""
    rng = np.random.default_rng(9)
    L = 16
    head = rng.integers(0, 4, size=8)
    tails = sorted({tuple(t) for t in rng.integers(0, 4, size=(400, 8))})[:300]
    seqs = [np.concatenate([head, np.array(t)]) for t in tails]
    other = [rng.integers(0, 4, size=L) for _ in range(40)]
    for kind in (2, 3):
        for order in ("sorted", "shuffled"):
            s = sorted([tuple(x) for x in seqs + other + [seqs[7], other[3]]])
            s = [np.array(x) for x in s]
            if order == "shuffled":
                s = [s[i] for i in rng.permutation(len(s))]
            wl = codes_of(kind, s)
            qs = [one_off(rng, s[int(rng.integers(0, len(s)))]) for _ in range(300)]
            qs += [seqs[7], other[3], seqs[8]]
            # one substitution in the shared head: the candidates come through the B table
            for k in range(40):
                x = seqs[k].copy()
                x[k % 8] = (x[k % 8] + 1 + k % 3) % 4
                qs.append(x)
            queries = codes_of(kind, qs)
            quals = QBYTES[rng.integers(0, QBYTES.size, size=(queries.size, L))]
            case = (wl, queries, quals, R.scan(kind, L, wl.tolist(), queries.tolist()))
            wc = barcode.WhitelistCorrector(wl, encoding=ENC[kind], barcode_length=L)
            try:
                got = check(wc, L, case, None)
                assert got[300] == -2 and got[301] == -2 and got[302] >= 0
                check(wc, L, case, priors_for(rng, wl.size), threshold=(3, 4))
            finally:
                wc.close()


@functools.lru_cache(maxsize=None)
def clusters(kind):
    """60 random 16-base centres that are not in the whitelist; centre i brings k = 1, 2, 3, 4, 8 or
    all 48 of its neighbours.  The queries are the centres, at quality byte 70 with two random
    positions drawn from 33..44."""
    rng = np.random.default_rng(2024)
    L = 16
    centres = [rng.integers(0, 4, size=L) for _ in range(60)]
    seqs = []
    for i, c in enumerate(centres):
        k = [1, 2, 3, 4, 8, 48][i % 6]
        nb = [(p, b) for p in range(L) for b in range(1, 4)]
        for t in rng.permutation(48)[:k]:
            s = c.copy()
            s[nb[t][0]] = (s[nb[t][0]] + nb[t][1]) % 4
            seqs.append(s)
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    wl = codes_of(kind, seqs)
    queries = codes_of(kind, centres)
    quals = np.full((60, L), 70, dtype=np.uint8)
    for r in range(60):
        quals[r, rng.permutation(L)[:2]] = rng.integers(33, 45, size=2)
    scanned = R.scan(kind, L, wl.tolist(), queries.tolist())
    assert all(row[0] == "near" for row in scanned)
    return wl, queries, quals, scanned


@pytest.mark.parametrize("threshold", [(39, 40), (3, 4)])
@pytest.mark.parametrize("prior_kind", ["ones", "random", "zero_one"])
@pytest.mark.parametrize("kind", [2, 3])
def test_clusters(kind, prior_kind, threshold):
    case = clusters(kind)
    wl, _, _, scanned = case
    rng = np.random.default_rng(7)
    prior = {"ones": None, "random": rng.integers(1, 1 << 30, size=wl.size),
             "zero_one": rng.integers(0, 2, size=wl.size)}[prior_kind]
    wc = barcode.WhitelistCorrector(wl, encoding=ENC[kind], barcode_length=16)
    try:
        want = check(wc, 16, case, prior, threshold=threshold)
    finally:
        wc.close()
    # the input must reach both outcomes of a query with several candidates (prior > 0), under the
    # reference; and with 0/1 priors a good share of the queries keeps no candidate at all
    assert sum(len(row[1]) >= 2 for row in scanned) == 50
    multi = np.array([sum(prior is None or prior[j] > 0 for j, _ in row[1]) >= 2 for row in scanned])
    outcomes = [(want[multi] >= 0).mean(), (want[multi] == -2).mean()]
    if prior_kind == "zero_one":
        outcomes.append((want == -1).mean())
    assert multi.sum() >= 30 and min(outcomes) >= 0.10, outcomes


@pytest.mark.parametrize("kind", [2, 3])
def test_worst_case_sums(kind):
    """48 candidates at prior 2^30 - 1 and weight 2^20 with den = 64: the largest products."""
    case = clusters(kind)
    wl = case[0]
    heavy = np.full(256, 1 << 20, dtype=np.uint32)
    top = np.full(wl.size, (1 << 30) - 1, dtype=np.int64)
    wc = barcode.WhitelistCorrector(wl, encoding=ENC[kind], barcode_length=16)
    try:
        for threshold in ((33, 64), (64, 64)):
            want = check(wc, 16, case, top, threshold=threshold, weights=heavy)
            assert (want == -2).sum() == 50 and (want >= 0).sum() == 10
        lone = top.copy()
        lone[1::2] = 1  # one heavy candidate among light ones wins at 63/64
        check(wc, 16, case, lone, threshold=(63, 64), weights=heavy)
    finally:
        wc.close()


def test_prior_changes_between_calls():
    case = family(3, 16, "shuffled")
    wl = case[0]
    rng = np.random.default_rng(3)
    a, b = priors_for(rng, wl.size), priors_for(rng, wl.size)
    wc = barcode.WhitelistCorrector(wl, barcode_length=16)
    try:
        ia = check(wc, 16, case, a, threshold=(3, 4))
        ib = check(wc, 16, case, b, threshold=(3, 4))
        assert (ia != ib).any()
        check(wc, 16, case, None, threshold=(3, 4))
        assert np.array_equal(check(wc, 16, case, a, threshold=(3, 4)), ia)
    finally:
        wc.close()


def test_two_slots_and_counts():
    """devices=[0, 0]: contiguous query and quality ranges per slot, the prior on both; and
    count_corrected over three batches equals the bincount of correct."""
    case = family(3, 16, "shuffled")
    wl, queries, quals, _ = case
    prior = priors_for(np.random.default_rng(8), wl.size)
    for devices in (None, [0, 0]):
        wc = barcode.WhitelistCorrector(wl, barcode_length=16, devices=devices)
        try:
            want = check(wc, 16, case, prior, threshold=(3, 4))
            acc = None
            for sl in (slice(0, 400), slice(400, 401), slice(401, None)):
                acc = wc.count_corrected(queries[sl], quals[sl], out=acc, threshold=(3, 4))
            counts, n_none, n_amb = acc
            assert counts.dtype == np.int64
            assert np.array_equal(counts, np.bincount(want[want >= 0], minlength=wl.size))
            assert (n_none, n_amb) == ((want == -1).sum(), (want == -2).sum())
            assert wc.count_corrected(queries[:0], quals[:0], out=acc, threshold=(3, 4))[1:] == (n_none, n_amb)
        finally:
            wc.close()


def test_agrees_with_nearest_where_it_answers():
    """All priors positive: wherever nearest answers an index or -1, correct answers the same (and
    the same distance); they differ only where nearest says -2 at distance 1."""
    wl2 = synthetic.whitelist_codes(5000, 16, seed=12)
    wl3 = synthetic.two_to_three(wl2)
    q, _, _ = synthetic.config4_queries(wl3, 20000, seed=4)
    queries = q.cpu().numpy().view(np.uint64)
    rng = np.random.default_rng(1)
    quals = rng.integers(33, 75, size=(queries.size, 16)).astype(np.uint8)
    wc = barcode.WhitelistCorrector(wl3, barcode_length=16)
    try:
        ni, nd = wc.nearest(queries)
        for prior in (None, rng.integers(1, 1000, size=wl3.size)):
            wc.set_prior(prior)
            ci, cd = wc.correct(queries, quals)
            same = ~((ni == -2) & (nd == 1))
            assert np.array_equal(ci[same], ni[same]) and np.array_equal(cd[same], nd[same])
            assert ((ci[~same] == -2) | (ci[~same] >= 0)).all() and (cd[~same] == 1).all()
            assert int(wc.last_stats[1]) <= int(wc.last_stats[0]) <= queries.size
    finally:
        wc.close()


def test_other_plans_are_refused():
    seqs = ["ACGTACGT", "ACGTACGA", "TTTTACGT"]
    q = np.array([R.encode(3, "ACGTACGC")], dtype=np.uint64)
    quals = np.full((1, 8), 40, dtype=np.uint8)
    with_n = np.array([R.encode(3, s) for s in seqs + ["ACNTACGT"]], dtype=np.uint64)
    for wc in (barcode.WhitelistCorrector(with_n, barcode_length=8),
               barcode.WhitelistCorrector(with_n[:3], max_distance=2, barcode_length=8)):
        try:
            with pytest.raises(ValueError, match="half-key"):
                wc.correct(q, quals)
            with pytest.raises(ValueError, match="half-key"):
                wc.count_corrected(q, quals)
        finally:
            wc.close()


def test_arguments():
    wl = np.array([R.encode(2, s) for s in ["AACGT", "AACGA", "ATTTT"]], dtype=np.uint64)
    q = np.array([R.encode(2, "AACGC")], dtype=np.uint64)
    # the first bases are all A: only barcode_length tells the index there are five
    wc = barcode.WhitelistCorrector(wl, encoding="TwoBit", barcode_length=5)
    try:
        assert wc.barcode_length == 5
        with pytest.raises(ValueError, match="barcode_length"):
            wc.correct(q, np.full((1, 4), 40, dtype=np.uint8))
        with pytest.raises(ValueError):
            wc.correct(q, np.full((2, 5), 40, dtype=np.uint8))
        with pytest.raises(ValueError):
            wc.set_prior([1, 2])
        with pytest.raises(ValueError):
            wc.set_prior([1, 2, 1 << 30])
        for threshold in ((1, 2), (0, 1), (65, 65), (3, 2)):
            with pytest.raises(ValueError):
                wc.correct(q, np.full((1, 5), 40, dtype=np.uint8), threshold=threshold)
        for bad in (0, (1 << 20) + 1):
            w = W.copy()
            w[200] = bad
            with pytest.raises(ValueError):
                wc.correct(q, np.full((1, 5), 40, dtype=np.uint8), quality_weights=w)
        wc.set_prior([3, 1, 5])
        quals = np.full((1, 5), 40, dtype=np.uint8)
        assert [a.tolist() for a in wc.correct(q, quals, threshold=(3, 4))] == [[0], [1]]
        assert [a.tolist() for a in wc.correct(q, quals, threshold=(4, 5))] == [[-2], [1]]
    finally:
        wc.close()
    empty = barcode.WhitelistCorrector(np.zeros(0, dtype=np.uint64), barcode_length=5)
    assert [a.tolist() for a in empty.correct(q, np.full((1, 5), 40, dtype=np.uint8))] == [[-1], [255]]
    assert empty.count_corrected(q, np.full((1, 5), 40, dtype=np.uint8))[1:] == (1, 0)


def test_prior_barcode_set_corrector():
    keys = {R.encode(2, "ACGT"): 3, R.encode(2, "ACGA"): 1, R.encode(2, "TTTT"): 5}
    pbs = barcode.PriorBarcodeSet(keys, 4)
    quals = np.full((1, 4), 40, dtype=np.uint8)
    for enc, kind in (("TwoBit", 2), ("ThreeBit", 3)):
        wc = pbs.corrector(encoding=enc)
        try:
            q = np.array([R.encode(kind, "ACGC")], dtype=np.uint64)
            assert [a.tolist() for a in wc.correct(q, quals, threshold=(3, 4))] == [[0], [1]]
            assert [a.tolist() for a in wc.correct(q, quals, threshold=(4, 5))] == [[-2], [1]]
        finally:
            wc.close()
