"""Collapsing UMIs one base apart on the device (sctools_amd/csrc/molecules.hip): a
MoleculeCounter(read_counts=True) against tests/umi_collapse_reference.py, the contract in plain
Python.  Every comparison is exact equality of integers and of order; there is no tolerance
anywhere.  All shapes are a few thousand reads, every case runs under each pre-aggregation form of
the insert (SCT_TUNE_COUNT_PREAGG), and a case's input and reference are computed once for the three
forms."""

import functools
import math

import numpy as np
import pytest

import umi_collapse_reference as U
from sctools_amd import _lib, counting

pytestmark = pytest.mark.gpu

PREAGG = [0, 1, 2]  # none, wave merge, LDS table
ENC = {3: "ThreeBit", 2: "TwoBit"}


def _snap(ref):
    """Everything the device counter is compared with, taken from the reference as it stands."""
    return {"counts": ref.counts(), "pairs": ref.pairs_counted(), "collapse": ref.collapse(), "total": ref.total,
            "saturation": ref.saturation(), "saturation_collapsed": ref.saturation_collapsed()}


def _same_float(a, b):
    return type(a) is float and (a == b or (math.isnan(a) and math.isnan(b)))


def _same(mc, snap, nw):
    """counts(), pairs() in all three forms, info(), len(), collapse() and both saturations of the
    device counter = the reference's."""
    reads, molecules, n_none, n_amb, n_bad = mc.counts()
    assert reads.dtype == np.int64 and molecules.dtype == np.int64 and reads.shape == molecules.shape == (nw,)
    assert (reads.tolist(), molecules.tolist(), n_none, n_amb, n_bad) == snap["counts"]
    rows = snap["pairs"]
    index, umi = mc.pairs()
    assert index.dtype == np.int32 and umi.dtype == np.uint64
    assert list(zip(index.tolist(), umi.tolist())) == [r[:2] for r in rows]
    three = mc.pairs(reads=True)
    assert len(three) == 3 and three[2].dtype == np.int64
    assert list(zip(*(a.tolist() for a in three))) == [r[:3] for r in rows]
    four = mc.pairs(reads=True, parents=True)
    assert [a.dtype for a in four] == [np.int32, np.uint64, np.int64, np.uint64]
    assert list(zip(*(a.tolist() for a in four))) == rows
    info = mc.info()
    assert info["nmolecules"] == len(rows) == len(mc) == int(molecules.sum()) and info["total"] == snap["total"]
    collapsed, n_corrected = mc.collapse()
    assert collapsed.dtype == np.int64 and collapsed.shape == (nw,) and type(n_corrected) is int
    assert (collapsed.tolist(), n_corrected) == snap["collapse"]
    again = mc.collapse()  # it reads only: the same answer, and nothing else moved
    assert (again[0].tolist(), again[1]) == snap["collapse"]
    assert int(four[2].sum()) == int(reads.sum())
    assert _same_float(mc.saturation(), snap["saturation"])
    assert _same_float(mc.saturation(collapsed=True), snap["saturation_collapsed"])
    return info


def _arrays(reads):
    return (np.array([r[0] for r in reads], dtype=np.int32), np.array([r[1] for r in reads], dtype=np.uint64))


def umi3(*bases):
    """A ThreeBit code written first base first (the first base in the high triplet)."""
    code = 0
    for b in bases:
        code = (code << 3) | b
    return code


C, A, G, T = 1, 2, 3, 4


def _mutated_family(kind, L, nw, nroots, seed):
    """nroots random UMIs under random barcodes, a geometric(0.25) number of reads each, every base of
    every read replaced by another base with probability 4 %; shuffled."""
    rng = np.random.default_rng(seed)
    lo = 1 if kind == 3 else 0
    roots = rng.integers(lo, lo + 4, size=(nroots, L))
    barcode = rng.integers(0, nw, size=nroots)
    rows = np.repeat(np.arange(nroots), rng.geometric(0.25, size=nroots))
    d = roots[rows]
    hit = rng.random(d.shape) < 0.04
    d = np.where(hit, (d - lo + rng.integers(1, 4, size=d.shape)) % 4 + lo, d).astype(np.uint64)
    umis = (d << (np.uint64(kind) * np.arange(L, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    perm = rng.permutation(rows.size)
    return barcode[rows][perm].astype(np.int32), umis[perm]


def _star(L, barcodes, hub_reads):
    """Under every barcode: one hub with hub_reads reads and its 3 * L neighbours with one read each."""
    hub = sum(((p % 4) + 1) << (3 * p) for p in range(L))
    reads = []
    for b in barcodes:
        reads += [(b, hub)] * hub_reads + [(b, v) for v in U.neighbours(hub, 3, L)]
    return reads


@functools.lru_cache(maxsize=None)
def _case(name):
    """(nw, kind, L, capacity_hint, batches, snapshot after every batch) of a named case."""
    hint = 64
    rng = np.random.default_rng(len(name))
    if name == "empty":
        nw, kind, L, reads = 3, 3, 2, []
    elif name == "chain":
        nw, kind, L = 1, 3, 2
        reads = [(0, umi3(A, A))] + [(0, umi3(A, C))] * 2 + [(0, umi3(G, C))] * 5
    elif name == "tie":  # AA x 1 between CA x 3 and TA x 3; GG x 1 between GC x 3 and GA x 3 (barcode 1)
        nw, kind, L = 2, 3, 2
        reads = [(0, umi3(A, A))] + [(0, umi3(C, A))] * 3 + [(0, umi3(T, A))] * 3
        reads += [(1, umi3(G, G))] + [(1, umi3(G, C))] * 3 + [(1, umi3(G, A))] * 3
    elif name == "equal_pair":
        nw, kind, L = 1, 3, 2
        reads = [(0, umi3(A, C))] * 4 + [(0, umi3(A, G))] * 4
    elif name == "length_one":
        nw, kind, L = 2, 3, 1
        reads = [(1, C)] * 2 + [(1, A)] * 7 + [(1, G)] * 7 + [(1, T)]
    elif name == "length_one_twobit":
        nw, kind, L = 1, 2, 1
        reads = [(0, 0), (0, 3)]
    elif name == "two_barcodes":
        nw, kind, L = 3, 3, 2
        reads = [(0, umi3(A, A)), (1, umi3(A, A)), (1, umi3(A, A))] + [(2, umi3(A, C))] * 9
    elif name == "star":
        nw, kind, L = 1, 3, 10
        reads = _star(L, [0], 40)
    elif name == "star50":
        nw, kind, L = 64, 3, 10
        reads = _star(L, range(7, 57), 3)
    elif name == "corner63":  # TwoBit, 15 + 48 = 63 key bits: the top key, all its UMI neighbours, and
        nw, kind, L = 2 ** 15, 2, 24  # the same UMIs under the index one bit away, which are unrelated
        top = 2 ** 48 - 1
        reads = [(32767, top)] * 5 + [(32767, v) for v in U.neighbours(top, 2, L)]
        reads += [(32766, top)] + [(32766, v) for v in U.neighbours(top, 2, L)[:9]] * 2
        reads += [(0, 0), (0, 1), (0, 1), (16383, top)]
    elif name == "copies":
        nw, kind, L = 10, 3, 4
        reads = [(7, int("1234", 8))] * 5000
    elif name == "bad_mixed":  # N, invalid triplets and a high bit one base away from stored UMIs; -1 / -2
        nw, kind, L = 5, 3, 4
        good = int("1234", 8)
        reads = [(2, good)] * 3 + [(2, int("1231", 8))]
        for pos in range(L):
            for t in (0, 5, 6, 7):
                reads += [(2, (good & ~(7 << (3 * pos))) | (t << (3 * pos)))] * 4
        reads += [(2, good | (1 << 12))] * 6 + [(-1, int("1233", 8))] * 7 + [(-2, int("1232", 8))] * 7
        reads += [(-1, good), (-2, good), (4, int("4444", 8)), (4, int("4443", 8)), (4, int("4443", 8))]
    elif name == "growth":  # 750 roots and three one-base neighbours of each, 1-4 reads a molecule
        nw, kind, L = 37, 3, 10
        g = np.random.default_rng(23)
        molecules = set()
        for _ in range(750):
            b = int(g.integers(0, nw))
            root = sum(int(d) << (3 * p) for p, d in enumerate(g.integers(1, 5, size=L)))
            nbs = U.neighbours(root, kind, L)
            molecules |= {(b, root)} | {(b, nbs[j]) for j in g.permutation(3 * L)[:3]}
        molecules = sorted(molecules)
        rows = np.repeat(np.arange(len(molecules)), g.integers(1, 5, size=len(molecules)))
        index, umis = _arrays([molecules[r] for r in g.permutation(rows)])
    elif name == "family_3_5_3":
        nw, kind, L = 3, 3, 5
        index, umis = _mutated_family(kind, L, nw, 300, 101)
    elif name == "family_2_4_2":
        nw, kind, L = 2, 2, 4
        index, umis = _mutated_family(kind, L, nw, 120, 102)
    elif name == "family_3_10_37":
        nw, kind, L = 37, 3, 10
        index, umis = _mutated_family(kind, L, nw, 2000, 103)
        hint = 1 << 14
    else:
        raise KeyError(name)
    if not name.startswith(("growth", "family")):
        index, umis = _arrays([reads[i] for i in rng.permutation(len(reads))])
    n = index.size
    cuts = [0, n // 3, 2 * n // 3, n] if name == "growth" else [0, n]
    batches = [(index[a:b], umis[a:b]) for a, b in zip(cuts, cuts[1:])]
    ref = U.CountedMolecules(nw, kind, L)
    snaps = [_snap(ref.update(*batch)) for batch in batches]
    return nw, kind, L, hint, batches, snaps, ref


def _run_case(name, preagg, check=None):
    nw, kind, L, hint, batches, snaps, ref = _case(name)
    with _lib.tuning(count_preagg=preagg):
        with counting.MoleculeCounter(nw, L, encoding=ENC[kind], capacity_hint=hint, read_counts=True) as mc:
            for batch, snap in zip(batches, snaps):
                assert mc.update(*batch) is mc
                info = _same(mc, snap, nw)
            if check:
                check(mc)
    return snaps[-1], info, ref


@pytest.mark.parametrize("preagg", PREAGG)
def test_hand_cases(preagg):
    """The contract's hand cases on the device: the AA / AC / GC chain (2 images, not 1 root), ties to
    the larger code, two equal neighbours of which one moves, L = 1, one UMI under two barcodes, and a
    counter that was fed nothing."""
    snap, _, ref = _run_case("chain", preagg)
    assert snap["collapse"] == ([2], 2) and ref.roots() == [1]
    assert snap["pairs"] == [(0, umi3(A, C), 2, umi3(G, C)), (0, umi3(A, A), 1, umi3(A, C)),
                             (0, umi3(G, C), 5, umi3(G, C))]
    snap, _, _ = _run_case("tie", preagg)
    assert snap["collapse"] == ([1, 1], 4)  # CA -> TA and GC -> GA too: equal reads, the larger code
    assert (0, umi3(A, A), 1, umi3(T, A)) in snap["pairs"] and (1, umi3(G, G), 1, umi3(G, A)) in snap["pairs"]
    assert _run_case("equal_pair", preagg)[0]["collapse"] == ([1], 1)
    assert _run_case("length_one", preagg)[0]["collapse"] == ([0, 1], 3)
    assert _run_case("length_one_twobit", preagg)[0]["collapse"] == ([1], 1)
    assert _run_case("two_barcodes", preagg)[0]["collapse"] == ([1, 1, 1], 0)
    assert _run_case("empty", preagg)[0]["collapse"] == ([0, 0, 0], 0)  # nothing fed: zeros written, nan saturation


@pytest.mark.parametrize("preagg", PREAGG)
def test_star(preagg):
    """One hub and its 30 one-read neighbours, L = 10: 31 lanes claim one bitmap bit, and exactly one
    of them counts.  Then the same star under 50 barcodes in one batch."""
    snap, info, _ = _run_case("star", preagg)
    assert snap["collapse"] == ([1], 30) and info["nmolecules"] == 31
    snap, info, _ = _run_case("star50", preagg)
    want = [1 if 7 <= b < 57 else 0 for b in range(64)]
    assert snap["collapse"] == (want, 30 * 50) and info["nmolecules"] == 31 * 50


@pytest.mark.parametrize("preagg", PREAGG)
def test_the_63_bit_corner(preagg):
    """Key 2^63 - 1 with all 72 UMI neighbours present: they collapse into it, and the same UMIs under
    index 32766 (one index bit away) stay where they are."""
    snap, _, _ = _run_case("corner63", preagg)
    collapsed, n_corrected = snap["collapse"]
    assert collapsed[32767] == 1 and snap["counts"][1][32767] == 73
    assert snap["pairs"][-1] == (32767, 2 ** 48 - 1, 5, 2 ** 48 - 1)
    assert all(r[3] == 2 ** 48 - 1 for r in snap["pairs"] if r[0] == 32767)
    # under 32766: top x 1 and nine neighbours x 2 -- top moves to its best neighbour, not across
    assert [r[3] for r in snap["pairs"] if r[:2] == (32766, 2 ** 48 - 1)] != [2 ** 48 - 1]
    assert collapsed[0] == 1 and collapsed[16383] == 1
    assert n_corrected == 72 + sum(r[1] != r[3] for r in snap["pairs"] if r[0] != 32767)


@pytest.mark.parametrize("preagg", PREAGG)
def test_forced_growth(preagg):
    """capacity_hint=64 and about 3,000 molecules in three batches, everything compared after every
    batch (collapse twice): counts survive at least four rehashes, and collapse in mid-stream
    disturbs nothing."""
    snap, info, _ = _run_case("growth", preagg)
    assert 2500 <= info["nmolecules"] <= 3500 and info["capacity"] >= 64 * 2 ** 4
    assert max(r[2] for r in snap["pairs"]) >= 4 and snap["collapse"][1] > 100


@pytest.mark.parametrize("preagg", PREAGG)
@pytest.mark.parametrize("name", ["family_3_5_3", "family_2_4_2", "family_3_10_37"])
def test_mutated_families(name, preagg):
    """Random roots with geometric reads and 4 % substitutions per base.  The input is first shown, on
    the reference alone, to hold a chain (a corrected molecule whose parent is itself corrected), a
    parent chosen among equal reads by code, and a barcode whose images are not its roots: a kernel
    that counts roots or ignores ties cannot pass."""
    nw, kind, L, _, _, snaps, ref = _case(name)
    parent = {(i, u): p for i, u, _, p in snaps[-1]["pairs"]}
    chains = sum(p != u and parent[(i, p)] != p for (i, u), p in parent.items())
    ties = 0
    for (i, u), p in parent.items():
        stored = [v for v in [u] + U.neighbours(u, kind, L) if (i, v) in parent]
        ties += sum(ref.mreads[(i, v)] == ref.mreads[(i, p)] for v in stored) > 1
    assert chains >= 1 and ties >= 1 and snaps[-1]["collapse"][0] != ref.roots(), (chains, ties)
    _run_case(name, preagg)


@pytest.mark.parametrize("name", ["chain", "tie", "length_one", "star50", "corner63", "growth", "family_2_4_2",
                                  "family_3_10_37"])
def test_a_lane_per_slot_gives_the_same(name):
    """SCT_TUNE_COLLAPSE_FORM 0, one lane per table slot, against the default, in which the lanes of a
    wave share one molecule's neighbours (corner63 has 72 of them, more than a wave has lanes) and
    reduce by the rule's order.  Every number as before."""
    assert _lib.tune_get("collapse_form") == -1  # every other test runs the default form
    with _lib.tuning(collapse_form=0):
        _run_case(name, 1)


@pytest.mark.parametrize("preagg", PREAGG)
def test_many_copies_of_one_read(preagg):
    snap, _, _ = _run_case("copies", preagg)
    assert snap["pairs"] == [(7, int("1234", 8), 5000, int("1234", 8))] and snap["collapse"][1] == 0


@pytest.mark.parametrize("preagg", PREAGG)
def test_bad_umis_and_missing_barcodes_are_nobodys_neighbour(preagg):
    """Reads with N, an invalid triplet or a high bit, and reads under -1 / -2, all one base away from
    stored UMIs and with more reads than they: none is stored, none is a parent."""
    snap, _, _ = _run_case("bad_mixed", preagg)
    assert snap["pairs"] == [(2, int("1231", 8), 1, int("1234", 8)), (2, int("1234", 8), 3, int("1234", 8)),
                             (4, int("4443", 8), 2, int("4443", 8)), (4, int("4444", 8), 1, int("4443", 8))]
    assert snap["collapse"] == ([0, 0, 1, 0, 1], 2)
    assert snap["counts"][2:] == (8, 8, 4 * 4 * 4 + 6)


@pytest.mark.parametrize("preagg", PREAGG)
def test_two_streams(preagg):
    """update_device on one stream, then collapse_device and fetch_counted_device on another, which
    have to wait for it; rows past nmolecules stay untouched."""
    torch = pytest.importorskip("torch")
    nw, kind, L, hint, batches, snaps, _ = _case("family_3_10_37")
    index, umis = batches[0]
    rows = snaps[-1]["pairs"]
    n = len(rows)
    d_index, d_umi = torch.from_numpy(index).cuda(), torch.from_numpy(umis.view(np.int64)).cuda()
    out_i = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
    out_u, out_r, out_p = (torch.full((n + 2,), -9, dtype=torch.int64, device="cuda") for _ in range(3))
    d_collapsed = torch.full((nw + 1,), -5, dtype=torch.int64, device="cuda")
    one, two = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with _lib.tuning(count_preagg=preagg):
        with counting.MoleculeCounter(nw, L, encoding=ENC[kind], capacity_hint=hint, read_counts=True) as mc:
            mc.update_device(d_index.data_ptr(), d_umi.data_ptr(), index.size, stream=one.cuda_stream)
            mc.collapse_device(d_collapsed.data_ptr(), d_collapsed.data_ptr() + 8 * nw, stream=two.cuda_stream)
            mc.fetch_counted_device(out_i.data_ptr(), out_u.data_ptr(), out_r.data_ptr(), out_p.data_ptr(), n + 2,
                                    stream=two.cuda_stream)
            torch.cuda.synchronize()
            c = d_collapsed.cpu().tolist()
            assert (c[:nw], c[nw]) == snaps[-1]["collapse"]
            got = list(zip(out_i[:n].cpu().tolist(), out_u[:n].cpu().numpy().view(np.uint64).tolist(),
                           out_r[:n].cpu().tolist(), out_p[:n].cpu().numpy().view(np.uint64).tolist()))
            assert got == rows
            assert out_i[n:].cpu().tolist() == [-7] * 2
            assert all(t[n:].cpu().tolist() == [-9] * 2 for t in (out_u, out_r, out_p))
            # without n_corrected and without parents
            d_collapsed.fill_(-5)
            out_p.fill_(-9)
            mc.collapse_device(d_collapsed.data_ptr(), None, stream=one.cuda_stream)
            mc.fetch_counted_device(out_i.data_ptr(), out_u.data_ptr(), out_r.data_ptr(), None, n,
                                    stream=one.cuda_stream)
            torch.cuda.synchronize()
            assert d_collapsed.cpu().tolist() == snaps[-1]["collapse"][0] + [-5]
            assert out_r[:n].cpu().tolist() == [r[2] for r in rows] and out_p.cpu().tolist() == [-9] * (n + 2)
            _same(mc, snaps[-1], nw)


@pytest.mark.parametrize("preagg", PREAGG)
def test_a_counter_without_read_counts(preagg):
    """collapse() and pairs(reads=True) raise ValueError, the C calls are SCT_E_INVALID and change
    nothing, and its counts() / pairs() are the counted counter's on the same input."""
    nw, kind, L, hint, batches, snaps, _ = _case("family_3_5_3")
    snap = snaps[-1]
    with _lib.tuning(count_preagg=preagg):
        with counting.MoleculeCounter(nw, L, encoding=ENC[kind], capacity_hint=hint) as mc:
            mc.update(*batches[0])
            for call in (mc.collapse, lambda: mc.pairs(reads=True), lambda: mc.pairs(reads=True, parents=True),
                         lambda: mc.saturation(collapsed=True), lambda: mc.collapse_device(0),
                         lambda: mc.fetch_counted_device(0, 0, 0, 0, 0)):
                with pytest.raises(ValueError):
                    call()
            out = np.full(nw + 1, 77, dtype=np.uint64)
            assert mc._lib.sct_molecules_collapse_host(mc._h, _lib._ptr(out), _lib._ptr(out[nw:])) == _lib.SCT_E_INVALID
            assert "read counts" in _lib.last_error()
            assert mc._lib.sct_molecules_collapse(mc._h, None, None, None) == _lib.SCT_E_INVALID
            assert mc._lib.sct_molecules_fetch_counted_host(mc._h, None, None, None, None, 0) == _lib.SCT_E_INVALID
            assert mc._lib.sct_molecules_fetch_counted(mc._h, None, None, None, None, 0, None) == _lib.SCT_E_INVALID
            assert out.tolist() == [77] * (nw + 1)
            reads, molecules, n_none, n_amb, n_bad = mc.counts()
            assert (reads.tolist(), molecules.tolist(), n_none, n_amb, n_bad) == snap["counts"]
            index, umi = mc.pairs()
            assert list(zip(index.tolist(), umi.tolist())) == [r[:2] for r in snap["pairs"]]
            assert _same_float(mc.saturation(), snap["saturation"])
        with counting.MoleculeCounter(nw, L, encoding=ENC[kind], capacity_hint=hint, read_counts=True) as mc:
            with pytest.raises(ValueError):
                mc.pairs(parents=True)
            with pytest.raises(ValueError):
                mc.update(*batches[0]).pairs(reads=True, room=len(snap["pairs"]) - 1)
            assert "room" in _lib.last_error()
            _same(mc, snap, nw)
