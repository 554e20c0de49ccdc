"""Directional UMI clusters on the device (sctools_amd/csrc/molecules.hip): a
MoleculeCounter(read_counts=True) with method='directional' against
tests/umi_directional_reference.py, the contract in plain Python.  Every comparison is exact equality
of integers and of order.  All shapes are a few thousand reads; a case's input and reference are
computed once and shared by the forms it runs under: the three pre-aggregation forms of the insert
(SCT_TUNE_COUNT_PREAGG) and the two forms of the sweeps (SCT_TUNE_DIRECTIONAL_FORM).  Every case
also shows that the one-step answers are what they were, before and after the directional calls."""

import ctypes
import functools
import math
import random

import numpy as np
import pytest

import count_matrix_reference as M
import umi_collapse_reference as U
import umi_directional_reference as D
from sctools_amd import _lib, counting

pytestmark = pytest.mark.gpu

PREAGG = [0, 1, 2]  # none, wave merge, LDS table
FORMS = [1, 0]  # sweeps over the worklist, sweeps over the whole table
ENC = {3: "ThreeBit", 2: "TwoBit"}
DIR = "directional"
C, A, G, T = 1, 2, 3, 4


def umi3(*bases):
    """A ThreeBit code written first base first (the first base in the high triplet)."""
    code = 0
    for b in bases:
        code = (code << 3) | b
    return code


def _snap(ref):
    """Everything the device counter is compared with, taken from the reference as it stands."""
    return {"counts": ref.counts(), "pairs": ref.pairs_counted(), "collapse": ref.collapse(),
            "dir_pairs": ref.pairs_directional(), "dir_collapse": ref.collapse_directional(),
            "dir_saturation": ref.saturation_directional()}


def _same_float(a, b):
    return type(a) is float and (a == b or (math.isnan(a) and math.isnan(b)))


def _one_step_same(mc, snap):
    collapsed, n_corrected = mc.collapse()
    assert (collapsed.tolist(), n_corrected) == snap["collapse"]
    reads, molecules, n_none, n_amb, n_bad = mc.counts()
    assert (reads.tolist(), molecules.tolist(), n_none, n_amb, n_bad) == snap["counts"]
    assert list(zip(*(a.tolist() for a in mc.pairs(reads=True, parents=True)))) == snap["pairs"]


def _same(mc, snap, nw):
    """collapse, pairs and saturation with method='directional' = the reference's, twice; the one-step
    answers and counts() are the reference's before and after."""
    _one_step_same(mc, snap)
    for _ in range(2):  # it reads only: the same answer again
        collapsed, n_corrected = mc.collapse(method=DIR)
        assert collapsed.dtype == np.int64 and collapsed.shape == (nw,) and type(n_corrected) is int
        assert (collapsed.tolist(), n_corrected) == snap["dir_collapse"]
        four = mc.pairs(reads=True, parents=True, method=DIR)
        assert [a.dtype for a in four] == [np.int32, np.uint64, np.int64, np.uint64]
        assert list(zip(*(a.tolist() for a in four))) == snap["dir_pairs"]
        assert _same_float(mc.saturation(collapsed=True, method=DIR), snap["dir_saturation"])
    # the method changes the parent column only
    assert list(zip(*(a.tolist() for a in mc.pairs(reads=True, method=DIR)))) == [r[:3] for r in snap["pairs"]]
    assert list(zip(*(a.tolist() for a in mc.pairs(method=DIR)))) == [r[:2] for r in snap["pairs"]]
    _one_step_same(mc, snap)
    return mc.info()


def _arrays(reads):
    return (np.array([r[0] for r in reads], dtype=np.int32), np.array([r[1] for r in reads], dtype=np.uint64))


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


def _hub(L, barcodes, hub_reads, spoke_reads):
    """Under every barcode: one hub with hub_reads reads and its 3 * L neighbours with spoke_reads each."""
    hub = sum(((p % 4) + 1) << (3 * p) for p in range(L))
    reads = []
    for b in barcodes:
        reads += [(b, hub)] * hub_reads + [(b, v) for v in U.neighbours(hub, 3, L)] * spoke_reads
    return reads


FAMILIES = {"family_3_5_3": (3, 5, 3, 300, 101), "family_2_4_2": (2, 4, 2, 200, 102),
            "family_3_10_37": (3, 10, 37, 2000, 103)}
V, P1, P2, GG = umi3(A, A, A), umi3(A, A, C), umi3(A, C, A), umi3(G, C, A)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(nw, kind, L, capacity_hint, batches, snapshot after every batch) of a named case."""
    hint, shuffle = 64, True
    rng = np.random.default_rng(len(name))
    if name == "empty":
        nw, kind, L, reads = 3, 3, 2, []
    elif name == "chain":
        nw, kind, L = 1, 3, 2
        reads = [(0, umi3(A, A))] + [(0, umi3(A, C))] * 2 + [(0, umi3(G, C))] * 5
    elif name == "threshold":  # 3 over 2 (barcode 0), 2 and 2 (1), 4 and 4 (2), 5 over 3 over 2 (3), 4 and 3 (4)
        nw, kind, L = 5, 3, 2
        reads = [(0, umi3(A, C))] * 3 + [(0, umi3(A, G))] * 2 + [(1, umi3(A, C))] * 2 + [(1, umi3(A, G))] * 2
        reads += [(2, umi3(A, C))] * 4 + [(2, umi3(A, G))] * 4
        reads += [(3, umi3(A, C))] * 5 + [(3, umi3(A, G))] * 3 + [(3, umi3(T, G))] * 2
        reads += [(4, umi3(A, C))] * 4 + [(4, umi3(A, G))] * 3
    elif name == "ancestor":  # v x 1 beside p1 x 10 and p2 x 8; g x 100 beside p2 only
        nw, kind, L = 1, 3, 3
        reads = [(0, V)] + [(0, P1)] * 10 + [(0, P2)] * 8 + [(0, GG)] * 100
    elif name == "mutual":  # three 1-read UMIs pairwise one base apart; under barcode 1 a fourth, two bases off
        nw, kind, L = 2, 3, 2
        reads = [(0, umi3(A, C)), (0, umi3(A, A)), (0, umi3(A, T))]
        reads += [(1, umi3(A, C)), (1, umi3(A, A)), (1, umi3(A, T)), (1, umi3(G, G))]
    elif name == "path":  # 100 one-read UMIs in a line under two barcodes, fed in ascending code order
        nw, kind, L, shuffle = 3, 3, 10, False
        line = sorted(D.snake(3, L, 100, random.Random(22)))
        reads = [(0, u) for u in line] + [(2, u) for u in line]
    elif name == "length_one":
        nw, kind, L = 2, 3, 1
        reads = [(1, C)] * 2 + [(1, A)] * 7 + [(1, G)] * 7 + [(1, T)] + [(0, C), (0, T)]
    elif name == "length_one_twobit":
        nw, kind, L = 2, 2, 1
        reads = [(0, 0), (0, 3), (1, 0), (1, 0), (1, 3), (1, 3), (1, 2)]
    elif name == "star50":
        nw, kind, L = 64, 3, 10
        reads = _hub(L, range(7, 57), 3, 1)
    elif name == "hubs":  # spokes of 2 reads under a hub of 3 (joined, barcode 0) and of 2 (not joined, 1)
        nw, kind, L = 2, 3, 10
        reads = _hub(L, [0], 3, 2) + _hub(L, [1], 2, 2)
    elif name == "corner63":  # TwoBit, 15 + 48 = 63 key bits: the top key, all its 72 UMI neighbours, and
        nw, kind, L = 2 ** 15, 2, 24  # the same UMIs under the index one bit away, which are unrelated
        top = 2 ** 48 - 1
        nbs = U.neighbours(top, 2, L)
        reads = [(32767, top)] * 5 + [(32767, v) for v in nbs] + [(32767, nbs[71])] * 9
        reads += [(32766, top)] + [(32766, v) for v in nbs[:9]] * 2 + [(32766, nbs[70])] * 3
        reads += [(0, 0), (0, 1), (0, 1), (16383, top)]
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
    elif name in FAMILIES:
        kind, L, nw, nroots, seed = FAMILIES[name]
        index, umis = _mutated_family(kind, L, nw, nroots, seed)
        hint = 1 << 14 if nroots >= 2000 else 64
    else:
        raise KeyError(name)
    if name != "growth" and name not in FAMILIES:
        index, umis = _arrays([reads[i] for i in (rng.permutation(len(reads)) if shuffle else range(len(reads)))])
    n = index.size
    cuts = [0, n // 3, 2 * n // 3, n] if name == "growth" else [0, n]
    batches = [(index[a:b], umis[a:b]) for a, b in zip(cuts, cuts[1:])]
    ref = D.DirectionalMolecules(nw, kind, L)
    snaps = [_snap(ref.update(*batch)) for batch in batches]
    return nw, kind, L, hint, batches, snaps


def _run_case(name, preagg=1, form=1, check=None):
    nw, kind, L, hint, batches, snaps = _case(name)
    with _lib.tuning(count_preagg=preagg, directional_form=form):
        with counting.MoleculeCounter(nw, L, encoding=ENC[kind], capacity_hint=hint, read_counts=True) as mc:
            for batch, snap in zip(batches, snaps):
                mc.update(*batch)
                info = _same(mc, snap, nw)
            if check:
                check(mc)
    return snaps[-1], info


def _root_of(snap, index, umi):
    return [r[3] for r in snap["dir_pairs"] if r[:2] == (index, umi)][0]


def _last_pass(mc):
    sweeps, listed, swept = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    _lib.check(mc._lib.sct_molecules_directional_info(mc._h, ctypes.byref(sweeps), ctypes.byref(listed),
                                                      ctypes.byref(swept)))
    assert listed.value <= swept.value <= sweeps.value * max(listed.value, 1)
    return sweeps.value, listed.value


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("preagg", PREAGG)
def test_hand_cases(preagg, form):
    """The header's chain (1 cluster where one step gives 2 images), the threshold (3 over 2 joined;
    2 and 2, 4 and 4, 4 and 3 not), three mutually joined 1-read UMIs named by the largest code, L = 1
    in both encodings, and a counter that was fed nothing."""
    assert _lib.tune_get("directional_form") == -1  # the default is the worklist form
    snap, _ = _run_case("chain", preagg, form)
    assert snap["dir_collapse"] == ([1], 2) and snap["collapse"] == ([2], 2)
    assert [r[3] for r in snap["dir_pairs"]] == [umi3(G, C)] * 3
    snap, _ = _run_case("threshold", preagg, form)
    assert snap["dir_collapse"] == ([1, 2, 2, 1, 2], 3) and snap["collapse"][0] == [1, 1, 1, 2, 1]
    snap, _ = _run_case("mutual", preagg, form)
    assert snap["dir_collapse"] == ([1, 2], 4) and _root_of(snap, 0, umi3(A, A)) == umi3(A, T)
    assert _run_case("length_one", preagg, form)[0]["dir_collapse"] == ([1, 2], 3)
    assert _run_case("length_one_twobit", preagg, form)[0]["dir_collapse"] == ([1, 2], 2)
    snap, _ = _run_case("empty", preagg, form)
    assert snap["dir_collapse"] == ([0, 0, 0], 0) and math.isnan(snap["dir_saturation"])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("preagg", PREAGG)
def test_best_ancestor_through_the_lesser_parent(preagg, form):
    """v's best parent is p1 x 10, but its root is g x 100, which reaches it through p2 x 8 only: a
    kernel that follows the best parent alone answers p1."""
    snap, _ = _run_case("ancestor", preagg, form)
    assert _root_of(snap, 0, V) == GG and _root_of(snap, 0, P2) == GG and _root_of(snap, 0, P1) == P1
    assert [r[3] for r in snap["pairs"] if r[1] == V] == [P1]
    assert snap["dir_collapse"] == ([2], 2)


@pytest.mark.parametrize("form", FORMS)
def test_a_long_path(form):
    """100 one-read UMIs, each one base from the next and from no other, under barcodes 0 and 2: one
    cluster each, named by the line's largest code, which the far end learns only step by step."""
    def check(mc):
        mc.collapse(method=DIR)
        sweeps, listed = _last_pass(mc)
        assert 2 <= sweeps <= 202 and listed == 200
    snap, info = _run_case("path", 1, form, check)
    top = max(r[1] for r in snap["dir_pairs"])
    assert snap["dir_collapse"] == ([1, 0, 1], 198) and info["nmolecules"] == 200
    assert {r[3] for r in snap["dir_pairs"]} == {top}
    assert D.fixpoint_roots({(r[0], r[1]): r[2] for r in snap["dir_pairs"]}, 3, 10)[1] >= 50


@pytest.mark.parametrize("preagg", PREAGG)
def test_hubs(preagg):
    """A hub of 3 reads and its 30 one-read neighbours under 50 barcodes; then spokes of 2 reads under
    a hub of 3 (3 >= 2 * 2 - 1: one cluster) and under a hub of 2 (31 clusters: equal reads >= 2 join
    nothing, neither hub and spoke nor two spokes of one position)."""
    snap, info = _run_case("star50", preagg)
    want = [1 if 7 <= b < 57 else 0 for b in range(64)]
    assert snap["dir_collapse"] == (want, 30 * 50) and info["nmolecules"] == 31 * 50
    snap, _ = _run_case("hubs", preagg)
    assert snap["dir_collapse"] == ([1, 31], 30) and snap["collapse"][0][0] == 1 and snap["collapse"][0][1] < 31


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("preagg", PREAGG)
def test_the_63_bit_corner(preagg, form):
    """Key 2^63 - 1 with all 72 UMI neighbours present, more than a wave has lanes: the last of them
    has 10 reads and is the root of them all.  The same UMIs under index 32766 stay apart."""
    snap, _ = _run_case("corner63", preagg, form)
    top, nbs = 2 ** 48 - 1, U.neighbours(2 ** 48 - 1, 2, 24)
    collapsed, _ = snap["dir_collapse"]
    assert snap["counts"][1][32767] == 73 and collapsed[32767] == 1
    assert all(r[3] == nbs[71] for r in snap["dir_pairs"] if r[0] == 32767)
    # under 32766: top x 1, nine neighbours x 2 and nbs[70] x 3 -- 3 over 1, 2 over 1, not 3 over 2
    assert _root_of(snap, 32766, top) == nbs[70] and _root_of(snap, 32766, nbs[0]) == nbs[0]
    assert collapsed[0] == 1 and collapsed[16383] == 1


@pytest.mark.parametrize("preagg", PREAGG)
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_mutated_families(name, preagg):
    """Random roots with geometric reads and 4 % substitutions per base.  The input is first shown, on
    the reference alone, to need the transitive part (more than one round) and to give fewer clusters
    than the one-step rule gives images."""
    nw, kind, L, _, _, snaps = _case(name)
    mreads = {(r[0], r[1]): r[2] for r in snaps[-1]["dir_pairs"]}
    assert D.fixpoint_roots(mreads, kind, L)[1] >= 2
    assert sum(snaps[-1]["dir_collapse"][0]) < sum(snaps[-1]["collapse"][0])
    assert any(r[3] != s[3] for r, s in zip(snaps[-1]["dir_pairs"], snaps[-1]["pairs"]))
    _run_case(name, preagg)


@pytest.mark.parametrize("name", sorted(FAMILIES) + ["growth", "bad_mixed"])
def test_sweeps_over_the_whole_table_give_the_same(name):
    """SCT_TUNE_DIRECTIONAL_FORM 0, no worklist, against the reference: every number as before."""
    _run_case(name, 1, 0)


@pytest.mark.parametrize("preagg", PREAGG)
def test_forced_growth(preagg):
    """capacity_hint=64 and about 3,000 molecules in three batches, everything compared after every
    batch: the labels are made for the table as it stands, whatever its capacity."""
    _, info = _run_case("growth", preagg)
    assert 2500 <= info["nmolecules"] <= 3500 and info["capacity"] >= 64 * 2 ** 4


@pytest.mark.parametrize("preagg", PREAGG)
def test_bad_umis_and_missing_barcodes_are_nobodys_neighbour(preagg):
    snap, _ = _run_case("bad_mixed", preagg)
    assert snap["dir_pairs"] == [(2, int("1231", 8), 1, int("1234", 8)), (2, int("1234", 8), 3, int("1234", 8)),
                                 (4, int("4443", 8), 2, int("4443", 8)), (4, int("4444", 8), 1, int("4443", 8))]
    assert snap["dir_collapse"] == ([0, 0, 1, 0, 1], 2)


@pytest.mark.parametrize("form", FORMS)
def test_two_streams(form):
    """update_device on one stream, then collapse_device and fetch_counted_device with
    method='directional' on another, which have to wait for it; rows past nmolecules stay untouched."""
    torch = pytest.importorskip("torch")
    nw, kind, L, hint, batches, snaps = _case("family_3_10_37")
    index, umis = batches[0]
    rows = snaps[-1]["dir_pairs"]
    n = len(rows)
    d_index, d_umi = torch.from_numpy(index).cuda(), torch.from_numpy(umis.view(np.int64)).cuda()
    out_i = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
    out_u, out_r, out_p = (torch.full((n + 2,), -9, dtype=torch.int64, device="cuda") for _ in range(3))
    d_collapsed = torch.full((nw + 2,), -5, dtype=torch.int64, device="cuda")
    one, two = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with _lib.tuning(directional_form=form):
        with counting.MoleculeCounter(nw, L, encoding=ENC[kind], capacity_hint=hint, read_counts=True) as mc:
            mc.update_device(d_index.data_ptr(), d_umi.data_ptr(), index.size, stream=one.cuda_stream)
            mc.collapse_device(d_collapsed.data_ptr(), d_collapsed.data_ptr() + 8 * nw, stream=two.cuda_stream,
                               method=DIR)
            mc.fetch_counted_device(out_i.data_ptr(), out_u.data_ptr(), out_r.data_ptr(), out_p.data_ptr(), n + 2,
                                    stream=two.cuda_stream, method=DIR)
            torch.cuda.synchronize()
            c = d_collapsed.cpu().tolist()
            assert (c[:nw], c[nw]) == snaps[-1]["dir_collapse"] and c[nw + 1] == -5
            got = list(zip(out_i[:n].cpu().tolist(), out_u[:n].cpu().numpy().view(np.uint64).tolist(),
                           out_r[:n].cpu().tolist(), out_p[:n].cpu().numpy().view(np.uint64).tolist()))
            assert got == rows
            assert out_i[n:].cpu().tolist() == [-7] * 2
            assert all(t[n:].cpu().tolist() == [-9] * 2 for t in (out_u, out_r, out_p))
            # without n_corrected and without parents
            d_collapsed.fill_(-5)
            out_p.fill_(-9)
            mc.collapse_device(d_collapsed.data_ptr(), None, stream=one.cuda_stream, method=DIR)
            mc.fetch_counted_device(out_i.data_ptr(), out_u.data_ptr(), out_r.data_ptr(), None, n,
                                    stream=one.cuda_stream, method=DIR)
            torch.cuda.synchronize()
            assert d_collapsed.cpu().tolist() == snaps[-1]["dir_collapse"][0] + [-5, -5]
            assert out_r[:n].cpu().tolist() == [r[2] for r in rows] and out_p.cpu().tolist() == [-9] * (n + 2)
            _same(mc, snaps[-1], nw)


@functools.lru_cache(maxsize=None)
def _feature_case():
    """The header's chain under features 1 and 4 of cell 2, a mutated family spread over 5 features, and
    reads without a feature."""
    nw, nf, kind, L = 6, 5, 3, 5
    index, umis = _mutated_family(kind, L, nw, 300, 104)
    feature = np.random.default_rng(105).integers(-2, nf, size=index.size).astype(np.int32)
    aa, ac, gc = umi3(C, C, C, A, A), umi3(C, C, C, A, C), umi3(C, C, C, G, C)
    chain = [aa] + [ac] * 2 + [gc] * 5
    index = np.concatenate([index, np.full(16, 2, np.int32)])
    umis = np.concatenate([umis, np.array(chain * 2, np.uint64)])
    feature = np.concatenate([feature, np.array([1] * 8 + [4] * 8, np.int32)])
    ref = M.FeatureMolecules(nw, nf, kind, L).update(index, umis, feature)
    return nw, nf, kind, L, (index, umis, feature), ref, D.feature_answers(ref), (aa, ac, gc)


@pytest.mark.parametrize("form", FORMS)
def test_features(form):
    """The same UMI chain under two features of one cell is two clusters; matrix(collapsed=True) is
    the reference's per entry and its row sums are collapse()'s; the one-step matrix is unchanged."""
    nw, nf, kind, L, (index, umis, feature), ref, (collapsed, n_corrected, rows, per_entry), (aa, ac, gc) = _feature_case()
    assert [r for r in rows if r[0] == 2 and r[2] in (aa, ac)] == [(2, 1, ac, 2, gc), (2, 1, aa, 1, gc),
                                                                    (2, 4, ac, 2, gc), (2, 4, aa, 1, gc)]
    assert per_entry != ref.matrix()[4] and sum(per_entry) == sum(collapsed)
    with _lib.tuning(directional_form=form):
        with counting.MoleculeCounter(nw, L, capacity_hint=64, read_counts=True, features=nf) as mc:
            mc.update(index, umis, features=feature)
            one_step = [a.tolist() for a in mc.matrix(reads=True, collapsed=True)]
            assert one_step == [list(x) for x in ref.matrix()]
            for _ in range(2):
                got = [a.tolist() for a in mc.matrix(reads=True, collapsed=True, method=DIR)]
                assert got[:4] == one_step[:4] and got[4] == per_entry
                c = mc.collapse(method=DIR)
                assert (c[0].tolist(), c[1]) == (collapsed, n_corrected)
                indptr = got[0]
                assert [sum(got[4][a:b]) for a, b in zip(indptr, indptr[1:])] == collapsed
                five = mc.pairs(features=True, reads=True, parents=True, method=DIR)
                assert list(zip(*(a.tolist() for a in five))) == rows
            assert [a.tolist() for a in mc.matrix(collapsed=True, method=DIR)] == got[:3] + [per_entry]
            assert [a.tolist() for a in mc.matrix(reads=True, collapsed=True)] == one_step
            assert list(zip(*(a.tolist() for a in mc.pairs(features=True, reads=True, parents=True)))) == ref.pairs()


def test_matrix_device_form():
    torch = pytest.importorskip("torch")
    nw, nf, kind, L, (index, umis, feature), ref, (collapsed, _, rows, per_entry), _ = _feature_case()
    nnz = len(per_entry)
    d_indptr = torch.full((nw + 1,), -1, dtype=torch.int64, device="cuda")
    d_feature = torch.full((nnz + 1,), -7, dtype=torch.int32, device="cuda")
    d_collapsed = torch.full((nnz + 1,), -9, dtype=torch.int64, device="cuda")
    with counting.MoleculeCounter(nw, L, capacity_hint=64, read_counts=True, features=nf) as mc:
        mc.update(index, umis, features=feature)
        assert mc.matrix_device(d_indptr.data_ptr(), d_feature.data_ptr(), None, None, d_collapsed.data_ptr(), nnz,
                                method=DIR) == nnz
        torch.cuda.synchronize()
        assert d_collapsed.cpu().tolist() == per_entry + [-9] and d_indptr.cpu().tolist() == ref.matrix()[0]
        assert d_feature.cpu().tolist() == ref.matrix()[1] + [-7]


@pytest.mark.parametrize("rows_route", [0, 1])
def test_merge(rows_route):
    """Two counters fed alternate reads of a family: after a.merge(b) every directional answer is the
    single counter's (a molecule's reads are split between the two, so neither alone has the edges)."""
    nw, kind, L, hint, batches, snaps = _case("family_3_5_3")
    index, umis = batches[0]
    with _lib.tuning(merge_rows=rows_route):
        with counting.MoleculeCounter(nw, L, encoding=ENC[kind], capacity_hint=64, read_counts=True) as a, \
                counting.MoleculeCounter(nw, L, encoding=ENC[kind], capacity_hint=64, read_counts=True) as b:
            a.update(index[0::2], umis[0::2])
            b.update(index[1::2], umis[1::2])
            alone = a.collapse(method=DIR)
            assert (alone[0].tolist(), alone[1]) != snaps[-1]["dir_collapse"]
            a.merge(b)
            _same(a, snaps[-1], nw)


def _c_collapse(mc, name, *method):
    out = np.full(mc.size + 1, 77, dtype=np.uint64)
    rc = getattr(mc._lib, name)(mc._h, *method, _lib._ptr(out), _lib._ptr(out[mc.size:]))
    return rc, out.tolist()


def _c_fetch(mc, name, n, *method, feature=False):
    cols = [np.full(n, 7, np.int32)] + ([np.full(n, 7, np.int32)] if feature else [])
    cols += [np.full(n, 7, np.uint64) for _ in range(3)]
    rc = getattr(mc._lib, name)(mc._h, *method, *(_lib._ptr(c) for c in cols), n)
    return rc, [c.tolist() for c in cols]


def _c_matrix(mc, name, n, *method):
    cols = [np.full(mc.size + 1, 7, np.int64), np.full(n, 7, np.int32)] + [np.full(n, 7, np.uint64) for _ in range(3)]
    nnz = ctypes.c_int64(-1)
    rc = getattr(mc._lib, name)(mc._h, *method, *(_lib._ptr(c) for c in cols), n, ctypes.byref(nnz))
    return rc, nnz.value, [c.tolist() for c in cols]


def test_method_0_is_the_old_entry_point_and_method_7_is_invalid():
    """Every _by_host form with SCT_COLLAPSE_ONE_STEP writes what its sibling writes; method 7 is
    SCT_E_INVALID, names the method and writes nothing.  The device forms likewise."""
    torch = pytest.importorskip("torch")
    nw, nf, kind, L, (index, umis, feature), ref, _, _ = _feature_case()
    with counting.MoleculeCounter(nw, L, capacity_hint=64, read_counts=True, features=nf) as mc:
        mc.update(index, umis, features=feature)
        n = len(mc)
        old = _c_collapse(mc, "sct_molecules_collapse_host")
        assert old[0] == _lib.SCT_OK and old == _c_collapse(mc, "sct_molecules_collapse_by_host", 0)
        assert _c_collapse(mc, "sct_molecules_collapse_by_host", 1)[1] != old[1]
        assert _c_collapse(mc, "sct_molecules_collapse_by_host", 7) == (_lib.SCT_E_INVALID, [77] * (nw + 1))
        assert "method 7" in _lib.last_error()
        old = _c_fetch(mc, "sct_molecules_fetch_counted_host", n)
        assert old[0] == _lib.SCT_OK and old == _c_fetch(mc, "sct_molecules_fetch_counted_by_host", n, 0)
        assert _c_fetch(mc, "sct_molecules_fetch_counted_by_host", n, 7) == (_lib.SCT_E_INVALID, [[7] * n] * 4)
        old = _c_fetch(mc, "sct_molecules_fetch_features_host", n, feature=True)
        assert old[0] == _lib.SCT_OK and old == _c_fetch(mc, "sct_molecules_fetch_features_by_host", n, 0, feature=True)
        assert _c_fetch(mc, "sct_molecules_fetch_features_by_host", n, -1, feature=True)[0] == _lib.SCT_E_INVALID
        old = _c_matrix(mc, "sct_molecules_matrix_host", n)
        assert old[0] == _lib.SCT_OK and old == _c_matrix(mc, "sct_molecules_matrix_by_host", n, 0)
        bad = _c_matrix(mc, "sct_molecules_matrix_by_host", n, 7)
        assert bad[:2] == (_lib.SCT_E_INVALID, -1) and bad[2][1:] == [[7] * n] * 4
        # the device forms, into torch arrays: `before` is the method, or nothing for the old entry point
        def dev(name, shapes, before, after):
            outs = [torch.full((s,), 7, dtype=t, device="cuda") for s, t in shapes]
            rc = getattr(mc._lib, name)(mc._h, *before, *(ctypes.c_void_p(o.data_ptr()) for o in outs), *after)
            torch.cuda.synchronize()
            return rc, [o.cpu().tolist() for o in outs]
        i64, i32 = torch.int64, torch.int32
        nnz = ctypes.c_int64(-1)
        for name, shapes, after in (
                ("sct_molecules_collapse", [(nw, i64), (1, i64)], (None,)),
                ("sct_molecules_fetch_counted", [(n, i32)] + [(n, i64)] * 3, (n, None)),
                ("sct_molecules_fetch_features", [(n, i32)] * 2 + [(n, i64)] * 3, (n, None)),
                ("sct_molecules_matrix", [(nw + 1, i64), (n, i32)] + [(n, i64)] * 3, (n, ctypes.byref(nnz), None))):
            old = dev(name, shapes, (), after)
            assert old[0] == _lib.SCT_OK and old == dev(name + "_by", shapes, (0,), after)
            rc, untouched = dev(name + "_by", shapes, (7,), after)
            assert rc == _lib.SCT_E_INVALID and all(set(u) == {7} for u in untouched)
        assert nnz.value == len(ref.matrix()[1])
        with pytest.raises(ValueError):
            mc.collapse(method="adjacency")
        for call in (mc.collapse, mc.pairs, mc.matrix, mc.saturation,
                     lambda method: mc.collapse_device(0, method=method),
                     lambda method: mc.fetch_counted_device(0, 0, 0, 0, 0, method=method),
                     lambda method: mc.matrix_device(0, 0, 0, 0, 0, 0, method=method)):
            with pytest.raises(ValueError, match="one_step"):
                call(method="cluster")
        assert [a.tolist() for a in mc.matrix(reads=True, collapsed=True)] == [list(x) for x in ref.matrix()]


@pytest.mark.parametrize("preagg", PREAGG)
def test_a_counter_without_read_counts(preagg):
    """method='directional' on a counter that keeps no read counts raises as collapse does, the C calls
    are SCT_E_INVALID, and nothing changes."""
    nw, kind, L, hint, batches, snaps = _case("family_3_5_3")
    snap = snaps[-1]
    with _lib.tuning(count_preagg=preagg):
        with counting.MoleculeCounter(nw, L, encoding=ENC[kind], capacity_hint=hint) as mc:
            mc.update(*batches[0])
            for call in (lambda: mc.collapse(method=DIR), lambda: mc.pairs(reads=True, parents=True, method=DIR),
                         lambda: mc.saturation(collapsed=True, method=DIR), lambda: mc.collapse_device(0, method=DIR),
                         lambda: mc.fetch_counted_device(0, 0, 0, 0, 0, method=DIR)):
                with pytest.raises(ValueError):
                    call()
            assert _c_collapse(mc, "sct_molecules_collapse_by_host", 1) == (_lib.SCT_E_INVALID, [77] * (nw + 1))
            assert "read counts" in _lib.last_error()
            assert mc._lib.sct_molecules_collapse_by(mc._h, 1, None, None, None) == _lib.SCT_E_INVALID
            assert mc._lib.sct_molecules_fetch_counted_by_host(mc._h, 1, None, None, None, None, 0) == _lib.SCT_E_INVALID
            assert mc._lib.sct_molecules_fetch_counted_by(mc._h, 1, None, None, None, None, 0, None) == _lib.SCT_E_INVALID
            reads, molecules, n_none, n_amb, n_bad = mc.counts()
            assert (reads.tolist(), molecules.tolist(), n_none, n_amb, n_bad) == snap["counts"]
            index, umi = mc.pairs(method=DIR)
            assert list(zip(index.tolist(), umi.tolist())) == [r[:2] for r in snap["pairs"]]
