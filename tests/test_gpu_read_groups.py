"""Read groups on the device (sctools_amd/csrc/molecules.hip, "read groups" in include/sctools_hip.h):
MoleculeCounter.read_groups and ReadGroups.tag against tests/read_groups_reference.py, the contract in
plain Python.  Every comparison is exact equality of integers.  The tag kernels can go wrong at the
64-lane wave, at the batch cut (the ordinals behind `first` run across calls), past one pass of the
grid and where a probe chain wraps round the table, so the shapes sit on those seams; tables start at
capacity_hint=64 unless a test says otherwise."""

import ctypes
import functools
import random

import numpy as np
import pytest

import feature_resolve_reference as F
import read_groups_cases as C
import read_groups_reference as G
import umi_directional_reference as D
from nearest_reference import mix64
from sctools_amd import _lib, counting

pytestmark = pytest.mark.gpu

ENC = {3: "ThreeBit", 2: "TwoBit"}


def arrays(index, umi, feature=None):
    out = (np.asarray(index, np.int32), np.asarray(umi, np.uint64))
    return out + ((np.asarray(feature, np.int32),) if feature is not None else ())


def feature_counter(fm, hint=64, reads=None):
    """A device counter fed the reads of a reference feature counter (key order unless given)."""
    mc = counting.MoleculeCounter(fm.nw, fm.L, ENC[fm.kind], capacity_hint=hint, read_counts=True, features=fm.nf)
    index, feature, umi = zip(*(reads if reads is not None else C.reads_of(fm.mreads)))
    idx, u, f = arrays(index, umi, feature)
    return mc.update(idx, u, features=f)


def plain_counter(cm, hint=64, read_counts=True):
    mc = counting.MoleculeCounter(cm.nw, cm.L, ENC[cm.kind], capacity_hint=hint, read_counts=read_counts)
    index, umi = zip(*C.reads_of(cm.mreads))
    return mc.update(*arrays(index, umi))


def tag(groups, batch):
    """groups.tag of a batch (index, feature or None, umi) as four lists; a column not asked for is None."""
    index, feature, umi = batch
    idx, u, *f = arrays(index, umi, feature)
    out = [col.tolist() for col in groups.tag(idx, u, features=f[0] if f else None)]
    reads = out.pop(2) if groups.reads else None
    first = out.pop(2) if groups.first else None
    return out[0], out[1], reads, first


def want_of(ref_groups, batch):
    index, feature, umi = batch
    return tuple(ref_groups.tag(index, umi, feature))


# ---- the cases worked by hand

@pytest.mark.parametrize("kind", [3, 2])
@pytest.mark.parametrize("name", ["worked", "kept_and_lost", "tied", "alone"])
def test_feature_cases_worked_by_hand(kind, name):
    nw, nf, mreads, batch, expected = C.feature_cases(kind)[name]
    fm = C.feature_reference(nw, nf, kind, 3, mreads)
    batch = tuple(list(col) for col in zip(*batch))
    with feature_counter(fm) as mc:
        for method in F.METHODS:
            for resolved in (False, True):
                want = C.columns(C.expected_of(expected, method, resolved))
                with mc.read_groups(method=method, resolved=resolved, reads=True, first=True) as groups:
                    assert tag(groups, batch) == want, (method, resolved)
                    assert groups.tagged == len(batch[0])


@pytest.mark.parametrize("kind", [3, 2])
def test_plain_case_worked_by_hand(kind):
    nw, mreads, batch, expected = C.plain_cases(kind)["worked"]
    cm = C.plain_reference(nw, kind, 3, mreads)
    index, umi = (list(col) for col in zip(*batch))
    with plain_counter(cm) as mc:
        for method in F.METHODS:
            with mc.read_groups(method=method, reads=True, first=True) as groups:
                assert tag(groups, (index, None, umi)) == C.columns(expected[method]), method
        with pytest.raises(ValueError):
            mc.read_groups(method="none", resolved=True)
    # a counter without read counts has the keys alone: 'none', no reads column
    with plain_counter(cm, read_counts=False) as mc:
        with counting.ReadGroups(mc, method="none", first=True) as groups:
            final, status, reads, first = tag(groups, (index, None, umi))
            want = C.columns(expected["none"])
            assert (final, status, first) == (want[0], want[1], want[3]) and reads is None
        for bad in (dict(method="one_step"), dict(method="directional"), dict(method="none", reads=True)):
            with pytest.raises(ValueError):
                mc.read_groups(**bad)


# ---- against the reference

@pytest.mark.parametrize("kind", [3, 2])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_mix_against_the_reference(seed, kind):
    fm, batch = C.mix_case(seed, kind)
    with feature_counter(fm) as mc:
        reads, molecules = mc.counts()[:2]
        for method in F.METHODS:
            collapsed = molecules.sum() if method == "none" else mc.collapse(method=method)[0].sum()
            resolved_per, _, _, _, reads_dropped = mc.resolve(method=method)
            for resolved in (False, True):
                C.assert_input_holds(fm, batch, method, resolved)
                ref = G.ReadGroups(fm, method, resolved)
                want = want_of(ref, batch)
                with mc.read_groups(method=method, resolved=resolved, reads=True, first=True) as groups:
                    got = tag(groups, batch)
                    assert got == want, (method, resolved)
                    assert groups.tally().tolist() == ref.tally and groups.tagged == ref.tagged == len(batch[0])
                _, status, mol_reads, first = got
                dropped = reads_dropped if resolved else 0
                assert sum(first) == (resolved_per.sum() if resolved else collapsed)
                assert status.count(G.LOST) == dropped
                assert sum(r for r, f in zip(mol_reads, first) if f) + dropped == reads.sum()


@pytest.mark.parametrize("kind", [3, 2])
def test_plain_mix_against_the_reference(kind):
    """A counter without features: the same reads with the feature dropped."""
    fm, (index, _, umi) = C.mix_case(0, kind)
    cm = D.DirectionalMolecules(fm.nw, kind, fm.L).update(*zip(*[(i, u) for i, _, u in C.reads_of(fm.mreads)]))
    with plain_counter(cm) as mc:
        for method in F.METHODS:
            ref = G.ReadGroups(cm, method)
            with mc.read_groups(method=method, reads=True, first=True) as groups:
                assert tag(groups, (index, None, umi)) == tuple(ref.tag(index, umi)), method
                assert groups.tally().tolist() == ref.tally
            with mc.read_groups(method=method) as groups:  # no optional column
                assert tag(groups, (index, None, umi)) == tuple(ref.last[:2]) + (None, None)


# ---- batch seams

@functools.lru_cache(maxsize=None)
def seam_case(at, then):
    """The mix batch of seed 1 with every read of one GROUPED molecule taken out and two of them put
    back at positions `at` and `then`: the molecule's two earliest reads."""
    fm, (index, feature, umi) = C.mix_case(1, 3)
    whole = list(zip(index, feature, umi))
    for key in sorted(k for k, r in fm.mreads.items() if r >= 2):
        reads = [r for r in whole if r != key]
        reads.insert(at, key)
        reads.insert(then, key)
        batch = tuple(list(col) for col in zip(*reads))
        want = want_of(G.ReadGroups(fm, "directional", True), batch)
        # (a key whose molecule is lost, or has an earlier read under another of its UMIs, is passed over)
        if want[3][at] and not want[3][then] and want[1][at] == want[1][then] == G.GROUPED:
            break
    else:
        raise AssertionError("no molecule of the input serves")
    return fm, batch, want


@pytest.fixture(scope="module")
def seam_counter():
    with feature_counter(C.mix_case(1, 3)[0]) as mc:
        yield mc


# the earliest two reads in lanes 10 and 20 of one wave; on either side of the cut of 64, 256 (and 1)
@pytest.mark.parametrize("at,then", [(10, 20), (63, 64), (255, 256)])
@pytest.mark.parametrize("size", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_batch_seams(seam_counter, at, then, size):
    """One batch (size 0) or batches of `size` with an empty batch between them: the concatenated
    outputs are the reference's, `first` included, which pins the ordinals across calls."""
    fm, batch, want = seam_case(at, then)
    n = len(batch[0])
    with seam_counter.read_groups(method="directional", resolved=True, reads=True, first=True) as groups:
        got = [[], [], [], []]
        for lo in range(0, n, size or n):
            piece = tuple(col[lo:lo + (size or n)] for col in batch)
            for k, col in enumerate(tag(groups, piece)):
                got[k] += col
            assert tag(groups, ([], [], [])) == ([], [], [], [])
        assert tuple(got) == want
        assert groups.tagged == n


def test_past_one_grid_pass():
    """The tag launch is at most 2048 workgroups of 256 lanes (open_table.h's grid_for cap), so a batch
    of 2048 * 256 + 65 reads sends the first 65 lanes round a second time: a few hundred molecules'
    reads repeated, against the reference."""
    fm, (index, feature, umi) = C.mix_case(2, 3)
    n = 2048 * 256 + 65
    reps = -(-n // 400)
    batch = tuple((col[:400] * reps)[:n] for col in (index, feature, umi))
    ref = G.ReadGroups(fm, "one_step", True)
    want = want_of(ref, batch)
    with feature_counter(fm) as mc, mc.read_groups(method="one_step", resolved=True, reads=True, first=True) as groups:
        idx, u, f = arrays(batch[0], batch[2], batch[1])
        final, status, reads, first = groups.tag(idx, u, features=f)
        assert final.tolist() == want[0] and status.tolist() == want[1]
        assert reads.tolist() == want[2] and first.tolist() == want[3]
        assert groups.tally().tolist() == ref.tally


# ---- host form and device form

def test_device_form_equals_host_form():
    import torch
    fm, batch = C.mix_case(3, 2)
    idx, u, f = arrays(batch[0], batch[2], batch[1])
    n = idx.size
    with feature_counter(fm) as mc:
        dev = torch.device("cuda", mc.device if mc.device is not None else torch.cuda.current_device())
        with mc.read_groups(method="directional", resolved=True, reads=True, first=True) as host_groups:
            want = host_groups.tag(idx, u, features=f)
        with mc.read_groups(method="directional", resolved=True, reads=True, first=True) as groups:
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                d_idx, d_f = torch.from_numpy(idx).to(dev), torch.from_numpy(f).to(dev)
                d_u = torch.from_numpy(u.view(np.int64)).to(dev)
                final = torch.empty(n, dtype=torch.int64, device=dev)
                reads = torch.empty(n, dtype=torch.int64, device=dev)
                status = torch.empty(n, dtype=torch.uint8, device=dev)
                first = torch.empty(n, dtype=torch.uint8, device=dev)
                half = n // 2  # two calls: the ordinals run on
                for lo, m in ((0, half), (half, n - half)):
                    groups.tag_device(d_idx[lo:].data_ptr(), d_u[lo:].data_ptr(), m, final[lo:].data_ptr(),
                                      status[lo:].data_ptr(), reads_ptr=reads[lo:].data_ptr(),
                                      first_ptr=first[lo:].data_ptr(), feature_ptr=d_f[lo:].data_ptr(),
                                      stream=stream.cuda_stream)
            stream.synchronize()
            assert final.cpu().numpy().view(np.uint64).tolist() == want[0].tolist()
            assert status.cpu().numpy().tolist() == want[1].tolist()
            assert reads.cpu().numpy().tolist() == want[2].tolist()
            assert first.cpu().numpy().astype(bool).tolist() == want[3].tolist()
            assert groups.tagged == n
            # a column the flags did not ask for, or one they asked for and did not get
            with mc.read_groups(method="none") as bare:
                with pytest.raises(ValueError):
                    bare.tag_device(d_idx.data_ptr(), d_u.data_ptr(), n, final.data_ptr(), status.data_ptr(),
                                    reads_ptr=reads.data_ptr(), feature_ptr=d_f.data_ptr())
            with pytest.raises(ValueError):
                groups.tag_device(d_idx.data_ptr(), d_u.data_ptr(), n, final.data_ptr(), status.data_ptr(),
                                  feature_ptr=d_f.data_ptr())


# ---- the snapshot

def test_snapshot_outlives_updates_growth_and_the_counter():
    fm, batch = C.mix_case(0, 3, nw=5, nf=6, L=6)
    before = want_of(G.ReadGroups(fm, "one_step", True), batch)
    mc = feature_counter(fm)
    old = mc.read_groups(method="one_step", resolved=True, reads=True, first=True)
    with mc.read_groups(method="one_step", resolved=True, reads=True, first=True) as groups:
        assert tag(groups, batch) == before
    # new molecules, enough to grow the table several times; some are neighbours of stored ones
    rng = random.Random(5)
    more = [(rng.randrange(fm.nw), rng.randrange(fm.nf), sum(rng.randrange(1, 5) << (3 * p) for p in range(6)))
            for _ in range(30000)]
    capacity = mc.info()["capacity"]
    index, feature, umi = zip(*more)
    idx, u, f = arrays(index, umi, feature)
    mc.update(idx, u, features=f)
    fm.update(index, umi, feature)
    assert mc.info()["capacity"] >= 4 * capacity
    after = want_of(G.ReadGroups(fm, "one_step", True), batch)
    assert after != before
    with mc.read_groups(method="one_step", resolved=True, reads=True, first=True) as groups:
        assert tag(groups, batch) == after
    mc.close()
    assert tag(old, batch) == before
    old.close()


# ---- a probe chain over the end of the table

def test_probe_chain_wraps():
    """Keys whose mix64 starts them in the last four slots of a 64-slot table: eight of them make
    chains that run over the end into slots 0, 1, ...  Stored keys and absent keys that hash into the
    chain are tagged."""
    kind, L, nw = 2, 10, 2
    landing = [u for u in range(1 << 14) if mix64(u) & 63 >= 60]  # index 0: the key is the UMI
    stored, absent = landing[:8], landing[8:16]
    cm = C.plain_reference(nw, kind, L, {(0, u): 1 + k % 3 for k, u in enumerate(stored)})
    with plain_counter(cm) as mc:
        assert mc.info()["capacity"] == 64
        index = [0] * 16
        umi = [u for pair in zip(stored, absent) for u in pair]
        for method in F.METHODS:
            ref = G.ReadGroups(cm, method)
            want = tuple(ref.tag(index, umi))
            assert set(want[1]) == {G.GROUPED, G.ABSENT}
            with mc.read_groups(method=method, reads=True, first=True) as groups:
                assert tag(groups, (index, None, umi)) == want, method


# ---- errors

def test_errors():
    nw, nf, mreads, batch, expected = C.feature_cases(3)["kept_and_lost"]
    fm = C.feature_reference(nw, nf, 3, 3, mreads)
    u = batch[0][2]
    with feature_counter(fm) as mc:
        with mc.read_groups(method="none", reads=True, first=True) as groups:
            with pytest.raises(ValueError):
                groups.tag(*arrays([nw, 1, 1], [u] * 3), features=np.array([0, nf, 0], np.int32))
            assert groups.tagged == 3
            assert groups.tally().tolist() == [1, 0, 0, 0, 0, 0, 0, 2]
            # the batch was tagged: its GROUPED read took the molecule's first
            assert tag(groups, ([1], [0], [u])) == ([u], [G.GROUPED], [5], [False])
            with pytest.raises(ValueError):
                groups.tag(*arrays([1, 1], [u]), features=np.array([0, 0], np.int32))
            with pytest.raises(ValueError):
                groups.tag(*arrays([1], [u]), features=np.array([0, 0], np.int32))
            with pytest.raises(ValueError):
                groups.tag(*arrays([1], [u]))
            assert groups.tagged == 4
        for bad in (dict(method="adjacency"), dict(method=None)):
            with pytest.raises(ValueError):
                mc.read_groups(**bad)
        lib, handle = _lib.lib(), counting._vp()
        assert lib.sct_read_groups_create(mc._h, 7, 0, ctypes.byref(handle), None) == _lib.SCT_E_INVALID
        assert lib.sct_read_groups_create(mc._h, 0, 8, ctypes.byref(handle), None) == _lib.SCT_E_INVALID
        assert "flags" in _lib.last_error()
    with counting.MoleculeCounter(nw, 3, "ThreeBit", capacity_hint=64, features=nf) as uncounted:
        for bad in (dict(method="one_step"), dict(method="none", resolved=True), dict(method="none", reads=True)):
            with pytest.raises(ValueError):
                uncounted.read_groups(**bad)
        lib, handle = _lib.lib(), counting._vp()
        for method, flags in ((0, 0), (1, 0), (2, 1), (2, 2)):
            assert lib.sct_read_groups_create(uncounted._h, method, flags, ctypes.byref(handle), None) == _lib.SCT_E_INVALID
            assert "read counts" in _lib.last_error()
    cm = C.plain_reference(1, 3, 3, {(0, u): 1})
    with plain_counter(cm) as mc, mc.read_groups(method="none") as groups:
        with pytest.raises(ValueError):
            groups.tag(*arrays([0], [u]), features=np.array([0], np.int32))
        lib, handle = _lib.lib(), counting._vp()
        assert lib.sct_read_groups_create(mc._h, 2, 1, ctypes.byref(handle), None) == _lib.SCT_E_INVALID
        assert "features" in _lib.last_error()


def test_an_empty_counter_gives_absent():
    u, bad = C.umi_of(3, 1, 2, 3), 6
    with counting.MoleculeCounter(3, 3, "ThreeBit", capacity_hint=64, read_counts=True, features=2) as mc:
        for method in F.METHODS:
            with mc.read_groups(method=method, resolved=True, reads=True, first=True) as groups:
                got = tag(groups, ([0, 2, -1, -2, 1, 1], [0, 1, 0, 0, -1, 0], [u, u, u, u, u, bad]))
                assert got == ([u, u, u, u, u, bad],
                               [G.ABSENT, G.ABSENT, G.NO_BARCODE, G.AMBIGUOUS, G.NO_FEATURE, G.BAD_UMI],
                               [0] * 6, [False] * 6)


def test_other_device():
    if _lib.device_count() < 2:
        pytest.skip("one device visible")
    import torch
    fm, batch = C.mix_case(0, 2)
    torch.cuda.set_device(0)
    mc = counting.MoleculeCounter(fm.nw, fm.L, ENC[fm.kind], capacity_hint=64, read_counts=True, features=fm.nf, device=1)
    index, feature, umi = zip(*C.reads_of(fm.mreads))
    idx, u, f = arrays(index, umi, feature)
    with mc.update(idx, u, features=f):
        with mc.read_groups(method="directional", resolved=True, reads=True, first=True) as groups:
            assert tag(groups, batch) == want_of(G.ReadGroups(fm, "directional", True), batch)
            assert groups.device == 1
        assert torch.cuda.current_device() == 0
