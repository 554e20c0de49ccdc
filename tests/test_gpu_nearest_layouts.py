"""The open-addressing and CSR nearest indexes (sctools_amd/csrc/nearest.hip) against the brute
force of the contract (oracle.c_nearest), exact equality on every query: every width of 1..64 bits,
open-addressing chains that fill a group, run on and wrap, CSR buckets that hold the whole
whitelist, launch seams, whitelists that are not A/C/G/T, and the user-facing forms past 16 bases.
The inputs come from tests/nearest_reference.py, whose claims tests/test_nearest_reference_host.py
checks on the CPU; the plan's scheme and index_bytes are compared with the mirror's, so a change of
layout fails here instead of un-aiming the inputs."""

import numpy as np
import pytest

import nearest_reference as R
from oracle import oracle as O
from sctools_amd import _lib, barcode

pytestmark = pytest.mark.gpu

_SCHEMES = {"auto": _lib.NEAREST_AUTO, "oa": _lib.NEAREST_OA, "csr": _lib.NEAREST_CSR}


def _plan_answers(kind, wl, q, code_bits, max_d, scheme, load=None):
    """(index, dist, info) of a device plan built under the forced scheme."""
    import torch
    d_wl = torch.from_numpy(wl.view(np.int64)).cuda()
    d_q = torch.from_numpy(q.view(np.int64)).cuda()
    out_i = torch.empty(q.size, dtype=torch.int32, device="cuda")
    out_d = torch.empty(q.size, dtype=torch.uint8, device="cuda")
    with _lib.tuning(nearest_scheme=_SCHEMES[scheme], nearest_load=load):
        plan = _lib.NearestPlan(kind, d_wl.data_ptr(), wl.size, code_bits, max_d)
    try:
        info = plan.info()
        plan.query(d_q.data_ptr(), q.size, out_i.data_ptr(), out_d.data_ptr())
        torch.cuda.synchronize()
    finally:
        plan.close()
    return out_i.cpu().numpy(), out_d.cpu().numpy(), info


def _check_info(info, scheme, kind, code_bits, max_d, wl, load=4):
    """The plan's layout is the one the mirror describes."""
    G = R.positions(kind, code_bits)
    if scheme == "auto":
        if G > 16 or max_d >= 2:
            assert info["scheme"] != "halves"
        elif 2 <= G:
            assert info["scheme"] == "halves"  # (A/C/G/T whitelists only reach here)
        if info["scheme"] == "halves":
            assert info["index_bytes"] == R.halves_index_bytes(kind, code_bits, wl.size)
            return
        want = info["scheme"]
    else:
        want = R.expected_scheme(scheme, kind, code_bits, max_d, wl.size)
        assert info["scheme"] == want, (scheme, kind, code_bits, max_d)
    if want == "oa":
        assert info["index_bytes"] == R.oa_layout(kind, code_bits, max_d, wl.size)["index_bytes"]
    else:
        assert info["index_bytes"] == R.csr_layout(kind, code_bits, max_d, wl.size, load, wl)["index_bytes"]


def _same(got_i, got_d, ref):
    assert np.array_equal(got_i, ref[0]) and np.array_equal(got_d, ref[1])


# ---------------------------------------------------------------- 1. every width
@pytest.mark.parametrize("scheme", ["auto", "oa", "csr"])
@pytest.mark.parametrize("kind", [2, 3])
def test_every_width(kind, scheme):
    """Lengths 1..32 (TwoBit) / 1..21 (ThreeBit) through barcode.nearest_whitelist and a plan of the
    same code_bits, and widths that are no multiple of the code width through the plan alone, at
    max_d 0..min(3, G - 1)."""
    lengths = range(1, 33) if kind == 2 else range(1, 22)
    cells = [(kind * L, True) for L in lengths]
    cells += [(b, False) for b in ((31, 63) if kind == 2 else (46, 47, 62, 63, 64))]
    for code_bits, by_call in cells:
        wl, q, info = R.width_case(kind, code_bits, 300, 600)
        for max_d in range(0, min(3, info["G"] - 1) + 1):
            ref = O.c_nearest(kind, wl, q, max_d)
            if by_call:
                assert R.auto_code_bits(kind, wl, max_d) == code_bits
                with _lib.tuning(nearest_scheme=_SCHEMES[scheme]):
                    idx, dist = barcode.nearest_whitelist(q, wl, max_distance=max_d, encoding=kind)
                _same(idx, dist, ref)
            idx, dist, pinfo = _plan_answers(kind, wl, q, code_bits, max_d, scheme)
            _same(idx, dist, ref)
            _check_info(pinfo, scheme, kind, code_bits, max_d, wl)


# ---------------------------------------------------------------- 2. open-addressing chains
@pytest.mark.parametrize("max_d", [0, 1, 2])
@pytest.mark.parametrize("kind,L", [(2, 24), (2, 32), (3, 17), (3, 21)])
def test_open_addressing_chains(kind, L, max_d):
    """Whitelists whose first pair key is shared by a chain of codes that starts in the table's
    last group: a partly filled group, an exactly full one, chains that run into the next groups
    and wrap to group 0 (so a unique exact match lies past the first group, out of the shortcut's
    sight), and a heavy key of 175 groups; with and without a duplicated chain code."""
    for nw, chain in R.OA_CHAINS:
        for dup in (False, True):
            wl, q, info = R.oa_chain_case(kind, L, max_d, nw, chain, dup=dup)
            idx, dist, pinfo = _plan_answers(kind, wl, q, info["code_bits"], max_d, "oa")
            assert pinfo["scheme"] == "oa" and pinfo["index_bytes"] == info["layout"]["index_bytes"]
            _same(idx, dist, O.c_nearest(kind, wl, q, max_d))


# ---------------------------------------------------------------- 3. CSR buckets
@pytest.mark.parametrize("load", [1, 4])
@pytest.mark.parametrize("kind,L", [(2, 8), (3, 8), (2, 32), (3, 21)])
def test_csr_heavy_buckets(kind, L, load):
    """One block constant over the whitelist (its part keeps one occupied bucket that holds every
    code), each block in turn, whitelists of 1..17 codes (provisional tables of 1, 2, 4, 8 and 16
    buckets), max_d 0..7 (all eight probe counts of the query kernel), 1 and 4 buckets per distinct
    block value (at 1, different block values share buckets)."""
    for max_d in range(8):
        for nw in R.CSR_HEAVY_NW:
            for block in range(max_d + 1):
                wl, q, info = R.csr_heavy_case(kind, L, max_d, nw, block)
                idx, dist, pinfo = _plan_answers(kind, wl, q, info["code_bits"], max_d, "csr", load=load)
                assert pinfo["scheme"] == "csr"
                assert pinfo["index_bytes"] == info[load]["layout"]["index_bytes"], (max_d, nw, block)
                _same(idx, dist, O.c_nearest(kind, wl, q, max_d))


# ---------------------------------------------------------------- 4. launch seams
@pytest.mark.parametrize("scheme", ["oa", "csr"])
@pytest.mark.parametrize("kind,L", [(2, 24), (3, 21)])
def test_launch_seams(kind, L, scheme):
    """One query, a workgroup less one, exactly one, one more, two and one more; outputs one
    element into a larger buffer (not 16-byte aligned) with guard values around them; the same plan
    queried twice."""
    import torch
    wl, q_all, info = R.width_case(kind, kind * L, 300, 600)
    d_wl = torch.from_numpy(wl.view(np.int64)).cuda()
    for max_d in (1, 2):
        ref_i, ref_d = O.c_nearest(kind, wl, q_all, max_d)
        with _lib.tuning(nearest_scheme=_SCHEMES[scheme]):
            plan = _lib.NearestPlan(kind, d_wl.data_ptr(), wl.size, kind * L, max_d)
        try:
            assert plan.info()["scheme"] == scheme
            for nq in (1, 255, 256, 257, 513):
                d_q = torch.from_numpy(q_all[:nq].view(np.int64)).cuda()
                for _ in range(2):
                    out_i = torch.full((nq + 5,), 7, dtype=torch.int32, device="cuda")
                    out_d = torch.full((nq + 5,), 9, dtype=torch.uint8, device="cuda")
                    plan.query(d_q.data_ptr(), nq, out_i[1:].data_ptr(), out_d[1:].data_ptr())
                    torch.cuda.synchronize()
                    got_i, got_d = out_i.cpu().numpy(), out_d.cpu().numpy()
                    assert np.array_equal(got_i[1:nq + 1], ref_i[:nq]) and np.array_equal(got_d[1:nq + 1], ref_d[:nq])
                    assert got_i[0] == 7 and (got_i[nq + 1:] == 7).all()
                    assert got_d[0] == 9 and (got_d[nq + 1:] == 9).all()
        finally:
            plan.close()


# ---------------------------------------------------------------- 5. whitelists that are not A/C/G/T
@pytest.mark.parametrize("scheme", ["auto", "oa", "csr"])
@pytest.mark.parametrize("L", [16, 21])
def test_whitelists_with_other_triplets(L, scheme):
    """ThreeBit whitelists holding an N, a 0 in the middle, a 5, a 7 and a code one base short;
    queries with the same triplets at the same and at other positions (N against N is distance 0
    under the XOR rule: the brute force decides)."""
    wl, q, info = R.odd_whitelist_case(L)
    for max_d in (1, 2):
        ref = O.c_nearest(3, wl, q, max_d)
        with _lib.tuning(nearest_scheme=_SCHEMES[scheme]):
            idx, dist = barcode.nearest_whitelist(q, wl, max_distance=max_d, encoding=3)
        _same(idx, dist, ref)
        idx, dist, pinfo = _plan_answers(3, wl, q, info["code_bits"], max_d, scheme)
        _same(idx, dist, ref)
        assert pinfo["scheme"] != "halves"
        if scheme != "auto":
            _check_info(pinfo, scheme, 3, info["code_bits"], max_d, wl)


# ---------------------------------------------------------------- 6. the user-facing forms
@pytest.mark.parametrize("max_d", [1, 2])
@pytest.mark.parametrize("kind,L", [(2, 24), (3, 21)])
def test_corrector_forms_past_16_bases(kind, L, max_d):
    """WhitelistCorrector.nearest in three batches (one empty) and .count against the brute
    force's indices, 2,000 codes and 20,000 queries."""
    wl, q, info = R.width_case(kind, kind * L, 2000, 20000)
    ref_i, ref_d = O.c_nearest(kind, wl, q, max_d)
    corr = barcode.WhitelistCorrector(wl, max_distance=max_d, encoding=kind, barcode_length=L)
    try:
        got_i, got_d = [], []
        for lo, hi in ((0, 7001), (7001, 7001), (7001, q.size)):
            i, d = corr.nearest(q[lo:hi])
            assert i.size == hi - lo and d.size == hi - lo
            got_i.append(np.array(i))
            got_d.append(np.array(d))
        _same(np.concatenate(got_i), np.concatenate(got_d), (ref_i, ref_d))
        counts, n_none, n_tie = corr.count(q)
        assert np.array_equal(counts, np.bincount(ref_i[ref_i >= 0], minlength=wl.size))
        assert n_none == int((ref_i == -1).sum()) and n_tie == int((ref_i == -2).sum())
        assert n_none > 0 and n_tie > 0 and counts.sum() > 0
    finally:
        corr.close()
