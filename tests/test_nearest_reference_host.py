"""CPU checks of tests/nearest_reference.py: the mirror of the open-addressing and CSR nearest
layouts answers as the brute force at every width, every builder's input reaches the seam it
claims, each deliberately wrong variant of the mirror is told from the brute force by the inputs
aimed at its seam, and the width inputs hold every outcome.  No GPU, no kernel."""

import numpy as np
import pytest

import nearest_reference as R
from oracle import oracle as O


def _brute(kind, wl, q, max_d):
    idx, dist = O.c_nearest(kind, wl, q, max_d)
    return idx.tolist(), dist.tolist()


def _agrees(scheme, kind, code_bits, max_d, wl, q, load=4, wrong=None):
    got = R.mirror_nearest(scheme, kind, code_bits, max_d, wl, q, load=load, wrong=wrong)
    return got is None or got == _brute(kind, wl, q, max_d)


# ---------------------------------------------------------------- width sweep
@pytest.mark.parametrize("kind", [2, 3])
def test_mirror_equals_brute_force_at_every_width(kind):
    for code_bits in range(1, 65):
        wl, q, info = R.width_case(kind, code_bits, 40, 150, seed=1)
        for max_d in range(0, min(3, info["G"] - 1) + 1):
            want = _brute(kind, wl, q, max_d)
            oa = R.mirror_nearest("oa", kind, code_bits, max_d, wl, q)
            # ten keys at max_d = 3; max_d + 2 blocks need as many positions
            assert (oa is None) == (max_d == 3 or (max_d > 0 and max_d + 2 > info["G"])), (code_bits, max_d)
            assert oa is None or oa == want, ("oa", code_bits, max_d)
            for load in (1, 4):
                assert R.mirror_nearest("csr", kind, code_bits, max_d, wl, q, load=load) == want, (code_bits, max_d, load)


def test_block_split_and_slot_count():
    # 21 ThreeBit positions in 4 blocks: 5, 5, 5, 6 positions; six pair keys
    lay = R.oa_layout(3, 63, 2, 3000)
    assert [R.block_range(21, 4, b) for b in range(4)] == [(0, 5), (5, 10), (10, 15), (15, 21)]
    assert len(lay["keys"]) == 6 and lay["slots"] == 8192 and lay["index_bytes"] == 6 * 8192 * 16
    assert lay["keymasks"][0] == (1 << 30) - 1
    # 22 positions, the top one a single bit: the last block's mask ends at bit 63
    lay = R.oa_layout(3, 64, 1, 1)
    assert lay["slots"] == 4 and lay["keymasks"][2] == ((1 << 64) - 1) ^ ((1 << 21) - 1)
    assert R.oa_layout(2, 8, 3, 10) is None and R.oa_layout(2, 4, 1, 10) is None  # 10 keys; P > G
    assert R.oa_layout(2, 6, 1, 10) is not None


# ---------------------------------------------------------------- open-addressing chains
_CHAIN_SHAPES = [(2, 24), (2, 32), (3, 17), (3, 21)]


@pytest.mark.parametrize("kind,L", _CHAIN_SHAPES)
@pytest.mark.parametrize("max_d", [0, 1, 2])
def test_chain_cases_reach_their_seams(kind, L, max_d):
    for nw, chain in R.OA_CHAINS[:-1]:
        for dup in (False, True):
            wl, q, info = R.oa_chain_case(kind, L, max_d, nw, chain, dup=dup)
            lay = info["layout"]
            tables = R.oa_build(lay, wl)
            assert wl.size == nw and q.size == nw * (L + 1 + (max_d > 0))
            keys0 = {int(wl[j]) & lay["keymasks"][0] for j in info["chain_idx"]}
            assert len(keys0) == 1  # one pair key for the whole chain
            outside = 0
            for j in info["chain_idx"]:
                groups, seen = R.oa_probe(lay, tables, 0, int(wl[j]))
                assert groups[0] == lay["groups"] - 1  # the key's first group is the table's last
                assert sum(e[0] & lay["keymasks"][0] in keys0 for e in seen) >= chain
                if chain >= 4:  # the group is full: the sequence runs on, and wraps to group 0
                    assert len(groups) >= 2 and groups[1] == 0
                if chain == 4 and nw == 4:  # exactly full: nothing of the chain lies past it
                    assert len(seen) == 4 and len(groups) == 2
                first = tables[0][groups[0] * R.GROUP:(groups[0] + 1) * R.GROUP]
                outside += all(e is None or e[1] != j for e in first)
            if max_d > 0 and not dup:
                # the exact match of the 5th and later chain codes lies outside the first group
                assert outside == max(0, chain - 4)
            assert _agrees("oa", kind, info["code_bits"], max_d, wl, q)


def test_heavy_chain_case():
    wl, q, info = R.oa_chain_case(3, 17, 2, 3000, 700)
    lay = info["layout"]
    tables = R.oa_build(lay, wl)
    assert lay["groups"] == 2048 and len(lay["keys"]) == 6
    groups, seen = R.oa_probe(lay, tables, 0, int(wl[info["chain_idx"][0]]))
    assert groups[0] == 2047 and groups[1] == 0 and len(groups) >= 176  # 700 entries: 175 groups and on
    assert sum(e[1] in set(info["chain_idx"]) for e in seen) == 700
    some = q[::97]  # the mirror walks 700 slots per chain query: a sample here, every query on the GPU
    assert _agrees("oa", 3, info["code_bits"], 2, wl, some)


# ---------------------------------------------------------------- CSR heavy buckets
_HEAVY_SHAPES = [(2, 8), (3, 8), (2, 32), (3, 21)]


@pytest.mark.parametrize("kind,L", _HEAVY_SHAPES)
def test_heavy_cases_reach_their_seams(kind, L):
    provisional = {1: 1, 2: 1, 3: 2, 4: 2, 5: 4, 8: 4, 9: 8, 16: 8, 17: 16}
    for max_d in (0, 1, 3, 7):
        shared_somewhere = False
        for nw in R.CSR_HEAVY_NW:
            for block in range(max_d + 1):
                wl, q, info = R.csr_heavy_case(kind, L, max_d, nw, block)
                for load in (1, 4):
                    c = info[load]
                    assert c["heavy"] == nw and c["heavy_part_buckets"] == 1  # one bucket holds them all
                    part = c["layout"]["parts"][block]
                    assert part["buckets"] == min(provisional[nw], load)  # one occupied bucket -> `load`
                    assert all(p["buckets"] <= provisional[nw] for p in c["layout"]["parts"])
                    if nw <= 2:  # one-bucket tables: multiplier 0, shift 63
                        assert all((p["mul"], p["shift"], p["buckets"]) == (0, 63, 1) for p in c["layout"]["parts"])
                    assert _agrees("csr", kind, info["code_bits"], max_d, wl, q, load=load)
                shared_somewhere |= info[1]["shared"]
                if max_d >= 1 and nw >= 3 and 4 ** (L // (max_d + 1)) >= 32:
                    # more distinct block values than provisional buckets: some bucket is shared
                    assert info[1]["shared"], (max_d, nw, block)
        assert shared_somewhere or max_d == 0


# ---------------------------------------------------------------- discrimination
def _caught(scheme, wrong, cases, load=4):
    """True if the wrong variant disagrees with the brute force on at least one of the cases."""
    for kind, max_d, wl, q, info in cases:
        if not _agrees(scheme, kind, info["code_bits"], max_d, wl, q, load=load, wrong=wrong):
            return True
    return False


def _with(kind, max_d, case):
    return (kind, max_d) + tuple(case)


def test_wrong_open_addressing_variants_are_caught():
    for kind, L in _CHAIN_SHAPES:
        for max_d in (1, 2):
            long_chains = [_with(kind, max_d, R.oa_chain_case(kind, L, max_d, n, n)) for n in (5, 6, 9, 13)]
            # a chain code past the first group is lost if the walk stops there, or at the table's end
            assert _caught("oa", "first_group_only", long_chains)
            assert _caught("oa", "no_wrap", long_chains)
            # (taken together: in tables of 4 or 8 groups another key's walk can cross the chain's
            # groups and meet the lost code by accident, so one small case alone may not tell)
            # an exactly full group that is not walked past changes nothing: chain = 4 cannot tell
            assert not _caught("oa", "no_wrap", [_with(kind, max_d, R.oa_chain_case(kind, L, max_d, 4, 4))])
            dups = [_with(kind, max_d, R.oa_chain_case(kind, L, max_d, n, n, dup=True)) for n in (2, 3, 4, 5)]
            for case in dups:
                assert _caught("oa", "shortcut_ignores_dup", [case])
                assert _caught("oa", "no_tie", [case])
            # max_d = 1: a substitution in block 0 leaves only the key of blocks 1 and 2, which holds
            # the last block (max_d = 2 needs two substitutions: the width inputs, below)
            assert max_d == 2 or _caught("oa", "drop_last_block", long_chains)
        # max_d = 0: the chain is copies of one code; the flag alone keeps the shortcut from answering
        copies = [_with(kind, 0, R.oa_chain_case(kind, L, 0, n, n)) for n in (2, 5)]
        for case in copies:
            assert _caught("oa", "shortcut_ignores_dup", [case])


def test_wrong_csr_variants_are_caught():
    for kind, L in _HEAVY_SHAPES:
        for max_d in (1, 3, 7):
            for load in (1, 4):
                # a query that shares the constant block with the whole whitelist and lies further
                # than max_d from all of it is answered by nothing; without the distance check the
                # heavy bucket answers it
                cases = [_with(kind, max_d, R.csr_heavy_case(kind, L, max_d, nw, 0)) for nw in (5, 9, 17)]
                if L > max_d + 1:  # (at L = 8, max_d = 7 nothing that shares a block is further than 7)
                    assert _caught("csr", "no_distance_check", cases, load=load)
                # the last block constant: a code with one base substituted in every other block is
                # met only in the heavy bucket of the last part
                cases = [_with(kind, max_d, R.csr_heavy_case(kind, L, max_d, nw, max_d)) for nw in (5, 9, 17)]
                if L > max_d + 1:  # (one base per block: its four values share the few buckets of
                    # so small a table, and another part's shared bucket meets the code anyway)
                    assert _caught("csr", "drop_last_block", cases, load=load)
    for kind in (2, 3):  # duplicated codes and midpoints: ties
        wl, q, info = R.width_case(kind, 16 * kind, 300, 600)
        for max_d in (0, 1, 2):
            assert _caught("csr", "no_tie", [(kind, max_d, wl, q, info)])
            assert _caught("oa", "no_tie", [(kind, max_d, wl, q, info)])
            if max_d:
                assert _caught("csr", "drop_last_block", [(kind, max_d, wl, q, info)])
                assert _caught("oa", "drop_last_block", [(kind, max_d, wl, q, info)])


# ---------------------------------------------------------------- outcome classes
def _width_cells():
    for kind, top in ((2, 32), (3, 21)):
        for L in range(1, top + 1):
            yield kind, kind * L
    for kind, bits in ((2, 31), (2, 63), (3, 46), (3, 47), (3, 62), (3, 63), (3, 64)):
        yield kind, bits


def test_width_cases_hold_every_outcome():
    """From the brute force's answers alone: every cell of the GPU width test whose space is at
    least four times the whitelist holds a query answered uniquely at 0, one answered uniquely at
    max_d, a tie and a query that matches nothing."""
    checked = 0
    for kind, code_bits in _width_cells():
        wl, q, info = R.width_case(kind, code_bits, 300, 600)
        G = info["G"]
        assert R.auto_code_bits(kind, wl, 0) == code_bits
        assert set(info["classes"]) >= {"exact", "sub", "high" if code_bits < 64 else "exact", "random"}
        if kind == 3:
            assert "odd" in info["classes"]
        if 4 ** G < 4 * 300:
            continue
        assert info["holes"] == 4
        for max_d in range(0, min(3, G - 1) + 1):
            idx, dist = O.c_nearest(kind, wl, q, max_d)
            assert ((idx >= 0) & (dist == 0)).any(), (kind, code_bits, max_d)
            assert ((idx >= 0) & (dist == max_d)).any(), (kind, code_bits, max_d)
            assert (idx == -2).any() and (idx == -1).any(), (kind, code_bits, max_d)
            checked += 1
    assert checked > 150


def test_odd_whitelists_are_not_acgt():
    for L in (16, 21):
        wl, q, info = R.odd_whitelist_case(L)
        digits = [[R.get_digit(3, int(w), p) for p in range(L)] for w in wl]
        bad = {d for row in digits for d in row if d not in (1, 2, 3, 4)}
        assert bad == {0, 5, 6, 7}
        assert R.auto_code_bits(3, wl, 1) == 3 * L
        for max_d in (1, 2):
            assert _agrees("oa", 3, 3 * L, max_d, wl, q) and _agrees("csr", 3, 3 * L, max_d, wl, q)
            idx, dist = O.c_nearest(3, wl, q, max_d)
            assert (idx[:wl.size] == np.arange(wl.size)).all()  # N against N: distance 0
