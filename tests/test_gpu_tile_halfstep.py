"""The int8 SPECTRAL tile leaves out stage 2's last butterfly (column bit 11) for N-tile 1, where
both M-tiles share a bin: it squares U = H_32 B[0] and V = H_32 B[1] instead of U + V and U - V
(tile_reg_kernel in sctools_amd/csrc/spectral.hip; tests/test_tile_halfstep_host.py has the
algebra).  The two-code sets of test_gpu_tile_digits give U = +-V or V = 0 everywhere; the sets here
make U and V unrelated: every non-empty subset of the four values of digit (10, 11), alone and
crossed with one other bit, random sets whose columns hold several codes, and columns of 125 and
126 codes (both sides of the chain form's launch rule) beside codes that vary bits 10 and 11.
Every case is one full SPECTRAL count compared bin for bin with the C oracle, with the chain form
allowed (tile_chain=1) and with the shift form forced (tile_chain=0)."""
import itertools

import numpy as np
import pytest

from oracle import oracle as O
from sctools_amd import _lib
from test_tile_chain_host import chain_max_m

pytestmark = pytest.mark.gpu

BITS = 14
DIGIT = [d << 10 for d in range(4)]
SUBSETS = [list(s) for r in range(1, 5) for s in itertools.combinations(DIGIT, r)]
OTHER_BITS = list(range(10)) + [12, 13, 14, 31]  # every other column bit, the lowest and highest slice bit
MASK_BITS = (10, 11, 0, 5, 7, 12)  # the random sets' column bits: 64 columns


def _ref(codes):
    """The oracle's histogram; every fixture's sums to C(n, 2)."""
    n = codes.size
    assert np.unique(codes).size == n
    ref = [int(v) for v in O.c_hist_rows(codes)[:17]] if n > 1 else [0] * 17
    assert sum(ref) == n * (n - 1) // 2
    return ref


def _spectral_hist(codes, chain):
    torch = pytest.importorskip("torch")
    d_codes = torch.from_numpy(codes.view(np.int64)).cuda()
    with _lib.tuning(tile_chain=chain):
        plan = _lib.AllPairsPlan(d_codes.data_ptr(), codes.size, 32, scheme=_lib.SCHEME_SPECTRAL)
    try:
        assert plan.scheme == _lib.SCHEME_SPECTRAL
        assert plan.spectral_info()["elem_bytes"] == 1  # the register tile
        counts = torch.zeros(plan.ncounts, dtype=torch.int64, device="cuda")
        plan.build()
        plan.count(counts.data_ptr(), 0, plan.items)
        return [int(v) for v in plan.counts_to_hist(counts.cpu().numpy().view(np.uint64))]
    finally:
        plan.close()


def _check(codes, name, bins=2):
    codes = np.asarray(codes, dtype=np.uint64)
    ref = _ref(codes)
    assert sum(1 for v in ref if v) >= bins, (name, ref)
    for chain in (1, 0):
        got = _spectral_hist(codes, chain)
        print("%s tile_chain=%d: %s" % (name, chain, got))
        assert got == ref, (name, chain)
    return ref


def crossed(subset, e):
    """The subset plus v ^ 2^e for part of it (every other member, from the first)."""
    return subset + [v ^ (1 << e) for v in subset[0::2]]


def test_digit_subsets_alone():
    """Codes d << 10 alone: all pairs lie inside digit (10, 11), at distance 1 (so one bin, or none
    for a single code: these fifteen sets cannot fill two)."""
    for s in SUBSETS:
        ref = _check(s, "subset %s" % [v >> 10 for v in s], bins=0)
        assert ref[1] == len(s) * (len(s) - 1) // 2


@pytest.mark.parametrize("e", OTHER_BITS)
def test_digit_subsets_crossed_with_one_bit(e):
    for s in SUBSETS:
        codes = crossed(s, e)
        # one member and its image make one pair; every larger set has pairs at distances 1 and 2
        _check(codes, "subset %s x bit %d" % ([v >> 10 for v in s], e), bins=2 if len(s) > 1 else 1)


def random_set(n, seed):
    """n distinct codes: column bits under MASK_BITS, slice bits free."""
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < n:
        c = sum(int(b) << bit for b, bit in zip(rng.integers(0, 2, len(MASK_BITS)), MASK_BITS))
        out.add(c | (int(rng.integers(0, 1 << 18)) << BITS))
    return np.array(sorted(out), dtype=np.uint64)


@pytest.mark.parametrize("n,seed", [(3, 31), (64, 32), (4096, 33)])
def test_random_sets_under_a_mask(n, seed):
    codes = random_set(n, seed)
    cols = np.bincount((codes & np.uint64((1 << BITS) - 1)).astype(np.int64))
    if n > 3:
        assert 1 < cols.max() <= chain_max_m()  # several codes a column, the chain form admitted
    _check(codes, "random%d" % n)


def dense_columns(m_b):
    """125 codes in column A and m_b in column B (slice bits alone differ within a column), beside
    codes that run through digit (10, 11) in two other columns."""
    rng = np.random.default_rng(50)
    col_a, col_b = 0x0C21, 0x0421  # bits 10 and 11 set / bit 10 set
    hi_a = rng.choice(1 << 18, 125, replace=False).astype(np.uint64)
    hi_b = rng.choice(1 << 18, 126, replace=False).astype(np.uint64)[:m_b]
    side = [np.uint64((d << 10) | base | (int(h) << BITS)) for base in (0x0023, 0x2203) for d in range(4)
            for h in rng.choice(1 << 18, 3, replace=False)]
    return np.concatenate([(hi_a << np.uint64(BITS)) | np.uint64(col_a), (hi_b << np.uint64(BITS)) | np.uint64(col_b),
                           np.array(side, np.uint64)])


@pytest.mark.parametrize("m_b", [126, 125])
def test_columns_of_125_and_126(m_b):
    """m_b = 126: the densest column is past kChainMaxM and the plan keeps the shift form; 125: the
    same set one code short, the chain form."""
    codes = dense_columns(m_b)
    cols = np.bincount((codes & np.uint64((1 << BITS) - 1)).astype(np.int64))
    assert cols.max() == m_b and np.sort(cols)[-2] == 125 and chain_max_m() == 125
    _check(codes, "dense125_%d" % m_b)
