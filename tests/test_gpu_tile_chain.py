"""The int8 SPECTRAL tile's two stage-2 bodies (tile_reg_kernel<true>: the high bytes as 64 H
against 4 h, one MFMA chain per tile; <false>: the shift form) and the rule that picks one: the
chain when the densest 14-bit column holds <= 125 codes, else the shift.  Every histogram is bin
for bin the C oracle's.
  (a) every column at 125 codes: the chain at its range ends (stage 1 at +-8000);
  (b) the same with one column raised to 126: the rule's other side;
  (c) a few thousand random codes, the tile_chain switch on and off;
  (d) y = v + 128 on both sides of multiples of 256: one column of 125 codes alone (as the case
      was first written: y stays within [3, 253], one high byte), and pairs of columns that one
      stage-1 bit (bit 0) joins, 125 + k and 125 - k codes' worth of seed per stage-2 row (bits
      5-9, 11), so that neighbouring bytes of the operand dwords hold 253..260 and 3..-4.
The path is the rule's: a plan reports its densest column, and a count with the switch off (the
shift form for every plan) must give the same histogram."""
import numpy as np
import pytest

import spectral_families as F
from oracle import oracle as O
from sctools_amd import _lib, synthetic
from test_tile_chain_host import chain_max_m

pytestmark = pytest.mark.gpu

BITS, M = 14, 125
E = 1 | (1 << 17)  # lowest | highest slice bit


def _hist(codes, max_column, chain):
    torch = pytest.importorskip("torch")
    d_codes = torch.from_numpy(codes.view(np.int64)).cuda()
    with _lib.tuning(tile_chain=chain):
        plan = _lib.AllPairsPlan(d_codes.data_ptr(), codes.size, 32, scheme=_lib.SCHEME_SPECTRAL)
    try:
        assert plan.scheme == _lib.SCHEME_SPECTRAL
        info = plan.spectral_info()
        assert (info["column_bits"], info["elem_bytes"], info["max_column"]) == (BITS, 1, max_column), info
        counts = torch.zeros(plan.ncounts, dtype=torch.int64, device="cuda")
        plan.build()
        plan.count(counts.data_ptr(), 0, plan.items)
        return [int(v) for v in plan.counts_to_hist(counts.cpu().numpy().view(np.uint64))]
    finally:
        plan.close()


def _check(codes, ref, max_column, name):
    n = codes.size
    assert sum(ref) == n * (n - 1) // 2
    assert (max_column <= chain_max_m()) == (max_column <= M)
    for chain in (1, 0):  # 1: the rule decides (the chain up to 125 codes per column); 0: the shift form
        got = _hist(codes, max_column, chain)
        print("%s max_column=%d tile_chain=%d: %s" % (name, max_column, chain, got))
        assert got == ref, (name, chain)


_FAMILIES = {
    "plus": lambda: F.saturating_distinct(BITS, 0, E),
    "bit6neg": lambda: F.saturating_distinct(BITS, 1 << 6, E, neg=True),
    "ones": lambda: F.saturating_distinct(BITS, (1 << BITS) - 1, E),
    "signs": lambda: F.random_sign_distinct(BITS, seed=125),
}
_family_cache = {}


def _family(name):
    if name not in _family_cache:
        distinct = _FAMILIES[name]()
        _family_cache[name] = (distinct, F.family_hist(distinct, M))
    return _family_cache[name]


@pytest.mark.parametrize("name", list(_FAMILIES))
def test_saturated_125(name):
    """(a) 16,384 x 125 codes: seeds +-125 in every column, stage 1 +-8000, y = 8128 and -7872."""
    distinct, ref = _family(name)
    _check(F.expand(distinct, M, shuffle_seed=9), ref, M, name)


def test_one_column_of_126():
    """(b) one column of 126 among 16,383 of 125: y can reach 8192, the plan keeps the shift form."""
    distinct, base = _family("bit6neg")
    x = distinct[0x1ABC]
    codes = np.concatenate([F.expand(distinct, M), [x]]).astype(np.uint64)
    np.random.default_rng(3).shuffle(codes)
    row = O.c_hist_rows(np.concatenate([[x], distinct]).astype(np.uint64), 0, 1)[:17]
    ref = [a + M * int(b) for a, b in zip(base, row)]
    _check(codes, ref, M + 1, "m126")


@pytest.mark.parametrize("n,seed", [(3000, 11), (5003, 12)])
def test_sparse_switch_on_and_off(n, seed):
    """(c) random whitelist codes: the same histogram from both bodies, and the oracle's."""
    codes = synthetic.whitelist_codes(n, 16, seed=seed)
    ref = [int(v) for v in O.c_hist_rows(codes)[:17]]
    max_column = int(np.bincount((codes & np.uint64((1 << BITS) - 1)).astype(np.int64)).max())
    _check(codes, ref, max_column, "sparse%d" % n)


def test_one_column_alone():
    """(d) one column of 125 distinct codes, every other column empty."""
    rng = np.random.default_rng(21)
    hi = rng.choice(1 << 18, M, replace=False).astype(np.uint64)
    codes = (hi << np.uint64(BITS)) | np.uint64(0x2B5C)
    _check(codes, [int(v) for v in O.c_hist_rows(codes)[:17]], M, "column")


# the six stage-2 column bits: the 64 stage-2 rows q of one stage-1 group
_Q_BITS = (5, 6, 7, 8, 9, 11)


@pytest.mark.parametrize("offset", [0, 3])
def test_carry_between_bytes(offset):
    """(d) per stage-2 row q a column of 125 equal codes and, one stage-1 bit away, a column of
    k_q = (q + offset) % 8 equal codes, slice parts 0 or E at random: stage 1 gives +-125 +- k_q,
    so y = 128 + v takes 253..260, -4..3 and the values between in neighbouring operand bytes --
    on both sides of 256 and of 0, where a high byte steps by one."""
    rng = np.random.default_rng(40 + offset)
    parts = []
    for q in range(64):
        col = sum(((q >> b) & 1) << bit for b, bit in enumerate(_Q_BITS)) | (2 << 12)
        ha, hb = (int(v) * E for v in rng.integers(0, 2, 2))
        parts.append(np.full(M, col | (ha << BITS), np.uint64))
        parts.append(np.full((q + offset) % 8, (col | 1) | (hb << BITS), np.uint64))
    codes = np.concatenate(parts)
    rng.shuffle(codes)
    _check(codes, [int(v) for v in O.c_hist_rows(codes)[:17]], M, "carry%d" % offset)
