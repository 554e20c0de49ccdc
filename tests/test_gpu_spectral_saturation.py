"""Both SPECTRAL tile kernels at the bounds their range arguments rest on (spectral_families.py):
every column of the column space holding 127 identical codes, so that stage 1 reaches +-8128 per
plane, the packed int16 plane sums +-32,512 (tile16_kernel: y = 64 and 16,320, four-wave LDS
halves of 256 and 65,280), |F| = 2^bits * 127, the weight sums the bound under the kernels'
"< 2^62" comments, and the 16-bit build's packed byte counts 0x7F in every byte -- bin for bin
against the C oracle on the distinct codes.  Each case is counted with the codes sorted (one
build workgroup owns all 127 codes of a column) and shuffled (spread over the workgroups), in
one slice range and in three that cut walks."""
import numpy as np
import pytest

import spectral_families as F
from oracle import oracle as O
from sctools_amd import _lib

pytestmark = pytest.mark.gpu

RANGES = ([(0, 1 << 18)], [(0, 1001), (1001, 70001), (70001, 1 << 18)])


def _masks(bits):
    return [0, (1 << bits) - 1] + [1 << b for b in range(bits)]


def _e(bits):
    return 1 | (1 << (31 - bits))  # lowest | highest slice bit


def _hists(codes, want_info):
    """The plan's histogram of `codes` for each entry of RANGES (one plan, fresh counts each)."""
    torch = pytest.importorskip("torch")
    d_codes = torch.from_numpy(codes.view(np.int64)).cuda()
    plan = _lib.AllPairsPlan(d_codes.data_ptr(), codes.size, 32, scheme=_lib.SCHEME_SPECTRAL)
    try:
        assert plan.scheme == _lib.SCHEME_SPECTRAL and plan.items == 1 << 18
        info = plan.spectral_info()
        assert {k: info[k] for k in want_info} == want_info, info
        out = []
        for ranges in RANGES:
            counts = torch.zeros(plan.ncounts, dtype=torch.int64, device="cuda")
            credited = 0
            for b, e in ranges:  # as separate ranks would: each builds, then counts its slices
                plan.build(0, b, e)
                plan.count(counts.data_ptr(), b, e)
                credited += plan.range_pairs(b, e)
            assert credited == codes.size * (codes.size - 1) // 2
            out.append(plan.counts_to_hist(counts.cpu().numpy().view(np.uint64)))
        return out
    finally:
        plan.close()


def _check(bits, distinct, m, name):
    n = distinct.size * m
    ref = F.family_hist(distinct, m)
    assert sum(ref) == n * (n - 1) // 2
    want_info = {"column_bits": bits, "elem_bytes": 1, "max_column": m}
    for order, shuffle_seed in (("sorted", None), ("shuffled", 5)):
        codes = F.expand(distinct, m, shuffle_seed)
        assert codes.size == n
        for ranges, hist in zip(RANGES, _hists(codes, want_info)):
            got = [int(v) for v in hist]
            print("%s bits=%d m=%d %s %d ranges: %s" % (name, bits, m, order, len(ranges), got))
            assert got == ref, (name, order, len(ranges))
            assert sum(got) == n * (n - 1) // 2


@pytest.mark.parametrize("mask", _masks(14), ids=lambda v: "mask%04x" % v)
def test_saturated_14bit_columns(mask):
    _check(14, F.saturating_distinct(14, mask, _e(14)), 127, "sat")


@pytest.mark.parametrize("mask", _masks(16), ids=lambda v: "mask%04x" % v)
def test_saturated_16bit_columns(mask):
    _check(16, F.saturating_distinct(16, mask, _e(16)), 127, "sat")


# seeds -127 in half of the slices (stage 1: -8128 at P' = 0 in every row); bit 6 is a stage-2
# bit of both tiles
@pytest.mark.parametrize("bits", [14, 16])
@pytest.mark.parametrize("mask", [0, 1 << 6], ids=lambda v: "mask%04x" % v)
def test_saturated_negative(bits, mask):
    _check(bits, F.saturating_distinct(bits, mask, _e(bits), neg=True), 127, "neg")


# stage-1 outputs m * (a sum of 64 signs): low bytes 0x00, 0xFF and their neighbours under
# positive and negative high bytes, where a wrong borrow of the two-byte split would show
@pytest.mark.parametrize("bits", [14, 16])
@pytest.mark.parametrize("m", [127, 126, 64, 1])
def test_random_signs_byte_split(bits, m):
    distinct = F.random_sign_distinct(bits, seed=100 * bits + m)
    if bits == 16 and m < 32:
        # (14-bit columns would take int8 seeds: 4 m <= 127) the forced 16-bit layout
        with _lib.tuning(spectral_columns=16):
            _check(bits, distinct, m, "rand")
    else:
        _check(bits, distinct, m, "rand")


def test_column_of_128_leaves_int8():
    """One 14-bit column of 128 codes among 16,383 of 127: the plan's rule (<= 127 in every
    column for int8 seeds) on its other side -- int16 seeds, and still exact."""
    bits, m = 14, 127
    distinct = F.saturating_distinct(bits, 1 << 6, _e(bits))
    x = distinct[0x1ABC]
    codes = np.concatenate([F.expand(distinct, m), [x]]).astype(np.uint64)
    np.random.default_rng(3).shuffle(codes)
    n = codes.size
    # the extra copy pairs with the m copies of every distinct code (its own included, at 0)
    row = O.c_hist_rows(np.concatenate([[x], distinct]).astype(np.uint64), 0, 1)[:17]
    ref = [a + m * int(b) for a, b in zip(F.family_hist(distinct, m), row)]
    assert sum(ref) == n * (n - 1) // 2
    for ranges, hist in zip(RANGES, _hists(codes, {"column_bits": 14, "elem_bytes": 2, "max_column": 128})):
        got = [int(v) for v in hist]
        print("m128 %d ranges: %s" % (len(ranges), got))
        assert got == ref, len(ranges)
