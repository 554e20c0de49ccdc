"""Host emulation of the half step of tile_reg_kernel's stage 2 (sctools_amd/csrc/spectral.hip).
Stage 2 is H_64 = H_2 x H_32 over the set Q; its outer bit is column bit 11 (the M-tile t on the
output side, the K-step ks on the input side).  With U = H_32 B[0] and V = H_32 B[1] the two
M-tiles are c[0] = U + V and c[1] = U - V.  For N-tile nt = 1 the digit (10, 11) = nt + 2 t is 1
or 3, non-zero either way, so both M-tiles fall into one bin, which needs only
c[0]^2 + c[1]^2 = 2 (U^2 + V^2): the kernel stops at U and V there (two chains of two MFMAs on the
+H_32 block) and doubles their squares.  For nt = 0 the digit is 0 or 2 and the M-tiles differ in
weight: the rule must not be applied.

Both operand paths are built bit for bit as the kernel builds them (int16 pairs of y = v + 128, the
two v_perm byte selections; chain form: 4 h by the dword shift and mask against 64 H; shift form:
the high bytes' result << 8) over the whole admitted range of stage-1 outputs: |v| <= 64 * 125 in
the chain form, plane sums y up to +-32,640 in the shift form, both ends of every byte carry."""
import numpy as np
import pytest

from test_tile32_map_host import (LANES, digit_weight, direct, h_regs, halves, load_plane, mfma, out_index,
                                  out_weight, pairs16, pk_add16, signed_bytes, split16, stage2, CSP_START)
from test_tile_chain_host import Y_MAX, Y_MIN, h_words, pack_pairs, split_chain, stage2_chain

SUM_MAX = 32640  # |plane sum of y| the int16 pairs hold (tile_reg_kernel's comment)
I16 = np.arange(16)


def half_shift(pr):
    """int16 pairs pr[mt][lane][8] -> [U, V], shift form: chain ks = (H_32 high[ks] << 8) + H_32 low[ks]."""
    H = h_regs()
    out = []
    for ks in range(2):
        lo, hi = split16(pr[ks])
        c = mfma(H[0][0], hi, np.zeros((64, 16), np.int64))
        assert np.all(np.abs(c) < 2 ** 23)
        out.append(mfma(H[0][0], lo, c << 8))
    return out


def half_chain(pr):
    """The same, chain form: (64 H_32) (4 h[ks]) + H_32 low[ks] in one accumulator."""
    H, H64 = h_words()
    out = []
    for ks in range(2):
        lo, hi4 = split_chain(pr[ks])
        c = mfma(H64[0][0], signed_bytes(hi4), np.zeros((64, 16), np.int64))
        c = mfma(H[0][0], signed_bytes(lo), c)
        assert np.all(np.abs(c) < 2 ** 31)
        out.append(c)
    return out


def _edges(rng, hmax, lim):
    """Values a borrow or a carry of the byte split away from every multiple of 256 in range."""
    y = 256 * rng.integers(-hmax, hmax + 1, (2, 64, 16)) + rng.integers(-2, 2, (2, 64, 16))
    return np.clip(y, -lim, lim)


def _y_vectors(lo, hi):
    """y = v + 128 of both K-steps, [ks][lane][i], over [lo, hi] including the bounds."""
    rng = np.random.default_rng(11)
    alt = np.where((I16[None, :] + LANES[:, None]) & 1, hi, lo)
    yield "max", np.full((2, 64, 16), hi)
    yield "min", np.full((2, 64, 16), lo)
    yield "max_min", np.stack([np.full((64, 16), hi), np.full((64, 16), lo)])
    yield "alternating", np.stack([alt, alt[::-1]])
    yield "one_step_zero", np.stack([alt, np.full((64, 16), 128)])  # v = 0 in K-step 1: U = +-c, V = 0
    yield "edges", np.clip(_edges(rng, hi >> 8, hi), lo, hi)
    yield "byte_ends", np.clip(rng.choice([-256, -255, -129, -128, -1, 0, 127, 128, 255, 256], (2, 64, 16)) +
                               256 * rng.integers(lo >> 8, (hi >> 8) + 1, (2, 64, 16)), lo, hi)
    yield "random", rng.integers(lo, hi + 1, (2, 64, 16))
    yield "unrelated", np.stack([rng.integers(lo, hi + 1, (64, 16)), rng.integers(-3, 4, (64, 16))])


CHAIN = list(_y_vectors(Y_MIN, Y_MAX))
SHIFT = list(_y_vectors(-SUM_MAX, SUM_MAX))


def _check_identity(full, half):
    (c0, c1), (U, V) = full, half
    assert np.array_equal(U + V, c0) and np.array_equal(U - V, c1)
    assert np.array_equal(c0 ** 2 + c1 ** 2, 2 * (U ** 2 + V ** 2))  # element by element, |.| < 2^31: no wrap
    assert np.array_equal(c0 ** 2 + c1 ** 2, (2 * U) * U + (2 * V) * V)  # the plane-sum calls' form
    assert int(np.abs(2 * U).max()) < 2 ** 31 and int(np.abs(2 * V).max()) < 2 ** 31


@pytest.mark.parametrize("name,y", CHAIN, ids=[n for n, _ in CHAIN])
def test_chain_form(name, y):
    assert y.min() >= Y_MIN and y.max() <= Y_MAX
    pr = [pack_pairs(y[ks]) for ks in range(2)]
    assert all(np.array_equal(halves(pr[ks]), y[ks]) for ks in range(2))
    _check_identity(stage2_chain(pr), half_chain(pr))
    _check_identity(stage2(pr, h_regs(), 1), half_shift(pr))  # the shift form admits the chain's range too


@pytest.mark.parametrize("name,y", SHIFT, ids=[n for n, _ in SHIFT])
def test_shift_form(name, y):
    assert y.min() >= -SUM_MAX and y.max() <= SUM_MAX
    pr = [pack_pairs(y[ks]) for ks in range(2)]
    assert all(np.array_equal(halves(pr[ks]), y[ks]) for ks in range(2))
    _check_identity(stage2(pr, h_regs(), 1), half_shift(pr))


def test_bounds_are_reached():
    names = dict(CHAIN)
    assert names["max"].max() == Y_MAX == 64 * 125 + 128 and names["min"].min() == Y_MIN == -64 * 125 + 128
    names = dict(SHIFT)
    assert names["max"].max() == SUM_MAX and names["min"].min() == -SUM_MAX
    for vecs in (CHAIN, SHIFT):
        lows = np.concatenate([(y & 0xFF).ravel() for _, y in vecs])
        assert {0, 1, 127, 128, 254, 255} <= set(lows.tolist())  # both ends of the byte carries


def test_nt1_rows_carry_one_weight():
    """Row i (and the lane) of U and V weighs what row i of c[0] and c[1] weighs for nt = 1: the
    index of (l, i) differs between the M-tiles in bit 11 alone, inside a digit that bit 10 = nt
    already makes non-zero."""
    l, i = LANES[:, None], I16[None, :]
    e0, e1 = out_index(l, i, 1, 0), out_index(l, i, 1, 1)
    assert np.array_equal(e0 ^ e1, np.full((64, 16), 1 << 11))
    assert np.array_equal(digit_weight(e0), digit_weight(e1))
    w = digit_weight(l) + digit_weight(i & 3) + digit_weight(i >> 2) + 1  # the kernel: entry wi + 1
    assert np.array_equal(out_weight(l, i, 1, 0), w) and np.array_equal(out_weight(l, i, 1, 1), w)
    assert np.array_equal(digit_weight(e0), w)
    assert digit_weight(I16 & 3).max() + digit_weight(I16 >> 2).max() == 2  # wi in {0, 1, 2}: Bn[3]


def test_nt0_must_keep_the_butterfly():
    """nt = 0: the M-tiles are digit values 0 and 2, one weight apart everywhere, and binning
    2 (U^2 + V^2) at either weight moves mass between bins."""
    l, i = LANES[:, None], I16[None, :]
    assert np.array_equal(out_weight(l, i, 0, 1) - out_weight(l, i, 0, 0), np.ones((64, 16), np.int64))
    y = dict(CHAIN)["unrelated"]
    pr = [pack_pairs(y[ks]) for ks in range(2)]
    c0, c1 = stage2_chain(pr)
    U, V = half_chain(pr)
    assert np.array_equal(c0 ** 2 + c1 ** 2, 2 * (U ** 2 + V ** 2))  # the sum still holds ...
    assert not np.array_equal(c0 ** 2, U ** 2 + V ** 2)  # ... but its split between the two bins is lost
    assert not np.array_equal(c1 ** 2, U ** 2 + V ** 2)


def emulate_half(row, z, chain):
    """One slice as the kernel now bins it: per-plane N-tile 0 squares in accB, N-tile 1's
    U^2 + V^2 in Bn[wi], the plane-sum calls in accA with N-tile 1 as (2 U) U at entry wi + 1;
    flush: bins[w + k] += accA[k], bins[w + k + 1] += 4 (accB[k] + 2 Bn[k - 1]) - accA[k]."""
    H = h_regs()
    wi = digit_weight(I16 & 3) + digit_weight(I16 >> 2)
    accA, accB = np.zeros((64, 4), dtype=object), np.zeros((64, 4), dtype=object)
    Bn = np.zeros((64, 3), dtype=object)
    csp = np.full((2, 2, 64, 8), CSP_START, np.uint32)

    def squares_nt0(c, acc):
        for t in range(2):
            for k in range(4):
                acc[:, k] += (c[t][:, wi + t == k].astype(object) ** 2).sum(axis=1)

    for R in range(4):
        d = load_plane(row, R)
        for nt in range(2):
            pr = []
            for mt in range(2):
                c1 = np.full((64, 16), 128, np.int64)
                for ks in range(2):
                    c1 = mfma(d[2 * mt + ks], H[nt][ks], c1)
                pr.append(pairs16(c1))
                csp[nt][mt] = pk_add16(csp[nt][mt], pr[mt])
            if nt == 0:
                squares_nt0(stage2_chain(pr) if chain else stage2(pr, H, 0), accB)
            else:
                for c in (half_chain(pr) if chain else half_shift(pr)):
                    for k in range(3):
                        Bn[:, k] += (c[:, wi == k].astype(object) ** 2).sum(axis=1)
    squares_nt0(stage2(csp[0], H, 0), accA)
    for c in half_shift(csp[1]):
        for k in range(3):
            accA[:, k + 1] += ((2 * c[:, wi == k]).astype(object) * c[:, wi == k].astype(object)).sum(axis=1)
    bins = np.zeros(17, dtype=object)
    wt = digit_weight(z) + digit_weight(LANES)
    for l in range(64):
        for k in range(4):
            bins[wt[l] + k] += accA[l, k]
            bins[wt[l] + k + 1] += 4 * (accB[l, k] + (2 * Bn[l, k - 1] if k else 0)) - accA[l, k]
    return bins


@pytest.mark.parametrize("chain", [True, False], ids=["chain", "shift"])
@pytest.mark.parametrize("seed,z,amp", [(1, 0, 125), (2, 0x2D, 125), (3, 0x3FFFF, 40)])
def test_slice_bins_match_direct_wht(seed, z, amp, chain):
    """A whole slice through both stages and the new flush against the direct 14-bit transform
    (columns of at most 125 codes, the chain form's launch rule)."""
    rng = np.random.default_rng(seed)
    row = rng.integers(-amp, amp + 1, 16384).astype(np.int8)
    if seed == 1:
        row[:6000] = 125  # long runs of the extreme value
    assert emulate_half(row, z, chain).tolist() == direct(row, z).tolist()
