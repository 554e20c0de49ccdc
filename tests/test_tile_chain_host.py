"""Host emulation of the unbroken stage-2 chain of tile_reg_kernel<true> (sctools_amd/csrc/
spectral.hip): H v = (64 H) (4 h) + H (l' - 128) with y = v + 128 = 256 h + l', the high K-steps
on A = 64 H (bytes 0x40 / 0xC0, made from the H registers by one shift and one mask) against
B = 4 h = (Bh << 2) & 0xFCFCFCFC, all four K-steps into one int32 accumulator.  The operands are
built bit for bit as the kernel builds them -- int16 pairs of y, the two v_perm byte selections,
the dword shift and mask reinterpreted as int8 -- and checked against the plain H_64 @ v:
exhaustively over the range the launch rule admits (every y in [-7872, 8128] in every byte of a
dword, so the packed shift leaks nothing between bytes), on vectors at both range ends, and on
the gate (y = 8192, first reached by a column of 126 codes, overflows; the rule excludes it)."""
import os
import re

import numpy as np
import pytest

from test_tile32_map_host import LANES, h_regs, mfma, pairs16, perm, result_regs, signed_bytes

Y_MIN, Y_MAX = -64 * 125 + 128, 64 * 125 + 128  # stage 1: |v| <= 64 m, m <= 125


def chain_max_m():
    """The launch rule's bound, from the kernel source."""
    src = open(os.path.join(os.path.dirname(__file__), "..", "sctools_amd", "csrc", "spectral.hip")).read()
    (m,) = re.findall(r"constexpr unsigned kChainMaxM = (\d+);", src)
    return int(m)


def pack_pairs(y):
    """int16 values y[..., 2 k] -> words [..., k] (value 2 k in the low half), as pairs16 leaves them."""
    u = (np.asarray(y, np.int64) & 0xFFFF).astype(np.uint32)
    return u[..., 0::2] | (u[..., 1::2] << np.uint32(16))


def split_chain(pr):
    """int16 pairs pr[..., 2 d] -> (low operand words, 4 h operand words) [..., d]."""
    lo = perm(pr[..., 1::2], pr[..., 0::2], 0x06040200) ^ np.uint32(0x80808080)
    hi = perm(pr[..., 1::2], pr[..., 0::2], 0x07050301)
    hi4 = ((hi.astype(np.uint64) << np.uint64(2)) & np.uint64(0xFCFCFCFC)).astype(np.uint32)  # the dword shift
    return lo, hi4


def h_words():
    """The kernel's H registers as packed words [t][ks][lane][4] (bytes 0x01 / 0xFF) and 64 H made
    from them as the kernel does: (H << 6) & 0xC0C0C0C0, the block t = ks = 1 ^ 0x80808080."""
    H = h_regs()
    w = np.ascontiguousarray((H[0][0] & 0xFF).astype(np.uint8)).view(np.uint32)
    assert signed_bytes(w).tolist() == H[0][0].tolist()
    w64 = ((w.astype(np.uint64) << np.uint64(6)) & np.uint64(0xC0C0C0C0)).astype(np.uint32)
    neg = w64 ^ np.uint32(0x80808080)
    return H, [[signed_bytes(w64), signed_bytes(w64)], [signed_bytes(w64), signed_bytes(neg)]]


def stage2_chain(pr):
    """int16 pairs pr[mt][lane][8] -> c[t][lane][i]: the four-MFMA chain of each M-tile t."""
    H, H64 = h_words()
    ops = [split_chain(pr[mt]) for mt in range(2)]
    out = []
    for t in range(2):
        c = np.zeros((64, 16), np.int64)
        for ks in range(2):
            c = mfma(H64[t][ks], signed_bytes(ops[ks][1]), c)
        for ks in range(2):
            c = mfma(H[t][ks], signed_bytes(ops[ks][0]), c)
        assert np.all(np.abs(c) < 2 ** 31)  # one int32 accumulator throughout
        out.append(c)
    return out


def plain(v):
    """H_64 @ v for stage-1 outputs v[mt][lane][i] (k = 32 mt + 16 (l >> 5) + i, column l & 31),
    in stage 2's result registers: c[t][lane][i]."""
    k = np.arange(64)
    H64 = np.array([[(-1) ** bin(a & b).count("1") for b in k] for a in k], np.int64)
    V = np.zeros((64, 32), np.int64)
    for mt in range(2):
        for l in LANES:
            V[32 * mt + 16 * (l >> 5):32 * mt + 16 * (l >> 5) + 16, l & 31] = v[mt][l]
    C = H64 @ V
    return [result_regs(C[32 * t:32 * t + 32]) for t in range(2)]


def test_64h_bytes():
    H, H64 = h_words()
    for t in range(2):
        for ks in range(2):
            assert np.array_equal(H64[t][ks], 64 * H[t][ks])


@pytest.mark.parametrize("pos", range(4))
def test_every_y_in_every_byte(pos):
    """Every y the rule admits, in byte `pos` of an operand dword, beside neighbours at both range
    ends and at the byte borders: 64 * (4 h byte) + (low byte) is v = y - 128 in all four bytes."""
    ys = np.arange(Y_MIN, Y_MAX + 1)
    for other in (Y_MIN, Y_MAX, -1, 0, 255, 256, -256, -257):
        y = np.full((ys.size, 4), other, np.int64)
        y[:, pos] = ys
        lo, hi4 = split_chain(pack_pairs(y))
        h4, l = signed_bytes(hi4), signed_bytes(lo)
        assert np.array_equal(h4, 4 * (y >> 8)), (pos, other)
        assert np.array_equal(64 * h4 + l, y - 128), (pos, other)


def _vectors():
    rng = np.random.default_rng(7)
    alt = np.where((np.arange(16)[None, :] + LANES[:, None]) & 1, 8000, -8000)
    yield "plus", [np.full((64, 16), 8000), np.full((64, 16), 8000)]
    yield "minus", [np.full((64, 16), -8000), np.full((64, 16), -8000)]
    yield "alternating", [alt, -alt]
    yield "halves", [np.full((64, 16), 8000), np.full((64, 16), -8000)]
    # around every multiple of 256 in range, a borrow or carry of the split away
    edges = 256 * rng.integers(-31, 32, (2, 64, 16)) + rng.integers(-2, 2, (2, 64, 16)) - 128
    yield "edges", [np.clip(edges[0], -8000, 8000), np.clip(edges[1], -8000, 8000)]
    yield "random", list(rng.integers(-8000, 8001, (2, 64, 16)))


@pytest.mark.parametrize("name,v", list(_vectors()), ids=[n for n, _ in _vectors()])
def test_chain_is_h64_times_v(name, v):
    pr = [pairs16(np.asarray(v[mt], np.int64) + 128) for mt in range(2)]
    got, want = stage2_chain(pr), plain(v)
    for t in range(2):
        assert np.array_equal(got[t], want[t]), (name, t)
    if name in ("plus", "minus"):  # a constant vector: one transform point of 64 * 8000
        assert max(int(np.abs(c).max()) for c in got) == 64 * 8000


def test_gate():
    """y = 8192 makes 4 h = 128, which as int8 is -128: the chain is wrong there, the first column
    count whose stage 1 reaches it is 126, and the launch rule stops at 125."""
    m = chain_max_m()
    assert m == 125
    assert 64 * m + 128 == Y_MAX <= 8191 < 64 * (m + 1) + 128 == 8192
    assert -64 * m + 128 == Y_MIN and 4 * (Y_MIN >> 8) >= -128
    lo, hi4 = split_chain(pack_pairs(np.array([[8192, 0, 0, 0]])))
    assert signed_bytes(hi4)[0, 0] == -128 and 4 * (8192 >> 8) == 128
    v = [np.zeros((64, 16), np.int64), np.zeros((64, 16), np.int64)]
    v[0][5, 3] = 8192 - 128
    pr = [pairs16(v[mt] + 128) for mt in range(2)]
    assert not np.array_equal(stage2_chain(pr)[0], plain(v)[0])
    v[0][5, 3] = Y_MAX - 128  # the admitted maximum beside it is exact
    pr = [pairs16(v[mt] + 128) for mt in range(2)]
    assert all(np.array_equal(a, b) for a, b in zip(stage2_chain(pr), plain(v)))
