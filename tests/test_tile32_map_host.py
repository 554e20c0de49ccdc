"""Host emulation of the register-resident tile transform (tile_reg_kernel in
sctools_amd/csrc/spectral.hip) for one 16 KiB slice of int8 seeds: the lane loads, the operand
and result layouts of v_mfma_i32_32x32x32_i8, stage 1, the byte split, stage 2, the Parseval step
over the four planes and the digit weight of every (lane, register, tile) -- against a direct
14-bit Walsh-Hadamard transform binned by the digit weight of the true index.  The GPU parity and
digit tests pin the kernel; this pins the index arithmetic on CPU."""
import numpy as np
import pytest

LANES = np.arange(64)


def digit_weight(z):
    z = np.asarray(z, dtype=np.int64)
    return sum(((z >> (2 * d)) & 3) != 0 for d in range(16)).astype(np.int64)


def wht(x):
    """Walsh-Hadamard transform of a vector (index bit k in <-> index bit k out)."""
    x = np.array(x, dtype=np.int64)
    n = x.size
    h = 1
    while h < n:
        y = x.reshape(n // (2 * h), 2, h)  # index = block * 2h + half * h + r
        x = np.stack([y[:, 0, :] + y[:, 1, :], y[:, 0, :] - y[:, 1, :]], axis=1).reshape(n)
        h *= 2
    return x


# ---- the kernel's maps -------------------------------------------------------------------------
def lane_off(l):
    return 16 * (l >> 5) + 32 * ((l >> 3) & 1) + 64 * (l & 3) + 256 * ((l >> 4) & 1) + 512 * ((l >> 2) & 1)


def load_plane(row, R):
    """d[k][lane][j]: the four 16-B loads (k = 2 mt + ks) of plane R."""
    j = np.arange(16)
    return np.stack([row[lane_off(LANES)[:, None] + 4096 * R + 1024 * k + j[None, :]] for k in range(4)])


def h_regs():
    """H[t][ks][lane][j] as the kernel builds them."""
    j = np.arange(16)
    r, c = (LANES & 31)[:, None], 16 * (LANES >> 5)[:, None] + j[None, :]
    par = np.zeros((64, 16), np.int64)
    for b in range(6):
        par ^= ((r & c) >> b) & 1
    hp = np.where(par == 1, -1, 1).astype(np.int64)
    return [[hp, hp], [hp, -hp]]


def operand(regs):
    """A (row, k) or, transposed, B (k, column) matrix of a 16-byte-per-lane operand:
    row / column = l & 31, k = 16 (l >> 5) + j."""
    m = np.zeros((32, 32), np.int64)
    for l in range(64):
        m[l & 31, 16 * (l >> 5):16 * (l >> 5) + 16] = regs[l]
    return m


def result_regs(c):
    """C (32 x 32) -> [lane][i]: row 8 (i >> 2) + 4 (l >> 5) + (i & 3), column l & 31."""
    i = np.arange(16)
    rows = 8 * (i >> 2)[None, :] + 4 * (LANES >> 5)[:, None] + (i & 3)[None, :]
    return c[rows, (LANES & 31)[:, None]]


def mfma(a_regs, b_regs, c_regs):
    return c_regs + result_regs(operand(a_regs) @ operand(b_regs).T)


def split16(y):
    """int16 values y = v + 128 -> (low byte - 128, high byte) as signed bytes."""
    assert np.all(np.abs(y) < 2 ** 15)
    u = y & 0xFFFF
    lo = ((u & 0xFF) ^ 0x80).astype(np.uint8).view(np.int8).astype(np.int64)
    hi = (u >> 8).astype(np.uint8).view(np.int8).astype(np.int64)
    return lo, hi


def stage2(y, H, nt):
    """y[mt][lane][i] -> c[t][lane][i] (M-tile t), as the kernel's stage2 lambda."""
    lo, hi = zip(*(split16(y[mt]) for mt in range(2)))
    out = []
    for t in range(2):
        c = np.zeros((64, 16), np.int64)
        for ks in range(2):
            c = mfma(H[t][ks], hi[ks], c)
        c = c << 8
        for ks in range(2):
            c = mfma(H[t][ks], lo[ks], c)
        out.append(c)
    return out


def out_index(l, i, nt, t):
    """True 12-bit column index of stage 2's output (lane l, register i, N-tile nt, M-tile t)."""
    return ((l & 31) | ((l >> 5) << 5) | ((i & 3) << 6) | ((i >> 2) << 8) | (nt << 10) | (t << 11))


def out_weight(l, i, nt, t):
    """Thread constant + compile-time constant, as the kernel bins it."""
    return digit_weight(l) + digit_weight(i & 3) + digit_weight(i >> 2) + digit_weight(nt | (2 * t))


def emulate(row, z):
    """The 17 per-weight sums of F^2 of one slice (slice index z) and the per-plane transforms."""
    H = h_regs()
    bins = np.zeros(17, dtype=object)
    accA = np.zeros((64, 4), dtype=object)
    accB = np.zeros((64, 4), dtype=object)
    csp = np.full((2, 2, 64, 16), -384, np.int64)
    G = np.zeros((4, 4096), np.int64)
    i = np.arange(16)

    def squares(c, nt, acc, sink=None):
        for t in range(2):
            w = digit_weight(i & 3) + digit_weight(i >> 2) + digit_weight(nt | (2 * t))
            for k in range(4):
                acc[:, k] += (c[t][:, w == k].astype(object) ** 2).sum(axis=1)
            if sink is not None:
                sink[out_index(LANES[:, None], i[None, :], nt, t)] = c[t]

    for R in range(4):
        d = load_plane(row, R)
        for nt in range(2):
            y = []
            for mt in range(2):
                c1 = np.full((64, 16), 128, np.int64)
                for ks in range(2):
                    c1 = mfma(d[2 * mt + ks], H[nt][ks], c1)
                csp[nt][mt] += c1
                assert np.all(np.abs(csp[nt][mt]) <= 32640)
                y.append(c1)
            squares(stage2(y, H, nt), nt, accB, G[R])
    for nt in range(2):
        squares(stage2(csp[nt], H, nt), nt, accA)
    wt = digit_weight(z) + digit_weight(LANES)
    for l in range(64):
        for k in range(4):
            bins[wt[l] + k] += accA[l, k]
            bins[wt[l] + k + 1] += 4 * accB[l, k] - accA[l, k]
    return bins, G


def direct(row, z):
    F = wht(row.astype(np.int64))
    w = digit_weight(z) + digit_weight(np.arange(16384))
    bins = np.zeros(17, dtype=object)
    for k in range(17):
        bins[k] = int((F[w == k].astype(object) ** 2).sum())
    return bins


def test_wht_helper():
    rng = np.random.default_rng(0)
    x = rng.integers(-5, 6, 64)
    h = np.array([[(-1) ** bin(a & b).count("1") for b in range(64)] for a in range(64)])
    assert np.array_equal(wht(x), h @ x)


def test_maps_are_bijections():
    j = np.arange(16)
    cols = np.concatenate([(lane_off(LANES)[:, None] + 4096 * R + 1024 * k + j[None, :]).ravel()
                           for R in range(4) for k in range(4)])
    assert np.array_equal(np.sort(cols), np.arange(16384))
    # every load instruction of a wave reads one whole contiguous KiB
    one = np.sort((lane_off(LANES)[:, None] + j[None, :]).ravel())
    assert np.array_equal(one, np.arange(1024))
    i = np.arange(16)
    idx = np.concatenate([out_index(LANES[:, None], i[None, :], nt, t).ravel() for nt in range(2) for t in range(2)])
    assert np.array_equal(np.sort(idx), np.arange(4096))
    # the binned weight is the digit weight of the true index
    for nt in range(2):
        for t in range(2):
            e = out_index(LANES[:, None], i[None, :], nt, t)
            assert np.array_equal(out_weight(LANES[:, None], i[None, :], nt, t), digit_weight(e))


@pytest.mark.parametrize("seed,z,amp", [(1, 0, 127), (2, 0x2D, 127), (3, 0x3FFFF, 40)])
def test_tile32_matches_direct_wht(seed, z, amp):
    rng = np.random.default_rng(seed)
    row = rng.integers(-amp, amp + 1, 16384).astype(np.int8)
    if seed == 1:  # high-energy planes: long runs of the extreme value
        row[:6000] = 127
    bins, G = emulate(row, z)
    for R in range(4):
        assert np.array_equal(G[R], wht(row[4096 * R:4096 * (R + 1)].astype(np.int64))), R
    assert bins.tolist() == direct(row, z).tolist()
