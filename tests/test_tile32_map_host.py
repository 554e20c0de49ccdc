"""Host emulation of the register-resident tile transform (tile_reg_kernel in
sctools_amd/csrc/spectral.hip) for one 16 KiB slice of int8 seeds: the lane loads, the operand
and result layouts of v_mfma_i32_32x32x32_i8, stage 1, the byte split, stage 2, the Parseval step
over the four planes and the digit weight of every (lane, register, tile) -- against a direct
14-bit Walsh-Hadamard transform binned by the digit weight of the true index.  The stage-1
outputs and the plane sums are held as the kernel holds them -- two int16 halves per 32-bit word,
added per half (v_pk_add_u16) from 0xFE80FE80, bytes taken out by the two v_perm selectors -- so a
value past the int16 range, a wrong bias or a wrong byte changes the result.  The GPU parity and
digit tests pin the kernel; this pins the index and range arithmetic on CPU."""
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


# ---- packed words, as the hardware holds them ---------------------------------------------------
def perm(s0, s1, sel):
    """v_perm_b32: result byte b = byte sel[b] of the 64-bit value {s0, s1} (s1 = bytes 0-3)."""
    src = (np.asarray(s0, np.uint64) << np.uint64(32)) | np.asarray(s1, np.uint64)
    out = np.zeros(src.shape, np.uint64)
    for b in range(4):
        k = (sel >> (8 * b)) & 0xFF
        assert k < 8
        out |= ((src >> np.uint64(8 * k)) & np.uint64(0xFF)) << np.uint64(8 * b)
    return out.astype(np.uint32)


def pk_add16(a, b):
    """v_pk_add_u16: both 16-bit halves added modulo 2^16, no carry from the low into the high."""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    lo = (a + b) & np.uint32(0xFFFF)
    hi = ((a >> np.uint32(16)) + (b >> np.uint32(16))) << np.uint32(16)
    return lo | hi


def halves(w):
    """The two int16 halves of packed words [..., k] -> int64 values [..., 2 k]."""
    w = np.asarray(w, np.uint32)
    h = np.stack([w & np.uint32(0xFFFF), w >> np.uint32(16)], axis=-1).astype(np.uint16).view(np.int16)
    return h.reshape(w.shape[:-1] + (2 * w.shape[-1],)).astype(np.int64)


def signed_bytes(w):
    """Packed words [..., k] -> their bytes as int8 values [..., 4 k] (an MFMA operand's k order)."""
    w = np.ascontiguousarray(w, np.uint32)
    return w.view(np.uint8).view(np.int8).reshape(w.shape[:-1] + (4 * w.shape[-1],)).astype(np.int64)


def pairs16(c1):
    """int32 accumulators [lane][16] -> eight words of int16 pairs (register 2 k low, 2 k + 1 high)."""
    assert np.all(np.abs(c1) < 2 ** 31)
    u = (c1 & 0xFFFFFFFF).astype(np.uint32)
    return perm(u[:, 1::2], u[:, 0::2], 0x05040100)


def split16(pr):
    """int16 pairs pr[lane][8] (y = v + 128) -> (low byte - 128, high byte) as the signed bytes of
    the two v_perm selections, four values per operand register."""
    lo = perm(pr[:, 1::2], pr[:, 0::2], 0x06040200) ^ np.uint32(0x80808080)
    hi = perm(pr[:, 1::2], pr[:, 0::2], 0x07050301)
    return signed_bytes(lo), signed_bytes(hi)


def stage2(pr, H, nt):
    """int16 pairs pr[mt][lane][8] -> c[t][lane][i] (M-tile t), as the kernel's stage2 lambda."""
    lo, hi = zip(*(split16(pr[mt]) for mt in range(2)))
    out = []
    for t in range(2):
        c = np.zeros((64, 16), np.int64)
        for ks in range(2):
            c = mfma(H[t][ks], hi[ks], c)
        assert np.all(np.abs(c) < 2 ** 23)  # int32 after the shift
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


CSP_START = 0xFE80FE80  # both halves -384


def emulate(row, z, stats=None, csp_start=CSP_START):
    """The 17 per-weight sums of F^2 of one slice (slice index z) and the per-plane transforms.
    The stage-1 outputs and the plane sums are the kernel's packed words (two int16 halves per
    uint32, added per half modulo 2^16), so a value past the int16 range or a wrong start wraps
    and changes the result.  `stats` collects the extremes of y = v + 128 and of the plane sums."""
    H = h_regs()
    bins = np.zeros(17, dtype=object)
    accA = np.zeros((64, 4), dtype=object)
    accB = np.zeros((64, 4), dtype=object)
    csp = np.full((2, 2, 64, 8), csp_start, np.uint32)
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
            pr = []
            for mt in range(2):
                c1 = np.full((64, 16), 128, np.int64)
                for ks in range(2):
                    c1 = mfma(d[2 * mt + ks], H[nt][ks], c1)
                pr.append(pairs16(c1))
                csp[nt][mt] = pk_add16(csp[nt][mt], pr[mt])
                if stats is not None:
                    stats.setdefault("y", []).extend([int(c1.min()), int(c1.max())])
            squares(stage2(pr, H, nt), nt, accB, G[R])
    if stats is not None:
        stats.setdefault("csp", []).extend([int(halves(csp).min()), int(halves(csp).max())])
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


def chi(mask, n=16384):
    """The character (-1)^<mask, c> over n columns."""
    c = np.arange(n)
    par = np.zeros(n, np.int64)
    for b in range(n.bit_length() - 1):
        if (mask >> b) & 1:
            par ^= (c >> b) & 1
    return 1 - 2 * par


# every column at the int8 limit: the seeds of the saturating families of spectral_families.py
# (stage 1 bits 0-4 and 10, stage 2 bits 5-9 and 11, planes 12 and 13)
SATURATED = [("plus", 0, 127), ("minus", 0, -127), ("bit0", 1, 127), ("bit5", 1 << 5, 127), ("bit10", 1 << 10, 127),
             ("bit11", 1 << 11, 127), ("bit12", 1 << 12, 127), ("ones", 0x3FFF, 127), ("mixed", 0x2C63, 127),
             ("bit5neg", 1 << 5, -127)]
_reached = {}


@pytest.mark.parametrize("name,mask,amp", SATURATED, ids=[s[0] for s in SATURATED])
def test_tile32_saturated_rows(name, mask, amp):
    row = (amp * chi(mask)).astype(np.int8)
    stats = {}
    bins, G = emulate(row, 0x155, stats)
    for R in range(4):
        assert np.array_equal(G[R], wht(row[4096 * R:4096 * (R + 1)].astype(np.int64))), R
    assert bins.tolist() == direct(row, 0x155).tolist()
    _reached[name] = stats


def test_tile32_saturated_rows_sit_on_the_bounds():
    """The rows above reach what the kernel's comments allow: y = v + 128 of +-8128 and plane
    sums (from -384) of 32,640 and -32,384 -- the whole int16 pair range the kernel relies on."""
    for name, mask, amp in SATURATED:
        if name not in _reached:
            emulate((amp * chi(mask)).astype(np.int8), 0, _reached.setdefault(name, {}))
    y = [v for s in _reached.values() for v in s["y"]]
    csp = [v for s in _reached.values() for v in s["csp"]]
    assert (min(y), max(y)) == (-8000, 8256)
    assert (min(csp), max(csp)) == (-32384, 32640)
    for name in ("plus", "bit0", "bit5", "bit12"):  # a character is one transform point: +8128 somewhere
        assert max(_reached[name]["y"]) == 8256, name
    for name in ("minus", "bit5neg"):
        assert min(_reached[name]["y"]) == -8000, name
    assert max(_reached["plus"]["csp"]) == 32640 and min(_reached["minus"]["csp"]) == -32384


def test_packed_words_carry_like_the_hardware():
    """The emulation wraps where the kernel would: a start one off moves every plane sum, and a
    sum past the int16 range changes the result instead of passing."""
    row = np.full(16384, 127, np.int8)
    assert emulate(row, 0, csp_start=CSP_START + 1)[0].tolist() != direct(row, 0).tolist()
    assert emulate(row, 0, csp_start=0xFF00FF00)[0].tolist() != direct(row, 0).tolist()  # 32,768 wraps
    a = np.array([0xFFFF0001, 0x7FFF8000], np.uint32)
    assert pk_add16(a, np.array([0x0001FFFF, 0x00018000], np.uint32)).tolist() == [0x00000000, 0x80000000]
    assert perm(np.uint32(0x44332211), np.uint32(0xDDCCBBAA), 0x07050301).tolist() == 0x4422DDBB
    assert split16(np.array([[0x00FF0100, 0x80007FFF] + [0] * 6], np.uint32))[0][0, :4].tolist() == [-128, 127, 127, -128]
    assert split16(np.array([[0x00FF0100, 0x80007FFF] + [0] * 6], np.uint32))[1][0, :4].tolist() == [1, 0, 127, -128]
