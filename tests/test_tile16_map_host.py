"""Host emulation of the 16-bit-column tile transform (tile16_kernel in
sctools_amd/csrc/spectral16.hip) for one 64 KiB slice of int8 seeds, one workgroup of four waves:
the lane loads, the operand and result layouts of v_mfma_i32_16x16x64_i8, stage 1 from an
accumulator of 8192, the int16 pairs, the LDS image of U_r as 64-bit words that all four waves add
into modulo 2^64, the + 0x8080 rebias, the plane sums from 0x80808080, the byte split, stage 2
with its -2016 correction at Q' = 0, V as the sum of the U_r transforms, and the flush with both
Parseval levels and the thread / quarter / compile-time digit weights -- against a direct 16-bit
Walsh-Hadamard transform binned by the digit weight of the true index.  Words are packed as the
hardware holds them, so a carry between halves or a wrong bias changes the result.  The GPU digit
pins (test_gpu_tile16_digits.py) pin the kernel; this pins the index and range arithmetic on CPU."""
import numpy as np
import pytest

from test_tile32_map_host import chi, digit_weight, halves, perm, pk_add16, signed_bytes, wht

LANES = np.arange(64)
REGS = np.arange(4)
ACC_START = 8192
CSP_START = 0x80808080
CORR = -2016


# ---- the kernel's maps -------------------------------------------------------------------------
def lane_off(l, wave):
    return 16 * (l >> 4) + 64 * (l & 15) + 16384 * wave


def load_plane(row, wave, R):
    """d[mt][lane][j]: the four 16-B loads of plane R of wave `wave`."""
    j = np.arange(16)
    return np.stack([row[lane_off(LANES, wave)[:, None] + 4096 * R + 1024 * mt + j[None, :]] for mt in range(4)])


def h_regs():
    """H[q][lane][j] = H_64[16 q + (l & 15)][16 (l >> 4) + j] as the kernel builds them."""
    j = np.arange(16)
    out = []
    for q in range(4):
        r, c = (16 * q + (LANES & 15))[:, None], 16 * (LANES >> 4)[:, None] + j[None, :]
        par = np.zeros((64, 16), np.int64)
        for b in range(6):
            par ^= ((r & c) >> b) & 1
        out.append(np.where(par == 1, -1, 1).astype(np.int64))
    return out


def operand(regs):
    """A (row, k) or, transposed, B (k, column) matrix of a 16-byte-per-lane operand:
    row / column = l & 15, k = 16 (l >> 4) + j."""
    return np.asarray(regs).reshape(4, 16, 16).transpose(1, 0, 2).reshape(16, 64)


def result_regs(c):
    """C (16 x 16) -> [lane][i]: row 4 (l >> 4) + i, column l & 15."""
    return c[4 * (LANES >> 4)[:, None] + REGS[None, :], (LANES & 15)[:, None]]


def mfma(a_regs, b_regs, c_regs):
    return c_regs + result_regs(operand(a_regs) @ operand(b_regs).T)


def pairs16(c1):
    """int32 accumulators c1[mt][lane][4] -> pr[mt][lane][2]: registers (0, 1) and (2, 3) as int16 pairs."""
    assert np.all(np.abs(c1) < 2 ** 31)
    u = (np.asarray(c1) & 0xFFFFFFFF).astype(np.uint32)
    return np.stack([perm(u[..., 1], u[..., 0], 0x05040100), perm(u[..., 3], u[..., 2], 0x05040100)], axis=-1)


def split16(pr):
    """pr[mt][lane][2] -> (low byte - 128, high byte) operands [lane][16], byte 4 mt + i."""
    lo = perm(pr[..., 1], pr[..., 0], 0x06040200) ^ np.uint32(0x80808080)  # [mt][lane]
    hi = perm(pr[..., 1], pr[..., 0], 0x07050301)
    return signed_bytes(lo.T), signed_bytes(hi.T)


def stage2(pr, H, corr=0):
    """Byte-split pairs of one quarter -> c[q2][lane][i]; corr: the start of the high-byte chain
    at Q' = 0."""
    lo, hi = split16(pr)
    out = []
    for q2 in range(4):
        c = np.zeros((64, 4), np.int64)
        if q2 == 0:
            c[:16, 0] = corr  # Q' = 0: lanes 0-15, element 0
        c = mfma(H[q2], hi, c)
        assert np.all(np.abs(c) < 2 ** 23)  # int32 after the shift
        out.append(mfma(H[q2], lo, c << 8))
    return np.stack(out)


def out_index(l, i, q, q2):
    """True 12-bit column index of stage 2's output (lane l, register i, stage-1 quarter q, stage-2
    tile q2): P' = 16 q + (l & 15); stage 2's k = 16 (l >> 4) + 4 mt + i carries column bits 6, 7
    in k bits 0, 1 (i), bits 10, 11 in k bits 2, 3 (mt) and bits 8, 9 in k bits 4, 5 (the row's
    l >> 4), and its output row 16 q2 + 4 (l >> 4) + i labels them the same way."""
    return (l & 15) | (q << 4) | (i << 6) | (q2 << 8) | ((l >> 4) << 10)


def wt_thread(l):
    return digit_weight(l & 15) + digit_weight(l >> 4)


def wt_const(i, q2):
    return digit_weight(i) + digit_weight(q2)


def emulate(row, z, stats=None, acc_start=ACC_START, corr=CORR):
    """The 17 per-weight sums of F^2 of one 64 KiB slice (slice index z) and the 12-bit transforms
    G[s][r] of its sixteen planes, as one workgroup of tile16_kernel computes them."""
    H = h_regs()
    bins = np.zeros(17, dtype=object)
    U = np.zeros(4 * 4 * 4 * 64, np.uint64)  # word ((r 4 + q) 4 + mt) 64 + lane
    G = np.zeros((4, 4, 4096), np.int64)
    k_of = wt_const(REGS[None, :], REGS[:, None])  # [q2][i]

    def squares(c, acc, base):  # c[q2][lane][i] into acc[lane][base + compile-time weight of (q2, i)]
        for k in range(3):
            acc[:, base + k] += (c.transpose(0, 2, 1)[k_of == k].astype(object) ** 2).sum(axis=0)

    def flush_own(wave, accG, accT):
        b = digit_weight(z) + wt_thread(LANES)
        for l in range(64):
            for k in range(4):
                bins[b[l] + k + 1] += 4 * accT[l, k]
                bins[b[l] + k + 2] += 16 * accG[l, k] - 4 * accT[l, k]

    def flush_quarter(wave, accU, accV):
        b = digit_weight(z) + wt_thread(LANES) + digit_weight(wave)  # wt_q
        for l in range(64):
            for k in range(3):
                bins[b[l] + k] += accV[l, k]
                bins[b[l] + k + 1] += 4 * accU[l, k] - 2 * accV[l, k]
                bins[b[l] + k + 2] += accV[l, k] - 4 * accU[l, k]

    for wave in range(4):
        accG, accT = np.zeros((64, 4), dtype=object), np.zeros((64, 4), dtype=object)
        csp = np.full((4, 4, 64, 2), CSP_START, np.uint32)  # [q][mt][lane][h]
        for R in range(4):
            d = load_plane(row, wave, R)
            for q in range(4):
                c1 = np.stack([mfma(d[mt], H[q], np.full((64, 4), acc_start, np.int64)) for mt in range(4)])
                pr = pairs16(c1)
                csp[q] = pk_add16(csp[q], pr)
                words = (pr[..., 1].astype(np.uint64) << np.uint64(32)) | pr[..., 0].astype(np.uint64)
                for mt in range(4):
                    w0 = ((R * 4 + q) * 4 + mt) * 64
                    U[w0:w0 + 64] += words[mt]  # ds_add_u64: modulo 2^64, carries cross the halves
                c2 = stage2(pr, H, corr)
                squares(c2, accG, int(digit_weight(q)))
                G[wave][R][out_index(LANES[None, :, None], REGS[None, None, :], q, REGS[:, None, None])] = c2
                if stats is not None:
                    stats.setdefault("y", []).extend([int(c1.min()), int(c1.max())])
        for q in range(4):
            squares(stage2(csp[q], H), accT, int(digit_weight(q)))
        if stats is not None:
            stats.setdefault("csp", []).extend([int(halves(csp).min()), int(halves(csp).max())])
        flush_own(wave, accG, accT)
    if stats is not None:
        h16 = np.stack([(U >> np.uint64(16 * k)) & np.uint64(0xFFFF) for k in range(4)])
        stats.setdefault("lds", []).extend([int(h16.min()), int(h16.max())])
    for wave in range(4):  # after the barrier: quarter q = wave of every U_r
        accU, accV = np.zeros((64, 3), dtype=object), np.zeros((64, 3), dtype=object)
        fv = np.zeros((4, 64, 4), np.int64)
        for r in range(4):
            v = np.stack([U[((r * 4 + wave) * 4 + mt) * 64:((r * 4 + wave) * 4 + mt) * 64 + 64] for mt in range(4)])
            uu = np.stack([pk_add16((v & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.uint32(0x80808080)),
                           pk_add16((v >> np.uint64(32)).astype(np.uint32), np.uint32(0x80808080))], axis=-1)
            c2 = stage2(uu, H)
            squares(c2, accU, 0)
            fv += c2
        assert np.all(np.abs(fv) < 2 ** 31)
        squares(fv, accV, 0)
        flush_quarter(wave, accU, accV)
    return bins, G


def direct(row, z):
    F = wht(row.astype(np.int64))
    w = digit_weight(z) + digit_weight(np.arange(65536))
    bins = np.zeros(17, dtype=object)
    for k in range(17):
        bins[k] = int((F[w == k].astype(object) ** 2).sum())
    return bins


def check(row, z, stats=None):
    bins, G = emulate(row, z, stats)
    for s in range(4):
        for r in range(4):
            p = 16384 * s + 4096 * r
            assert np.array_equal(G[s][r], wht(row[p:p + 4096].astype(np.int64))), (s, r)
    assert bins.tolist() == direct(row, z).tolist()


def test_maps_are_bijections():
    j = np.arange(16)
    cols = np.concatenate([(lane_off(LANES, w)[:, None] + 4096 * R + 1024 * mt + j[None, :]).ravel()
                           for w in range(4) for R in range(4) for mt in range(4)])
    assert np.array_equal(np.sort(cols), np.arange(65536))
    # every load instruction of a wave reads one whole contiguous KiB
    one = np.sort((lane_off(LANES, 0)[:, None] + j[None, :]).ravel())
    assert np.array_equal(one, np.arange(1024))
    idx = np.concatenate([out_index(LANES[:, None], REGS[None, :], q, q2).ravel() for q in range(4) for q2 in range(4)])
    assert np.array_equal(np.sort(idx), np.arange(4096))
    # the binned weight (thread + quarter + compile time) is the digit weight of the true index
    for q in range(4):
        for q2 in range(4):
            e = out_index(LANES[:, None], REGS[None, :], q, q2)
            w = wt_thread(LANES)[:, None] + digit_weight(q) + wt_const(REGS[None, :], q2)
            assert np.array_equal(w, digit_weight(e))
    # the LDS words of U: (r, q, mt, lane) each once
    words = np.array([((r * 4 + q) * 4 + mt) * 64 + l for r in range(4) for q in range(4) for mt in range(4)
                      for l in range(64)])
    assert np.array_equal(np.sort(words), np.arange(4096))
    # the H operand is H_64, symmetric: the same registers serve as stage 1's B and stage 2's A
    h64 = np.concatenate([operand(h) for h in h_regs()])
    assert np.array_equal(h64, h64.T) and np.array_equal(h64 @ h64, 64 * np.eye(64, dtype=np.int64))


@pytest.mark.parametrize("seed,z,amp", [(1, 0, 127), (2, 0x2D, 127), (3, 0xFFFF, 40)])
def test_tile16_matches_direct_wht(seed, z, amp):
    rng = np.random.default_rng(seed)
    row = rng.integers(-amp, amp + 1, 65536).astype(np.int8)
    if seed == 1:  # high-energy planes: long runs of the extreme value
        row[:24000] = 127
    check(row, z)


# every column at the int8 limit: the seeds of the saturating families of spectral_families.py
# (stage 1 bits 0-5, stage 2 bits 6-11, planes 12 and 13, waves 14 and 15)
SATURATED = [("plus", 0, 127), ("minus", 0, -127), ("bit0", 1, 127), ("bit5", 1 << 5, 127), ("bit6", 1 << 6, 127),
             ("bit10", 1 << 10, 127), ("bit12", 1 << 12, 127), ("bit14", 1 << 14, 127), ("bit15", 1 << 15, 127),
             ("ones", 0xFFFF, 127), ("mixed", 0xAC63, 127), ("bit5neg", 1 << 5, -127)]
_reached = {}


@pytest.mark.parametrize("name,mask,amp", SATURATED, ids=[s[0] for s in SATURATED])
def test_tile16_saturated_rows(name, mask, amp):
    stats = {}
    check((amp * chi(mask, 65536)).astype(np.int8), 0x155, stats)
    _reached[name] = stats


def test_tile16_saturated_rows_sit_on_the_bounds():
    """The rows above reach what the kernel's comments allow: y = v + 8192 of 64 and 16,320, LDS
    halves (four waves' y) of 256 and 65,280, plane sums (+ 128) of -32,384 and 32,640."""
    for name, mask, amp in SATURATED:
        if name not in _reached:
            emulate((amp * chi(mask, 65536)).astype(np.int8), 0, _reached.setdefault(name, {}))
    for key, lo, hi in (("y", 64, 16320), ("lds", 256, 65280), ("csp", -32384, 32640)):
        v = [x for s in _reached.values() for x in s[key]]
        assert (min(v), max(v)) == (lo, hi), key
    assert max(_reached["plus"]["y"]) == 16320 and max(_reached["plus"]["lds"]) == 65280
    assert min(_reached["minus"]["y"]) == 64 and min(_reached["minus"]["lds"]) == 256
    assert min(_reached["bit5neg"]["y"]) == 64 and max(_reached["bit5"]["y"]) == 16320
    # a wave-bit character: the four waves' y cancel to 4 * 8192 in the LDS halves where v != 0
    assert max(_reached["bit14"]["y"]) == 16320 and max(_reached["bit14"]["lds"]) == 4 * 8192


def test_emulation_notices_wrong_constants():
    """The two hand-derived constants are live in the emulation: one off in either changes the
    result (as the same mutants of the kernel fail the GPU tests)."""
    row = np.random.default_rng(9).integers(-127, 128, 65536).astype(np.int8)
    want = direct(row, 3).tolist()
    assert emulate(row, 3)[0].tolist() == want
    assert emulate(row, 3, corr=-2015)[0].tolist() != want
    assert emulate(row, 3, acc_start=8191)[0].tolist() != want
