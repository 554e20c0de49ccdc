"""CPU, nothing loaded into Python: tests/host/nearest_index_layout_check.cpp includes the header that
holds the arithmetic of the nearest index layouts (sctools_amd/csrc/nearest_index_layout.h) -- the
functions nearest.hip's builders and sct_nearest_plan_info call -- and prints its answers.  It is
compiled by the host C++ compiler with AddressSanitizer and UBSan.  The answers are held against the
Python mirror (tests/nearest_reference.py), the automatic rule against its floating-point form, and
every layout's device block against what the kernels may touch in it."""

import math
import os
import shutil
import subprocess

import pytest

import nearest_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO, OA, CSR, HALVES = 0, 1, 2, 3
NAMES = {OA: "oa", CSR: "csr"}
NW = sorted({0, 1, 2, 3, 4, 5, 8, 9, 17, 300, 737280, 2 ** 31 - 1}
            | {2 ** k + d for k in range(2, 31) for d in (-1, 0, 1)})
TOUCH_LIMIT = 4 << 20


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("nearestindex") / "nearest_index_layout_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, os.path.join(ROOT, "tests", "host", "nearest_index_layout_check.cpp"), "-o", exe],
                   check=True)
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), check=True, capture_output=True, text=True,
                         timeout=300)
    got = out.stdout.splitlines()
    assert got[-1] == "ok %d limits %d %d %d" % (len(lines), R.MAX_PARTS, R.MAX_KEYS, R.GROUP), got[-1]
    return got[:-1]


def _cells():
    """(kind, code_bits, max_d): both kinds, every width, max_d 0..min(7, G - 1)."""
    for kind in (2, 3):
        for code_bits in range(1, 65):
            for max_d in range(0, min(7, R.positions(kind, code_bits) - 1) + 1):
                yield kind, code_bits, max_d


def _carve(line):
    """(the fields before the "|", segment offsets, total, touched)."""
    head, _, tail = line.partition(" | ")
    words = tail.split()
    assert words[-4] == "total" and words[-2] == "touched", line
    return head.split(), [int(w) for w in words[:-4]], int(words[-3]), int(words[-1])


def _check_block(case, offsets, total, touched, needs):
    """Segments 256-byte aligned, in order and disjoint, the total their end, and each at least as long as
    what the kernels may touch in it (and not a page longer)."""
    assert len(offsets) == len(needs) and offsets[0] == 0, case
    ends = offsets[1:] + [total]
    for off, end, need in zip(offsets, ends, needs):
        assert off % 256 == 0 and end % 256 == 0, (case, off, end)
        assert need <= end - off < need + 512, (case, off, end, need)  # (off < end: in order, disjoint)
    assert touched == (1 if total <= TOUCH_LIMIT else 0), (case, total)


def _float_rule(min_bases, nw):
    """The automatic rule as the build had it in floating point."""
    return 2.0 * min_bases >= math.log2(0.5 * max(nw, 2))


# ---------------------------------------------------------------- open addressing
def test_open_addressing_layout_is_the_mirrors(check_program):
    cases = [(kind, bits, max_d, nw) for kind, bits, max_d in _cells() for nw in NW]
    touched_some = False
    for case, line in zip(cases, _run(check_program, ["oa %d %d %d %d" % c for c in cases])):
        want = R.oa_layout(*case)
        if want is None:
            assert line == "none", case  # the plan cannot take open addressing
            continue
        head, offsets, total, touched = _carve(line)
        assert [int(w) for w in head[:5]] == [want["P"], len(want["keys"]), want["slots"], want["groups"],
                                              want["index_bytes"]], case
        keys = [w.split(":") for w in head[5:]]
        assert [(int(a), int(b)) for a, b, _ in keys] == want["keys"], case
        assert [int(m, 16) for _, _, m in keys] == want["keymasks"], case
        _check_block(case, offsets, total, touched, [16 * want["slots"]] * len(want["keys"]))
        touched_some |= bool(touched)
    assert touched_some


# ---------------------------------------------------------------- the choice
def test_builders_to_try(check_program):
    """Forced open addressing and CSR as the mirror expects them; the half keys first exactly under their
    static precondition (and never when another layout is forced); the automatic fallback open addressing
    where the plan can take it and the floating-point rule holds."""
    cases = [(kind, bits, max_d, nw, forced) for kind, bits, max_d in _cells() for nw in NW
             for forced in (AUTO, OA, CSR, HALVES)]
    can_oa = {cell: R.oa_layout(*cell, 0) is not None for cell in _cells()}
    for case, line in zip(cases, _run(check_program, ["scheme %d %d %d %d %d" % c for c in cases])):
        kind, bits, max_d, nw, forced = case
        got = [int(w) for w in line.split()]
        G = R.positions(kind, bits)
        halves = forced in (AUTO, HALVES) and max_d <= 1 and 2 <= G <= 16 and nw > 0
        assert got[:-1] == ([HALVES] if halves else []), case
        if forced in (OA, CSR):
            assert NAMES[got[-1]] == R.expected_scheme(NAMES[forced], kind, bits, max_d, nw), case
        else:
            min_bases = G if max_d == 0 else 2 * (G // (max_d + 2))
            assert got[-1] == (OA if can_oa[kind, bits, max_d] and _float_rule(min_bases, nw) else CSR), case


def test_automatic_rule_in_integers_is_the_float_rule(check_program):
    cases = sorted({(mb, 2 ** k + d) for mb in range(0, 33) for k in range(0, 31) for d in range(-3, 4)
                    if 0 <= 2 ** k + d < 2 ** 31})
    got = _run(check_program, ["auto %d %d" % c for c in cases])
    for case, line in zip(cases, got):
        assert int(line) == int(_float_rule(*case)), case


# ---------------------------------------------------------------- half keys
def test_half_key_arithmetic_and_block(check_program):
    cases = [(kind, bits, nw) for kind in (2, 3) for bits in range(1, 65) if 2 <= R.positions(kind, bits) <= 16
             for nw in NW if nw > 0]
    for case, line in zip(cases, _run(check_program, ["halves %d %d %d" % c for c in cases])):
        kind, bits, nw = case
        head, offsets, total, touched = _carve(line)
        GA, GB, pbits, ndw, index_bytes = (int(w) for w in head)
        G = R.positions(kind, bits)
        assert (GA, GB) == (G - G // 2, G // 2), case
        assert (pbits, ndw) == R.halves_packing(nw), case
        assert index_bytes == R.halves_index_bytes(kind, bits, nw), case
        # offA, offB | entA, entB: a 16-byte load starts at entry c + 8 j < nw | the packed permutation:
        # unpack_perm's 8-byte load at the dword of entry 2 nw - 1 | rankB
        packed = 4 * ((((2 * nw - 1) * pbits) >> 5) + 2)
        _check_block(case, offsets, total, touched,
                     [(4 ** GA + 1) * 4, (4 ** GB + 1) * 4, 2 * nw + 16, 2 * nw + 16, packed, nw])


# ---------------------------------------------------------------- CSR
def _csr_line(kind, bits, max_d, wl, load):
    occ = R.csr_occupied(kind, bits, max_d, wl)
    return "csr %d %d %d %d %d %s" % (kind, bits, max_d, len(wl), load, " ".join(str(o) for o in occ))


def _check_csr(case, line, want, nw):
    head, offsets, total, touched = _carve(line)
    assert int(head[1]) == want["index_bytes"], case
    parts = [w.split(":") for w in head[2:]]
    assert len(parts) == len(want["parts"]), case
    needs = []
    for (mask, lo_bit, nbits, mul, shift, buckets), part in zip(parts, want["parts"]):
        got = {"mask": int(mask, 16), "lo_bit": int(lo_bit), "mul": int(mul, 16), "shift": int(shift),
               "buckets": int(buckets)}
        assert got == part, (case, got, part)
        assert int(nbits) == bin(part["mask"]).count("1"), case
        needs += [(part["buckets"] + 1) * 4, 8 * nw, 4 * nw]
    _check_block(case, offsets, total, touched, [max(n, 1) for n in needs])


def test_csr_parts_on_the_width_whitelists(check_program):
    """The whitelists tests/test_gpu_nearest_layouts.py::test_every_width builds its plans from."""
    lines, wants = [], []
    for kind in (2, 3):
        cells = [kind * L for L in (range(1, 33) if kind == 2 else range(1, 22))]
        cells += (31, 63) if kind == 2 else (46, 47, 62, 63, 64)
        for bits in cells:
            wl, _, info = R.width_case(kind, bits, 300, 600)
            for max_d in range(0, min(3, info["G"] - 1) + 1):
                for load in (1, 4):
                    lines.append(_csr_line(kind, bits, max_d, wl, load))
                    wants.append(((kind, bits, max_d, load), R.csr_layout(kind, bits, max_d, wl.size, load, wl), wl.size))
    for line, (case, want, nw) in zip(_run(check_program, lines), wants):
        _check_csr(case, line, want, nw)


def test_csr_parts_on_the_heavy_bucket_whitelists(check_program):
    """The whitelists of test_csr_heavy_buckets: one block constant, 1..17 codes, max_d 0..7."""
    lines, wants = [], []
    for kind, L in ((2, 8), (3, 8), (2, 32), (3, 21)):
        for max_d in range(8):
            for nw in R.CSR_HEAVY_NW:
                for block in range(max_d + 1):
                    wl, _, info = R.csr_heavy_case(kind, L, max_d, nw, block)
                    for load in (1, 4):
                        lines.append(_csr_line(kind, kind * L, max_d, wl, load))
                        wants.append(((kind, L, max_d, nw, block, load), info[load]["layout"], nw))
    for line, (case, want, nw) in zip(_run(check_program, lines), wants):
        _check_csr(case, line, want, nw)


def test_csr_block_over_the_sweep(check_program):
    """The CSR block at every width and size, with the provisional bucket counts (no code occupies more)
    and with one occupied bucket per part (none occupies fewer)."""
    cases = [(kind, bits, max_d, nw, occ) for kind, bits, max_d in _cells() for nw in NW for occ in (0, 2 ** 31)]
    lines = ["csr %d %d %d %d 4 %s" % (kind, bits, max_d, nw, " ".join([str(occ)] * (max_d + 1)))
             for kind, bits, max_d, nw, occ in cases]
    for case, line in zip(cases, _run(check_program, lines)):
        kind, bits, max_d, nw, occ = case
        head, offsets, total, touched = _carve(line)
        lg0 = int(head[0])
        assert 2 ** lg0 * 2 >= min(nw, 2 ** 29) and (lg0 == 0 or 2 ** lg0 < nw), case
        buckets = [int(w.split(":")[5]) for w in head[2:]]
        assert buckets == [2 ** lg0 if occ else min(2 ** lg0, 4)] * (max_d + 1), case
        needs = []
        for b in buckets:
            needs += [(b + 1) * 4, max(8 * nw, 1), max(4 * nw, 1)]
        _check_block(case, offsets, total, touched, needs)
