"""CPU, nothing loaded into Python: tests/host/molecules_merge_plan_check.cpp includes the header that
gives sct_molecules_merge its growth target (sctools_amd/csrc/molecules_merge_plan.h), is compiled by
the host C++ compiler with AddressSanitizer and UBSan, and its answers are held against the contract
(include/sctools_hip.h, "merging molecule counters"): the target keeps dst.nmolecules +
src.nmolecules <= capacity / 2, is a power of two, is never smaller than dst's capacity, is the
smallest such, and does not exist exactly when it would pass 2^31 slots."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_CAP, MAX_CAP = 64, 2 ** 31
CAPACITIES = [2 ** b for b in range(6, 32)]


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("molmerge") / "molecules_merge_plan_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, os.path.join(ROOT, "tests", "host", "molecules_merge_plan_check.cpp"), "-o", exe],
                   check=True)
    return exe


def _run(exe, cases):
    text = "".join("%d %d %d\n" % c for c in cases)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True, timeout=120)
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok %d limits %d %d" % (len(cases), MIN_CAP, MAX_CAP), lines[-1]
    return [int(ln) for ln in lines[:-1]]


def _check(case, got):
    cap, dst_size, src_size = case
    keys = dst_size + src_size
    if 2 * keys > MAX_CAP:  # a load of 1/2 would take more than 2^31 slots
        assert got == 0, (case, got)
        return
    assert got != 0, (case, got)
    assert got & (got - 1) == 0 and MIN_CAP <= got <= MAX_CAP, (case, got)  # a power of two within the limits
    assert got >= cap, (case, got)  # a merge never shrinks the table
    assert keys <= got // 2, (case, got)  # the load bound
    assert got == cap or keys > got // 4, (case, got)  # and no doubling more than the bound asks for


def _splits(cap, keys):
    """(dst_size, src_size) pairs that sum to `keys`, dst_size within dst's own capacity."""
    out = {(0, keys), (min(keys, cap // 2), keys - min(keys, cap // 2)), (min(keys, cap), keys - min(keys, cap)),
           (min(keys, 1), keys - min(keys, 1)), (min(keys, cap // 4 + 1), keys - min(keys, cap // 4 + 1))}
    return sorted(out)


def test_sizes_at_and_around_half_of_every_capacity(check_program):
    """Every dst capacity 64 .. 2^31 against sums at, one below and one above half of every capacity
    from its own up to 2^31 (the thresholds between one target and the next), and 0 and 1."""
    cases = []
    for cap in CAPACITIES:
        sums = {0, 1}
        for target in CAPACITIES:
            if target >= cap:
                sums |= {target // 2 - 1, target // 2, target // 2 + 1, target // 4 + 1}
        for keys in sorted(sums):
            cases += [(cap, d, s) for d, s in _splits(cap, keys)]
    got = _run(check_program, cases)
    for case, g in zip(cases, got):
        _check(case, g)
    # the table stays when the keys fit it, and doubles exactly one key later
    by_case = dict(zip(cases, got))
    for cap in CAPACITIES:
        assert by_case[(cap, 0, cap // 2)] == cap
        assert by_case[(cap, 0, cap // 2 + 1)] == (2 * cap if cap < MAX_CAP else 0)


def test_does_not_fit_exactly_above_two_to_the_31(check_program):
    """2^30 keys fit (2^31 slots at a load of 1/2), 2^30 + 1 do not, whatever dst's capacity and
    however the keys are split between the two counters; nor do the largest sizes two tables can have."""
    cases = []
    for cap in CAPACITIES:
        for keys in (2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, 2 ** 30 + cap, 2 ** 31, 2 ** 32):
            cases += [(cap, d, keys - d) for d in sorted({0, min(cap, keys), min(cap // 2, keys), 1})]
    got = _run(check_program, cases)
    for case, g in zip(cases, got):
        _check(case, g)
        assert (g == 0) == (case[1] + case[2] > 2 ** 30), (case, g)
        assert g in (0, MAX_CAP), (case, g)


def test_growth_of_a_small_table_by_a_large_source(check_program):
    """The GPU growth test's shape and its neighbours: 64 slots and 10 molecules taking in about 5,000
    grows by at least four doublings in one step, to the capacity an update would have reached."""
    cases = [(64, 10, n) for n in (0, 22, 23, 54, 55, 4000, 5000, 5010, 8182, 8183)]
    got = _run(check_program, cases)
    assert got == [64, 64, 128, 128, 256, 8192, 16384, 16384, 16384, 32768]
    for case, g in zip(cases, got):
        _check(case, g)
