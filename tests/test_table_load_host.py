"""CPU, nothing loaded into Python: tests/host/table_load_check.cpp includes the header that holds the
limits and the feed policy of both counters' tables (sctools_amd/csrc/table_load.h) and runs its
feed loop -- the loop sct_counter_update and sct_molecules_update run -- over a simulated table.  It
is compiled by the host C++ compiler with AddressSanitizer and UBSan, and its lines are held against
the rule that keeps a probe from spinning: no launch ever leaves a table more than 3/4 full, the
size word is read before every growth, and capacities are powers of two within [64, 2^31]."""

import os
import re
import shutil
import subprocess
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_CAP, MAX_CAP = 64, 2 ** 31
ALL = 1_000_000  # parts per million: every item a new key


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("tableload") / "table_load_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, os.path.join(ROOT, "tests", "host", "table_load_check.cpp"), "-o", exe],
                   check=True)
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), check=True, capture_output=True, text=True,
                         timeout=120)
    got = out.stdout.splitlines()
    assert got[-1] == "ok %d limits %d %d" % (len(lines), MIN_CAP, MAX_CAP), got[-1]
    return got[:-1]


def _feeds(exe, cases):
    """Per (hint, n, ppm) case: (events, largest load, final capacity, status); an event is ("r",),
    ("g", capacity) or ("l", capacity, size after the launch)."""
    out = []
    for case, line in zip(cases, _run(exe, ["feed %d %d %d" % c for c in cases])):
        m = re.fullmatch(r"feed((?: \S+)*) max (\d+)/(\d+) end (\d+) (\d+)", line)
        assert m, (case, line)
        events = []
        for word in m.group(1).split():
            if word == "r":
                events.append(("r",))
            elif word[0] == "g":
                events.append(("g", int(word[1:])))
            else:
                cap, size = word[1:].split(":")
                events.append(("l", int(cap), int(size)))
        out.append((events, Fraction(int(m.group(2)), int(m.group(3))), int(m.group(4)), int(m.group(5))))
    return out


def _capacities(hint_capacity, events):
    return [hint_capacity] + [e[1] for e in events if e[0] == "g"]


def _check_rule(case, hint_capacity, events, largest, final, status):
    """The load rule on one feed's events."""
    cap = hint_capacity
    seen = Fraction(0)
    for k, e in enumerate(events):
        if e[0] == "g":
            assert events[k - 1] == ("r",) and k > 0, (case, k)  # a read of the size precedes every growth
            assert e[1] in (2 * cap, 4 * cap), (case, k, e)
            cap = e[1]
        elif e[0] == "l":
            assert e[1] == cap, (case, k, e)
            assert 4 * e[2] <= 3 * cap, (case, k, e)  # the load after the launch: at most 3/4
            seen = max(seen, Fraction(e[2], cap))
        assert cap & (cap - 1) == 0 and MIN_CAP <= cap <= MAX_CAP, (case, k, cap)
    assert largest == seen and largest <= Fraction(3, 4), (case, largest, seen)
    assert final == cap, (case, final, cap)
    if status == 0:
        assert any(e[0] == "l" for e in events) == (case[1] > 0), case


def _cap_for(hint):
    cap = MIN_CAP
    while cap < hint:
        cap *= 2
    return cap


def test_capacity_for_a_hint(check_program):
    hints = [0, 1, 64, 65, 2 ** 31]
    assert [int(x) for x in _run(check_program, ["cap %d" % h for h in hints])] == [64, 64, 64, 128, 2 ** 31]
    # every power of two and its neighbours: the smallest power of two at or above the hint, at least 64
    hints = sorted({h for b in range(0, 32) for h in (2 ** b - 1, 2 ** b, 2 ** b + 1) if h <= MAX_CAP})
    got = [int(x) for x in _run(check_program, ["cap %d" % h for h in hints])]
    for h, g in zip(hints, got):
        assert g & (g - 1) == 0 and MIN_CAP <= g <= MAX_CAP and g >= h and (g == MIN_CAP or g // 2 < h), (h, g)


def test_growth_past_two_to_the_31_is_refused(check_program):
    lines = ["grown %d %d" % (2 ** 30, 2), "grown %d %d" % (2 ** 30, 4), "grown %d %d" % (2 ** 31, 2),
             "grown %d %d" % (2 ** 31, 4), "grown %d %d" % (2 ** 29, 4), "grown 64 4", "grown 64 2"]
    assert [int(x) for x in _run(check_program, lines)] == [2 ** 31, 0, 0, 0, 2 ** 31, 256, 128]
    # a feed that needs more than 2^31 slots stops with a status at the growth, its table still within the rule
    cases = [(2 ** 31, 2 ** 31, ALL), (0, 2 ** 31, ALL), (2 ** 30, 2 ** 31, ALL)]
    for case, (events, largest, final, status) in zip(cases, _feeds(check_program, cases)):
        _check_rule(case, _cap_for(case[0]), events, largest, final, status)
        assert status != 0 and events[-1] == ("r",), (case, final, status)  # refused right after a read
    assert _feeds(check_program, cases[:1])[0][2] == MAX_CAP
    # and 2^30 distinct items, which 2^31 slots hold at a load of 1/2, go in
    (events, largest, final, status), = _feeds(check_program, [(0, 2 ** 30, ALL)])
    _check_rule((0, 2 ** 30, ALL), MIN_CAP, events, largest, final, status)
    assert status == 0 and events[-1][0] == "l" and events[-1][2] == 2 ** 30


def test_forced_growth_from_64_slots(check_program):
    """Hint 0 and 5,000 pairwise distinct items, by hand from the loop: sub-batches 16, 16, 16 | 64, 64 |
    256, 256 | 1024, 1024 | 2264, the capacity a merge plans for the same keys."""
    (events, largest, final, status), = _feeds(check_program, [(0, 5000, ALL)])
    assert status == 0
    assert _capacities(64, events) == [64, 256, 1024, 4096, 16384] and final == 16384
    sizes = [e[2] for e in events if e[0] == "l"]
    batches = [b - a for a, b in zip([0] + sizes, sizes)]
    assert batches == [16, 16, 16, 64, 64, 256, 256, 1024, 1024, 2264]
    assert largest == Fraction(3, 4)  # 48 of 64: the bound is reached, and never passed
    _check_rule((0, 5000, ALL), 64, events, largest, final, status)


def test_copies_of_one_item_never_grow(check_program):
    (events, largest, final, status), = _feeds(check_program, [(0, 5000, 0)])
    assert status == 0 and final == 64 and _capacities(64, events) == [64]
    assert sum(e[0] == "l" for e in events) == (5000 + 15) // 16  # sub-batches of capacity / 4
    assert largest == Fraction(1, 64)
    _check_rule((0, 5000, 0), 64, events, largest, final, status)


def test_load_rule_over_hints_sizes_and_shares(check_program):
    """Every hint capacity up to 2^20 against batch sizes at and around its quarter, half and multiples,
    with none, a few, half and all of the items new."""
    cases = []
    for b in range(6, 21, 2):
        cap = 2 ** b
        for n in sorted({0, 1, cap // 4 - 1, cap // 4, cap // 4 + 1, cap // 2, cap // 2 + 1, cap - 1, cap, 3 * cap + 1,
                         37 * cap + 5}):
            cases += [(cap, n, ppm) for ppm in (0, 1, 1000, 500_000, 999_999, ALL)]
    for case, (events, largest, final, status) in zip(cases, _feeds(check_program, cases)):
        assert status == 0, case
        _check_rule(case, case[0], events, largest, final, status)
        launches = [e for e in events if e[0] == "l"]
        if case[2] == ALL and launches:
            assert launches[-1][2] == case[1], case  # every item was fed and claimed a slot


def test_a_table_created_for_its_keys_never_grows(check_program):
    """A hint of at least twice the distinct keys: the bound never passes half, so the size is never read."""
    cases = [(10_000, 5000, ALL), (16384, 8192, ALL), (2 ** 31, 2 ** 30, ALL)]
    for case, (events, largest, final, status) in zip(cases, _feeds(check_program, cases)):
        _check_rule(case, _cap_for(case[0]), events, largest, final, status)
        assert status == 0 and final == _cap_for(case[0]) and all(e[0] == "l" for e in events), case
