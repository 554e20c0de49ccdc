"""CPU, nothing loaded into Python: tests/host/read_group_status_check.cpp includes the read-groups
header (sctools_amd/csrc/read_group_status.h: the status precedence and the per-slot word), is compiled
by the host C++ compiler with AddressSanitizer and UBSan, and checks the precedence over every
combination of its inputs and the word's round trip at the extreme UMI widths of both kinds."""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_status_precedence_and_slot_word(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "read_group_status_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, os.path.join(ROOT, "tests", "host", "read_group_status_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120)
    # 3 nw x 4 nf x (6 x 6 index-feature pairs, less those an int32 cannot hold) x 8 x 2; 4 widths x 6 x 2 x 3
    pairs = sum(sum(1 for i in (-3, -2, -1, 0, nw - 1, nw) for f in (-3, -2, -1, 0, nf - 1, nf)
                    if i < 2 ** 31 and f < 2 ** 31)
                for nw in (1, 5, 2 ** 31 - 1) for nf in (0, 1, 6, 2 ** 31 - 1))
    assert out.stdout.split() == ["ok", str(pairs * 16 + 4 * 6 * 2 * 3)], out.stdout + out.stderr
