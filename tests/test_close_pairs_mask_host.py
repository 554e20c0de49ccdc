"""CPU, nothing loaded into Python: tests/host/close_pairs_mask_check.cpp includes the close-pairs
header (sctools_amd/csrc/close_pairs_mask.h: the bit-sliced "distance <= t", the distance read back
from the planes, the sort word), is compiled by the host C++ compiler with AddressSanitizer and
UBSan, and checks the comparison exhaustively against plain integer compare: every B in 1..6, every
t in 0..3, every distance 0..2^B - 1 in every bit position."""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mask_distance_and_sort_word_exhaustively(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "close_pairs_mask_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, os.path.join(ROOT, "tests", "host", "close_pairs_mask_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120)
    # per B: 4^B (background, distance) x 32 positions x (4 thresholds + 32 read-backs); then the
    # sort word: 66 index pairs x 4 distances and 12 end bits
    planes = sum(4 ** b * 32 * (4 + 32) for b in range(1, 7))
    assert out.stdout.split() == ["ok", str(planes + 66 * 4 + 12)], out.stdout + out.stderr
