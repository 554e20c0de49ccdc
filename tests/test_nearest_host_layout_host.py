"""The host arithmetic behind the nearest *_host entry points, without a GPU and without Python in
the process under test: tests/host/nearest_host_layout_check.cpp exercises sct::NearestLayout (the
pool block of all four forms) and sct::PoolBlock (free, one synchronisation and the error merge on
every path) against a stub pool, compiled with AddressSanitizer and UBSan and run on its own."""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_and_guard_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "nearest_host_layout_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tests", "host", "nearest_host_layout_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120)
    assert "ok" in out.stdout
