"""The host arithmetic behind the chunked host pipeline (host_items in sctools_amd/csrc/encode_host.cpp:
the encode stream and the large element-wise calls on host arrays), without a GPU and without Python
in the process under test: tests/host/host_pipeline_check.cpp checks the two chunk policies and
sct::StageLayout of sctools_amd/csrc/host_pipeline.h, compiled with AddressSanitizer and UBSan and
run on its own."""

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunking_and_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "host_pipeline_check")
    # the sanitizer runtimes linked into the program itself: it needs nothing from its environment
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.realpath(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static, os.path.join(ROOT, "tests", "host", "host_pipeline_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120)
    assert "ok" in out.stdout
