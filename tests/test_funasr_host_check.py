"""The host-only code of Fun-ASR's audio half (csrc/funasr_host.h: window and filterbank builders, compact filter form, length and shape
rules) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program on the CPU (tools/funasr_host_check.cpp), and the
device's filterbank table against the frozen facts of tests/golden/funasr_fbank.npz."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_tables_and_rules_under_sanitizers(tmp_path):
    cxx = next((c for c in ("clang++", "g++", "c++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "funasr_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "funasr_host_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(l.split(":", 1) for l in r.stdout.splitlines() if ":" in l)
    g = np.load(os.path.join(ROOT, "tests", "golden", "funasr_fbank.npz"))
    first, last = (np.array(lines[k].split(), np.int64) for k in ("first", "last"))
    assert np.array_equal(first, g["first"])
    # the table keeps every non-zero float; the frozen `last` counts weights above 1e-9: the two may differ only where an edge meets a bin
    assert (np.abs(last - g["last"]) <= 1).all() and (last == g["last"]).sum() >= 78
    assert r.stdout.strip().endswith("ok")
