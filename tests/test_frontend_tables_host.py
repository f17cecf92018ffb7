"""The host-only table builders of the front ends (csrc/frontend_tables.h: windows, twiddles, DFT rows, Slaney and HTK filterbanks, the
compact filter form) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program on the CPU
(tools/frontend_tables_check.cpp).  The program checks the rules the kernels rely on itself; the tables it writes are compared here
with the oracle's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import campplus as OC
from oracle import logmel as OL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Largest |table - oracle| of the builders this header replaced, measured once on their tables before they were deleted, times 4
# (the oracle evaluates the same fp32 expressions through numpy, whose cos / log / exp may round another way):
#   windows      5.96e-8  (Whisper Hann, periodic Hann and Povey alike: one ulp below 1)
#   filterbanks  2.20e-7  (log-mel 128; log-mel 80: 4.8e-8, S3Gen: 6.3e-8, CAM++: 0)
WINDOW_ATOL = 2.4e-7
FILTER_ATOL = 8.8e-7
# Both sides are within one double ulp of the exactly reduced angle's cos / sin before the rounding to fp32: at most one fp32 ulp apart
# at a magnitude <= 1.  (The replaced builders showed 0.)
TWIDDLE_ATOL = 1.2e-7
# Filters whose (first bin, count) may differ from the oracle's non-zero support by one bin, where a triangle's edge lands on a bin:
# none did on the replaced builders' tables, so none may.
SUPPORT_OFF_BY_ONE = 0


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cxx = next((c for c in ("clang++", "g++", "c++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("frontend_tables")
    exe, out = str(tmp / "frontend_tables_check"), str(tmp / "tables.bin")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "frontend_tables_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    t = {}
    with open(out, "rb") as f:
        for line in iter(f.readline, b""):
            name, kind, n = line.decode().split()
            t[name] = np.frombuffer(f.read(4 * int(n)), {"f32": np.float32, "i32": np.int32}[kind])
            assert t[name].size == int(n)
    return t


def test_windows(tables):
    for name, want in (("logmel_win0", OL.whisper_hann_window(400)), ("logmel_win1", OL.periodic_hann_window(400)), ("cam_win", OC.povey_window(400))):
        d = np.abs(tables[name] - want).max()
        print(name, d)
        assert tables[name].shape == want.shape and d <= WINDOW_ATOL, (name, d)
    assert np.abs(tables["s3gen_dft"][:1920] - OL.periodic_hann_window(1920)).max() <= WINDOW_ATOL      # bin 0's cosine row is the window


@pytest.mark.parametrize("front, live", [("logmel", 201), ("funasr", 200)])
def test_twiddles(tables, front, live):
    tw = tables[front + "_tw"].reshape(400, 2, 224)
    k, j = np.arange(400)[:, None], np.arange(live)[None, :]
    ang = 2.0 * np.pi * ((k * j) % 400).astype(np.float64) / 400.0
    dc, ds = np.abs(tw[:, 0, :live] - np.cos(ang).astype(np.float32)).max(), np.abs(tw[:, 1, :live] - np.sin(ang).astype(np.float32)).max()
    print(front, dc, ds)
    assert dc <= TWIDDLE_ATOL and ds <= TWIDDLE_ATOL
    assert not tw[:, :, live:].any()


def _support(ref):
    """(first bin, count) of each row's non-zero support; (0, 0) for an all-zero row, like the compact form."""
    nz = ref != 0
    first = np.where(nz.any(1), nz.argmax(1), 0)
    last = np.where(nz.any(1), ref.shape[1] - 1 - nz[:, ::-1].argmax(1), -1)
    return first, last - first + 1


@pytest.mark.parametrize("name, suffix, ref", [
    ("logmel", "80", lambda: OL.mel_filters(16000, 400, 80)),
    ("logmel", "128", lambda: OL.mel_filters(16000, 400, 128)),
    ("s3gen", "", lambda: OL.mel_filters(24000, 1920, 80, 0.0, 8000.0)),
    ("cam", "", lambda: OC.mel_filters_htk(16000, 512, 80, 20.0, 8000.0).T),
])
def test_filterbanks(tables, name, suffix, ref):
    want = ref()
    dense = tables[f"{name}_dense{suffix}"].reshape(want.shape)
    d = np.abs(dense - want).max()
    print(name + suffix, d)
    assert d <= FILTER_ATOL, d
    meta = tables[f"{name}_meta{suffix}"].reshape(-1, 3)
    first, count = _support(want)
    off = (meta[:, 0] != first) | (meta[:, 1] != count)
    assert (np.abs(meta[:, 0] - first) <= 1).all() and (np.abs(meta[:, 1] - count) <= 1).all()
    assert int(off.sum()) <= SUPPORT_OFF_BY_ONE, np.flatnonzero(off)
    # the compact weights are the dense rows' supports back to back
    w = tables[f"{name}_w{suffix}"]
    rows = [dense[m, lo:lo + n] for m, (lo, n, _) in enumerate(meta)]
    assert np.array_equal(meta[:, 2], np.cumsum([0] + [len(r) for r in rows[:-1]])) and np.array_equal(w, np.concatenate(rows))


def test_s3gen_transform_stops_at_8khz(tables):
    assert int(tables["s3gen_nbp"][0]) == 672 and tables["s3gen_dft"].size == 2 * 672 * 1920
