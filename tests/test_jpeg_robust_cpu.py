"""CPU: csrc/jpeg.cpp, the parser of an untrusted upload, under AddressSanitizer + UndefinedBehaviorSanitizer.  tests/jpeg_robust/main.cpp
(a stand-alone program) is built together with the shipped source by g++ and run as an ordinary child process: every truncation
length and 2000 seeded single-byte corruptions of every synthetic stream of at most 2 KB.  The decoder must answer OK or an error
code every time and the sanitizers must stay silent."""
from __future__ import annotations

import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "chessvision-3lc_amd" / "csrc"


def test_jpeg_parser_survives_truncation_and_corruption_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed")
    z = np.load(ROOT / "tests" / "golden" / "jpeg_cases.npz")
    streams = [z[f"blob/{n}"].tobytes() for n, k in zip(z["names"], z["kind"]) if not str(n).startswith("truncated")]
    streams = [s for s in streams if len(s) <= 2048]
    assert len(streams) >= 150
    with open(tmp_path / "streams.bin", "wb") as f:
        for s in streams:
            f.write(struct.pack("<I", len(s)) + s)
    exe = tmp_path / "jpeg_robust"
    out = subprocess.run([gxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                          "-static-libasan", "-static-libubsan", "-pthread", f"-I{CSRC}", str(ROOT / "tests" / "jpeg_robust" / "main.cpp"), str(CSRC / "jpeg.cpp"), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0 and ("libasan" in out.stderr or "libubsan" in out.stderr):
        pytest.skip("g++ has no sanitizer runtime on this machine")
    assert out.returncode == 0, out.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(tmp_path / "streams.bin")], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-4000:])
    assert "jpeg robust: ok" in run.stdout and f"streams: {len(streams)}" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    calls = int(run.stdout.split("calls: ")[1].split()[0])
    assert calls >= sum(len(s) + 1 + 2000 for s in streams)
