"""The host entry points of the dosage container's lag calls (stormbitmaps_amd/csrc/storm_dosage_lag.c) as a stand-alone
program under AddressSanitizer, UBSan and LeakSanitizer: tests/host_sanitize/dosage_lag_driver.c on the common sources of
tests/_host_sanitize.py and dosage_lag_stub.c (the "device" is host memory and computes sample by sample). Outputs of exactly
n x L entries — a write outside the layout is a heap overflow there — and with a pitch, lags below, at and beyond n - 1,
every refusal, rows added between calls."""
import os
import shutil
import subprocess

import pytest

from tests._host_sanitize import ROOT, dosage_sources


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_lag_calls_under_asan_ubsan(tmp_path):
    exe = tmp_path / "dosage_lag_sanitize"
    srcs = dosage_sources(("storm_dosage_lag.c",), ("dosage_lag_stub.c", "dosage_lag_driver.c"))
    build = subprocess.run(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), *srcs,
                            "-o", str(exe), "-lm"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan not installed")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "dosage lag sanitize: ok" in run.stdout
