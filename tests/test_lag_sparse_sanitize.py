"""The host entry points of the dosage container's sparse LD report (stormbitmaps_amd/csrc/storm_dosage_lag_sparse.c and the
planner storm_ldscore_window.c) as a stand-alone program under AddressSanitizer, UBSan and LeakSanitizer:
tests/host_sanitize/dosage_lag_sparse_driver.c on the common sources of tests/_host_sanitize.py and a stub of its own
(dosage_lag_sparse_stub.c: the "device" is host memory listing the pairs sample by sample). row_start of exactly n + 1 and
col / val of exactly `total` elements — a write behind them is a heap overflow there — a capacity of total - 1, the count-only
call, windows that need exactly max_lag rows and one row more, every refusal. Nothing is loaded into Python under a sanitizer:
the program is its own executable."""
import os
import shutil
import subprocess

import pytest

from tests._host_sanitize import CSRC, ROOT, dosage_sources


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_sparse_calls_under_asan_ubsan(tmp_path):
    exe = tmp_path / "dosage_lag_sparse_sanitize"
    srcs = dosage_sources(("storm_dosage_lag_sparse.c",), ("dosage_lag_sparse_stub.c", "dosage_lag_sparse_driver.c"))
    build = subprocess.run(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, *srcs,
                            "-o", str(exe), "-lm"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan not installed")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "dosage lag sparse sanitize: ok" in run.stdout
