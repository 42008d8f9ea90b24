"""The host entry points of the dosage container's rectangle and of its calls for rows with missing genotypes
(stormbitmaps_amd/csrc/storm_dosage_pairs.c, and STORM_dosage_row_missing in storm_dosage.c) as a stand-alone program under
AddressSanitizer, UBSan and LeakSanitizer: tests/host_sanitize/dosage_complete_driver.c on device_stub.c, dosage_complete_stub.c
and dosage_pairs_stub.c (the "device" is host memory and computes sample by sample). Two containers, outputs with a pitch, every refusal, rows added between calls."""
import os
import shutil
import subprocess

import pytest

from tests._host_sanitize import ROOT, dosage_sources


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_rectangle_and_missing_genotype_calls_under_asan_ubsan(tmp_path):
    exe = tmp_path / "dosage_complete_sanitize"
    srcs = dosage_sources(("storm_dosage_pairs.c",), ("dosage_complete_driver.c",))
    build = subprocess.run(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), *srcs,
                            "-o", str(exe), "-lm"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan not installed")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "dosage complete sanitize: ok" in run.stdout
