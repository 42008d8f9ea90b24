"""The host side of the dosage container (storm.h: STORM_dosage_*) without a GPU: the 2-bit packing, every refusal code,
and — no CPU fallback — compute calls that fail with a reason when no device is visible. What the device computes is
tests/test_gpu_dosage.py's."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import stormbitmaps_amd as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pack(values, n_samples):
    """numpy restatement of the layout: sample s in bits 2 (s % 32), 2 (s % 32) + 1 of word s / 32"""
    v = np.zeros(((n_samples + 31) // 32) * 32, dtype=np.uint64)
    v[:n_samples] = values
    return (v.reshape(-1, 32) << (np.arange(32, dtype=np.uint64) * np.uint64(2))).sum(axis=1, dtype=np.uint64)


@pytest.mark.parametrize("n_samples", [1, 31, 32, 33, 64, 1000])
def test_add_packs_exactly_as_add_packed_expects(lib, n_samples):
    """rows through STORM_dosage_add, and the same rows packed by the numpy restatement of the layout through
    STORM_dosage_add_packed (accepted: their tail bits are zero); the words themselves are compared in the stand-alone
    program below"""
    rng = np.random.default_rng(n_samples)
    rows = rng.integers(0, 4, size=(5, n_samples), dtype=np.uint8)
    rows[0, :] = 3                                   # every bit of the row set: any tail spill would show
    packed = np.stack([pack(r, n_samples) for r in rows])
    assert packed.shape == (5, (n_samples + 31) // 32)
    # the layout by hand for one sample
    s = n_samples - 1
    assert (int(packed[1, s // 32]) >> (2 * (s % 32))) & 3 == int(rows[1, s])
    a, b = lib.STORM_dosage_new(n_samples), lib.STORM_dosage_new(n_samples)
    for r in rows:
        assert lib.STORM_dosage_add(a, r.ctypes.data, n_samples) == 0
    assert lib.STORM_dosage_add_packed(b, packed.ctypes.data, 5) == 0          # tail bits zero: accepted
    assert lib.STORM_dosage_n_rows(a) == lib.STORM_dosage_n_rows(b) == 5
    lib.STORM_dosage_free(a)
    lib.STORM_dosage_free(b)


def test_tail_bits_of_packed_rows_are_refused_bit_by_bit(lib):
    """every bit beyond the last sample of a packed row is refused (-3, nothing appended); the full row is accepted"""
    for n_samples in (1, 5, 31, 33, 63):
        h = lib.STORM_dosage_new(n_samples)
        n_words = (n_samples + 31) // 32
        good = pack(np.full(n_samples, 3, dtype=np.uint8), n_samples)
        assert lib.STORM_dosage_add_packed(h, good.ctypes.data, 1) == 0
        for bit in range(2 * (n_samples % 32), 64):
            bad = good.copy()
            bad[n_words - 1] |= np.uint64(1) << np.uint64(bit)
            assert lib.STORM_dosage_add_packed(h, bad.ctypes.data, 1) == -3, (n_samples, bit)
            assert b"beyond sample" in lib.STORM_hip_error()
        assert lib.STORM_dosage_n_rows(h) == 1
        lib.STORM_dosage_free(h)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_add_against_add_packed_word_for_word_under_asan_ubsan(tmp_path):
    """The words STORM_dosage_add packs against the words STORM_dosage_add_packed is given, as they reach the device
    (tests/host_sanitize/dosage_driver.c on the device stub: the upload's destination is host memory there), word for word
    and against the layout; growth, refusals, clear and free along the way. A stand-alone program under AddressSanitizer,
    UBSan and LeakSanitizer: the host side of the container (storm_dosage.c and storm_dosage_pairs.c on storm_host.c's locked
    paths; the calls the driver does not answer itself are dosage_pairs_stub.c's and dosage_band_stub.c's)."""
    exe = tmp_path / "dosage_sanitize"
    csrc = os.path.join(ROOT, "stormbitmaps_amd", "csrc")
    srcs = [os.path.join(csrc, f) for f in ("storm_host.c", "storm_host_call.c", "storm_dosage.c", "storm_dosage_pairs.c",
                                            "storm_synth.c", "storm_leaves.c")] + \
           [os.path.join(ROOT, "tests", "host_sanitize", f) for f in ("device_stub.c", "dosage_pairs_stub.c", "dosage_band_stub.c",
                                                                      "dosage_driver.c")]
    build = subprocess.run(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), *srcs,
                            "-o", str(exe), "-lm"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan not installed")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "dosage sanitize: ok" in run.stdout


def test_new_refuses_zero_and_more_than_2_pow_24_samples(lib):
    assert not lib.STORM_dosage_new(0)
    assert not lib.STORM_dosage_new((1 << 24) + 1)
    assert not lib.STORM_dosage_new(1 << 40)
    for n in (1, 1 << 24):
        h = lib.STORM_dosage_new(n)
        assert h
        lib.STORM_dosage_free(h)
    lib.STORM_dosage_free(None)


def test_every_refusal_code(lib):
    S = 40
    h = lib.STORM_dosage_new(S)
    good = np.arange(S, dtype=np.uint8) % 4
    out = np.zeros((4, 4), dtype=np.uint32)
    fout = np.zeros((4, 4), dtype=np.float32)
    sums = np.zeros(4, dtype=np.uint32)
    # NULL handle: -1
    assert lib.STORM_dosage_add(None, good.ctypes.data, S) == -1
    assert lib.STORM_dosage_add_packed(None, good.ctypes.data, 1) == -1
    assert lib.STORM_dosage_clear(None) == -1
    assert lib.STORM_dosage_n_rows(None) == 0
    assert lib.STORM_dosage_row_sums(None, sums.ctypes.data, sums.ctypes.data) == -1
    assert lib.STORM_dosage_pairw_dot(None, out.ctypes.data, 4, 4) == -1
    assert lib.STORM_dosage_pairw_dot_device(None, out.ctypes.data, 4, 4) == -1
    assert lib.STORM_dosage_pairw_corr(None, 0, fout.ctypes.data, 4, 4) == -1
    assert lib.STORM_dosage_pairw_corr_device(None, 0, fout.ctypes.data, 4, 4) == -1
    # NULL values / out: -2
    assert lib.STORM_dosage_add(h, None, S) == -2
    assert lib.STORM_dosage_add_packed(h, None, 1) == -2
    assert lib.STORM_dosage_row_sums(h, None, sums.ctypes.data) == -2
    assert lib.STORM_dosage_row_sums(h, sums.ctypes.data, None) == -2
    assert lib.STORM_dosage_pairw_dot(h, None, 4, 4) == -2
    assert lib.STORM_dosage_pairw_dot_device(h, None, 4, 4) == -2
    assert lib.STORM_dosage_pairw_corr(h, 0, None, 4, 4) == -2
    assert lib.STORM_dosage_pairw_corr_device(h, 1, None, 4, 4) == -2
    # bad rows: -3, nothing appended
    assert lib.STORM_dosage_add(h, good.ctypes.data, S - 1) == -3 and b"samples" in lib.STORM_hip_error()
    assert lib.STORM_dosage_add(h, good.ctypes.data, S + 1) == -3
    bad = good.copy()
    bad[S - 1] = 4
    assert lib.STORM_dosage_add(h, bad.ctypes.data, S) == -3 and b"value 4 at sample 39" in lib.STORM_hip_error()
    bad[S - 1] = 255
    assert lib.STORM_dosage_add(h, bad.ctypes.data, S) == -3
    assert lib.STORM_dosage_n_rows(h) == 0
    # fewer than two rows: 0, nothing written (no device is needed)
    out[:] = 77
    assert lib.STORM_dosage_pairw_dot(h, out.ctypes.data, 4, 4) == 0
    assert lib.STORM_dosage_add(h, good.ctypes.data, S) == 0
    assert lib.STORM_dosage_pairw_dot(h, out.ctypes.data, 4, 4) == 0
    assert lib.STORM_dosage_pairw_corr(h, 1, fout.ctypes.data, 4, 4) == 0
    assert (out == 77).all() and (fout == 0).all()
    # too small an output: -4, nothing written
    for _ in range(4):
        assert lib.STORM_dosage_add(h, good.ctypes.data, S) == 0
    assert lib.STORM_dosage_n_rows(h) == 5
    assert lib.STORM_dosage_pairw_dot(h, out.ctypes.data, 4, 8) == -4
    assert lib.STORM_dosage_pairw_dot(h, out.ctypes.data, 8, 4) == -4
    assert lib.STORM_dosage_pairw_dot_device(h, out.ctypes.data, 4, 4) == -4
    assert lib.STORM_dosage_pairw_corr(h, 0, fout.ctypes.data, 4, 4) == -4
    assert lib.STORM_dosage_pairw_corr_device(h, 0, fout.ctypes.data, 5, 4) == -4
    assert (out == 77).all() and (fout == 0).all()
    # an unknown measure: -3, before any device is asked for
    big = np.zeros((5, 5), dtype=np.float32)
    for measure in (2, -1, 99):
        assert lib.STORM_dosage_pairw_corr(h, measure, big.ctypes.data, 5, 5) == -3
        assert b"measure" in lib.STORM_hip_error()
    assert lib.STORM_dosage_clear(h) == 0 and lib.STORM_dosage_n_rows(h) == 0
    lib.STORM_dosage_free(h)


def test_no_cpu_fallback_without_device(lib):
    if lib.storm_hip_device_count() != 0:
        pytest.skip("a GPU is visible; the loud-failure path is exercised on the CPU container")
    S, n = 100, 3
    h = lib.STORM_dosage_new(S)
    rng = np.random.default_rng(1)
    for _ in range(n):
        r = rng.integers(0, 3, size=S, dtype=np.uint8)
        assert lib.STORM_dosage_add(h, r.ctypes.data, S) == 0
    out = np.full((n, n), 77, dtype=np.uint32)
    fout = np.full((n, n), 7.0, dtype=np.float32)
    sums = np.full(n, 77, dtype=np.uint32)
    assert lib.STORM_dosage_pairw_dot(h, out.ctypes.data, n, n) == -3
    assert lib.STORM_hip_error()
    assert lib.STORM_dosage_pairw_corr(h, 0, fout.ctypes.data, n, n) == -3
    assert lib.STORM_dosage_pairw_corr(h, 1, fout.ctypes.data, n, n) == -3
    assert lib.STORM_dosage_row_sums(h, sums.ctypes.data, sums.ctypes.data) == -3
    assert b"no CPU fallback" in lib.STORM_hip_error() or lib.STORM_hip_error()
    assert (out == 77).all() and (fout == 7.0).all() and (sums == 77).all()
    lib.STORM_dosage_free(h)
    with pytest.raises(ValueError):
        sb.StormDosage(0)
    d = sb.StormDosage(S)
    d.add(np.zeros(S, dtype=np.uint8))
    d.add(np.ones(S, dtype=np.uint8))
    with pytest.raises(RuntimeError):
        d.pairw_dot()
    with pytest.raises(RuntimeError):
        d.add(np.full(S, 4, dtype=np.uint8))
    assert d.n_rows == 2
