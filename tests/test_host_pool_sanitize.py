"""The worker pool of the host side (storm_host.c: pool_main / run_on_devices — one thread per device slot beyond the first,
the default of every all-pairs call on a node with several different GPUs) on the device stub, under ThreadSanitizer.

tests/host_sanitize/pool.c is a stand-alone program with the sanitizer linked in; nothing is preloaded. It is built the way
test_host_sanitize.py builds threads.c and started twice, one process per value of STORM_HIP_HOST_THREADS as a job would
have it: once with the pool forced on (the same ordinal three times would keep it off), once with it off. The program asserts the
totals, which thread launched each slot's shard, the recovery after a launch that fails (a return code from the stub) and
that a worker outside the configured slots stays parked; this file asserts what only a parent sees: exit status, a clean
sanitizer report and the stderr line that names the failing slot."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pool_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    exe = tmp_path_factory.mktemp("pool") / "host_pool"
    srcs = [os.path.join(ROOT, "stormbitmaps_amd", "csrc", "storm_host.c"),
            os.path.join(ROOT, "stormbitmaps_amd", "csrc", "storm_synth.c"),
            os.path.join(ROOT, "stormbitmaps_amd", "csrc", "storm_leaves.c"),
            os.path.join(ROOT, "tests", "host_sanitize", "device_stub.c"),
            os.path.join(ROOT, "tests", "host_sanitize", "pool.c")]
    build = subprocess.run(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=thread", "-pthread",
                            "-I" + os.path.join(ROOT, "include"), *srcs, "-o", str(exe), "-lm", "-ldl"],
                           capture_output=True, text=True)
    if build.returncode != 0 and "tsan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libtsan not installed")
    assert build.returncode == 0, build.stderr
    return str(exe)


def _run(exe, mode):
    # gcc's TSan runtime expects the address layout of a kernel with few ASLR bits and aborts at start-up
    # ("unexpected memory mapping") under more: the child alone runs with randomisation off (setarch -R)
    no_aslr = ["setarch", platform.machine(), "-R"]
    if shutil.which("setarch") is None or subprocess.run(no_aslr + ["true"], capture_output=True).returncode != 0:
        no_aslr = []
    env = {k: v for k, v in os.environ.items() if not k.startswith("STORM_HIP_")}
    env["TSAN_OPTIONS"] = "halt_on_error=1:exitcode=66"
    run = subprocess.run(no_aslr + [exe, mode], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "ThreadSanitizer" not in run.stderr
    return run


def _after(stderr, marker):
    """the stderr lines between `marker` and the next injection"""
    tail = stderr.split(marker + "\n", 1)
    assert len(tail) == 2, stderr[-2000:]
    return tail[1].split("-- injected", 1)[0]


def test_worker_pool_drives_the_other_slots_and_survives_a_failed_launch(pool_exe):
    run = _run(pool_exe, "1")
    assert "pool ok (host threads on)" in run.stdout
    # a worker's failure is reported with its slot, the caller's own without one
    for what, name in (("all-pairs pass (dense)", "contig"), ("all-pairs pass (STORM_t)", "STORM_t")):
        worker = _after(run.stderr, "-- injected: %s, slot 2" % name)
        assert "[storm_hip] %s (device slot 2): stub: injected launch failure" % what in worker, run.stderr[-2000:]
        caller = _after(run.stderr, "-- injected: %s, slot 0" % name)
        assert "[storm_hip] %s: stub: injected launch failure" % what in caller, run.stderr[-2000:]
        assert "device slot" not in caller


def test_host_threads_0_keeps_every_slot_on_the_callers_thread(pool_exe):
    run = _run(pool_exe, "0")
    assert "pool ok (host threads off)" in run.stdout
    assert "device slot" not in run.stderr   # (one thread: the failure is the caller's own)
    assert run.stderr.count("stub: injected launch failure") == 4


# ------------------------------------------------------------------------------------------ the environment's configuration
@pytest.fixture(scope="module")
def env_exe(tmp_path_factory):
    """tests/host_sanitize/env_config.c under AddressSanitizer + UBSan, as test_host_sanitize.py builds driver.c"""
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    exe = tmp_path_factory.mktemp("env") / "host_env"
    srcs = [os.path.join(ROOT, "stormbitmaps_amd", "csrc", "storm_host.c"),
            os.path.join(ROOT, "stormbitmaps_amd", "csrc", "storm_synth.c"),
            os.path.join(ROOT, "stormbitmaps_amd", "csrc", "storm_leaves.c"),
            os.path.join(ROOT, "tests", "host_sanitize", "device_stub.c"),
            os.path.join(ROOT, "tests", "host_sanitize", "env_config.c")]
    build = subprocess.run(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), *srcs,
                            "-o", str(exe), "-lm"], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan not installed")
    assert build.returncode == 0, build.stderr
    return str(exe)


def _configured(exe, **env):
    full = {k: v for k, v in os.environ.items() if not k.startswith("STORM_HIP_")}
    full.update(env, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=full, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    return run.stdout.strip(), run.stderr


SIXTEEN_SLOTS = ",".join(str(d) for d in range(16))


@pytest.mark.parametrize("value, slots", [(None, 1), ("", 1), ("all", 1), ("0", 1), ("0,0,0", 3), ("2,0", 2), ("-1", 1), ("99", 1),
                                          (SIXTEEN_SLOTS, 16)])
def test_devices_as_documented(env_exe, value, slots):
    """(the stub has one device and takes any ordinal: what a number that names no device does is a GPU test)"""
    out, err = _configured(env_exe, **({} if value is None else {"STORM_HIP_DEVICES": value}))
    assert out == "slots=%d total=whole" % slots and "STORM_HIP_DEVICES" not in err


@pytest.mark.parametrize("value", ["0,x", "x", "0,,1", "0,", ",0", " 0", "+1", "0 ,1", "1.5", "0x1", "3000000000", SIXTEEN_SLOTS + ",16"])
def test_malformed_devices_is_one_line_and_device_0_alone(env_exe, value):
    """strtol stood still on the first character it did not like: `0,x` configured sixteen slots of device 0, silently"""
    out, err = _configured(env_exe, STORM_HIP_DEVICES=value)
    assert out == "slots=1 total=whole"
    assert err.count('libstorm_hip: STORM_HIP_DEVICES: "%s" ignored' % value) == 1 and "device 0 alone" in err, err


@pytest.mark.parametrize("value, total", [("0/3", "whole"), ("1/3", "none"), ("2/3", "none"), ("0/1", "whole"), ("", "whole")])
def test_shard_as_documented(env_exe, value, total):
    out, err = _configured(env_exe, STORM_HIP_SHARD=value)
    assert out == "slots=1 total=" + total and "STORM_HIP_SHARD" not in err


@pytest.mark.parametrize("value", ["3/3", "1/0", "1", "x", "1/3x", " 1/3", "-1/3", "1/-3", "1/", "/3", "1/99999999999"])
def test_malformed_shard_is_one_line_and_no_shard(env_exe, value):
    """a value the parser did not like was dropped without a word: every rank of a job returned the whole total"""
    out, err = _configured(env_exe, STORM_HIP_SHARD=value)
    assert out == "slots=1 total=whole"
    assert err.count('libstorm_hip: STORM_HIP_SHARD: "%s" ignored (rank/world expected, rank < world)' % value) == 1, err


def test_options_of_any_length_entry_by_entry(env_exe):
    """2000 bytes of entries (a 512-byte buffer used to cut the string mid-entry): the stub's option check refuses keys that
    begin with `?`, the host side remembers 16 distinct keys"""
    entries = ["key%02d=%d" % (k % 16, k) for k in range(200)] + ["?typo=1", "seventeenth=1", "novalue", "key00=", "key00=1x"]
    assert len(",".join(entries)) > 1500
    out, err = _configured(env_exe, STORM_HIP_OPTIONS=",".join(entries))
    assert out == "slots=1 total=whole"
    lines = [ln for ln in err.splitlines() if "STORM_HIP_OPTIONS: entry" in ln]
    assert [ln.split('"')[1] for ln in lines] == ["?typo=1", "seventeenth=1", "novalue", "key00=", "key00=1x"], err
