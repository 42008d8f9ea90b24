"""The source list of the stand-alone host programs the test_*_sanitize.py files build for the dosage container: what every one
of them links, then the unit under test and its own stub and driver. Tests only."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stormbitmaps_amd", "csrc")
STUBS = os.path.join(ROOT, "tests", "host_sanitize")

# the containers, the frame of their entry points (storm_host_call.c) and what the calls on the band of r^2 share
# (storm_dosage_band.c, with its planner)
_HOST = ("storm_host.c", "storm_host_call.c", "storm_dosage.c", "storm_dosage_band.c", "storm_ldscore_window.c", "storm_synth.c",
         "storm_leaves.c")
# the "device" in host memory: contexts and matrices, the dosage calls storm_dosage.c and storm_dosage_pairs.c make, the band
# calls and the wait
_DEVICE = ("device_stub.c", "dosage_complete_stub.c", "dosage_pairs_stub.c", "dosage_band_stub.c")


def dosage_sources(units, extra):
    """`units` of stormbitmaps_amd/csrc and `extra` files of tests/host_sanitize (a stub of their own, the driver)."""
    return [os.path.join(CSRC, f) for f in _HOST + tuple(units)] + [os.path.join(STUBS, f) for f in _DEVICE + tuple(extra)]
