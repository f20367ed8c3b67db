"""The library's hardware-queue request (flx_hw_queue_request, FLX_HW_QUEUES): what a process finds in GPU_MAX_HW_QUEUES once the library is
loaded. The request is made by the library's load-time constructor, so every case is a fresh child process that only loads the library
and prints the variable - as Python sees it and as the C environment, which the HIP runtime reads, holds it - and what the library says
it did. No GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1])
import floxer_amd as F
requested, found = F.hw_queue_request()
getenv = ctypes.CDLL(None).getenv
getenv.restype, getenv.argtypes = ctypes.c_char_p, [ctypes.c_char_p]
c_value = getenv(b"GPU_MAX_HW_QUEUES")
print(json.dumps(dict(value=os.environ.get("GPU_MAX_HW_QUEUES"), c_value=None if c_value is None else c_value.decode(), requested=requested, found=found)))
"""


def load_library(on_entry, knob):
    """a child that loads the library with GPU_MAX_HW_QUEUES = on_entry and FLX_HW_QUEUES = knob (None: unset) and reports"""
    env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "FLX_HW_QUEUES")}
    if on_entry is not None:
        env["GPU_MAX_HW_QUEUES"] = on_entry
    if knob is not None:
        env["FLX_HW_QUEUES"] = knob
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


# (GPU_MAX_HW_QUEUES on entry, FLX_HW_QUEUES, the value behind the load, what the library says it wrote, what it says it found or None: not checked)
CASES = [
    ("4", None, "16", 16, 4),          # 1. a preset value does not win
    (None, None, "16", 16, -1),        # 2. nothing set: the default
    ("4", "8", "8", 8, None),          # 3. the knob's value
    ("4", "0", "4", 0, None),          # 4. the opt-out: the variable as it was found, nothing requested
    ("4", "64", "32", 32, None),       # 5. clamped from above
    ("4", "2", "4", 4, None),          # 6. clamped from below
    ("4", "abc", "16", 16, None),      # 7. not a number: the default
]


@pytest.mark.parametrize("on_entry,knob,value,requested,found", CASES, ids=[f"case{i + 1}" for i in range(len(CASES))])
def test_request_at_load(on_entry, knob, value, requested, found):
    got = load_library(on_entry, knob)
    assert got["value"] == value and got["c_value"] == value, got
    assert got["requested"] == requested, got
    if found is not None:
        assert got["found"] == found, got


def test_lane_overlap_refuses_null_arguments():
    import ctypes as C
    from floxer_amd import capi
    L = capi.lib()
    ms = (C.c_float * 4)()
    assert L.flx_ctx_lane_overlap(None, 4, 1000, ms, ms) == -1 and b"flx_ctx_lane_overlap" in L.flx_last_error()


def test_opt_out_leaves_an_unset_variable_unset():
    got = load_library(None, "0")
    assert got == dict(value=None, c_value=None, requested=0, found=-1)
