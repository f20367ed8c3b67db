"""Do the lanes' kernels overlap once the library's hardware-queue request holds? Two fresh child processes, one after the other, each in
the order of bench.py: GPU_MAX_HW_QUEUES=4 preset and FLX_LANES=12, import torch (no GPU call), import the package (which loads the
library), let torch make the process's first GPU call, make a context on a text of a few kilobases, run the lane-overlap probe
(flx_ctx_lane_overlap) on one lane and then on twelve.
The measure is C, the number of the twelve kernels that had started before the first of them stopped. Child A runs with the library's
default request and must show C above the preset's ceiling of four; child B is the control with FLX_HW_QUEUES=0 (the preset stays):
its C describes the runtime, not this code, and is printed only. Needs an MI355X (-m gpu)."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LANES = 12
PRESET = 4
ITERATIONS = 100000      # one wave's dependent chain of this many steps lasts about 2 ms on an MI355X (fixed, not calibrated by the test)

CHILD = """
import json, os, sys
sys.path.insert(0, sys.argv[1])
lanes, iterations = int(sys.argv[2]), int(sys.argv[3])
import torch
assert not torch.cuda.is_initialized()
import floxer_amd as F
from floxer_amd import simulate as S
assert torch.cuda.is_available()      # (as bench.py: the process's first GPU call comes from torch, behind both imports and before any call into the library)
torch.cuda.set_device(0)
requested, found = F.hw_queue_request()
ctx = F.context(F.fmindex(S.make_genome(8000, 1, seed=97)))
one_start, one_stop = ctx.lane_overlap(1, iterations)
start, stop = ctx.lane_overlap(lanes, iterations)
ctx.close()
print(json.dumps(dict(requested=requested, found=found, value=os.environ.get("GPU_MAX_HW_QUEUES"), single_ms=one_stop[0] - one_start[0], start=start, stop=stop)))
"""


def run_child(knob):
    env = {k: v for k, v in os.environ.items() if k != "FLX_HW_QUEUES"}
    env.update(GPU_MAX_HW_QUEUES=str(PRESET), FLX_LANES=str(LANES))
    if knob is not None:
        env["FLX_HW_QUEUES"] = knob
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(LANES), str(ITERATIONS)], env=env, capture_output=True, text=True, timeout=120)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    first_stop = min(got["stop"])
    got["C"] = sum(1 for s in got["start"] if s < first_stop)
    got["span_ms"] = max(got["stop"]) - min(got["start"])
    got["wall_s"] = wall
    return got


def describe(name, got):
    print(f"{name}: requested {got['requested']} found {got['found']} GPU_MAX_HW_QUEUES {got['value']}: single-lane kernel {got['single_ms']:.3f} ms, "
          f"C = {got['C']} of {LANES}, all {LANES} kernels within {got['span_ms']:.3f} ms, child wall {got['wall_s']:.2f} s")
    print(f"{name}: starts " + " ".join(f"{s:.3f}" for s in got["start"]))
    print(f"{name}: stops  " + " ".join(f"{s:.3f}" for s in got["stop"]))


def test_lanes_overlap_beyond_the_preset_queues():
    a = run_child(None)
    describe("default request", a)
    b = run_child("0")
    describe("control (FLX_HW_QUEUES=0)", b)
    assert (a["requested"], a["found"], a["value"]) == (16, PRESET, "16"), a
    assert (b["requested"], b["found"], b["value"]) == (0, PRESET, str(PRESET)), b
    for got in (a, b):
        assert len(got["start"]) == LANES and all(e > s for s, e in zip(got["start"], got["stop"])), got
    assert a["C"] > PRESET, a
