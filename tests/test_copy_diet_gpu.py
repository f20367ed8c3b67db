"""The chunk path without its per-buffer fills and small copies (stage clears, the lanes' mapped result block, staged uploads): a lane
that is used again sees nothing of its previous chunk, the root stage (union DP, last-row minima read without a fill in front of K4,
traceback) equals the oracle also over several arena chunks, chunks without a root or with one do not hang, and a context refuses to
go while a read batch of it is alive. Through the C ABI, bit-exact against the CPU oracle. Needs an MI355X (-m gpu)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
from floxer_amd import simulate as S
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _env:
    """environment variables for the duration of a block (the library reads these when a context is made, or per call)"""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def text_1mb():
    """a 1 Mb text, its index on both sides; shared by the tests of this file and left unchanged"""
    genome = S.make_genome(1000000, 1, seed=711)
    return genome, F.fmindex(genome), O.Index(genome)


# ---------------------------------------------------------------- 1. a lane used again
def test_reused_lane_sees_nothing_of_its_previous_chunk(text_1mb):
    """one context with one lane; batches of 64, 17 and 1 reads of 1 kb @ 5 % one after the other and then the first again: a count or
    job table left from the previous use would be over-read (17 after 64, 1 after 17) or under-read (64 after 1). Every result equals the
    oracle's record for record, the fourth equals the first."""
    genome, idx, oidx = text_1mb
    batches = [S.make_reads(genome, n, 1000, 0.05, seed=720 + i)[0] for i, n in enumerate((64, 17, 1))]
    exp = [oidx.run(b, O.params(error_probability=0.05), threads=8) for b in batches]
    with _env(FLX_LANES="1"):
        ctx = F.context(idx)
    al = F.aligner(ctx, F.params(error_probability=0.05))
    got = [al.align_reads(batches[i]) for i in (0, 1, 2, 0)]
    for g, i in zip(got, (0, 1, 2, 0)):
        assert g.skipped.tolist() == exp[i].skipped.tolist(), i
        assert g.records() == exp[i].records(), i
    assert got[3].records() == got[0].records()
    assert sum(1 for r in got[0].records() if not r[1] & 4) >= 64
    ctx.close()


# ---------------------------------------------------------------- 2. the root stage
TANDEM_PERIOD = 200      # > k = 160 (2 kb @ 8 %): a window holds the end of its own copy only; < 256: the copies' windows fall into one union


def root_stage_inputs():
    """24 reads of 2 kb @ 8 % on a 1 Mb text, two of them out of a tandem array planted in the text (13 copies of a 200-base unit): such a
    read aligns at every copy it fits, one period apart, with the same score. The windows of neighbouring copies start within 256 columns
    of each other, so they share one union DP, and each holds only the end of its own copy's alignment (the period is larger than k):
    two members of one union that end at different columns, built here on the CPU."""
    genome = S.make_genome(1000000, 1, seed=731)
    rng = np.random.default_rng(732)
    unit = rng.integers(1, 5, size=TANDEM_PERIOD, dtype=np.uint8)
    array = np.tile(unit, 13)
    at = 400000
    genome[0][at: at + len(array)] = array
    reads, _, _ = S.make_reads(genome, 22, 2000, 0.08, seed=733)
    for start in (0, 70):
        r = array[start: start + 2000].copy()
        for p in rng.choice(2000, size=40, replace=False):            # 2 % mismatches: every copy still aligns well within k
            r[p] = (r[p] % 4) + 1
        reads.append(np.ascontiguousarray(r))
    return genome, reads


_ROOT_CHILD = """
import sys, json, os
sys.path.insert(0, %r); sys.path.insert(0, %r)
import floxer_amd as F
import test_copy_diet_gpu as T
genome, reads = T.root_stage_inputs()
idx = F.fmindex(genome)
out = []
for kb in (None, '1024'):
    if kb: os.environ['FLX_TRACE_ARENA_KB'] = kb
    c = F.context(idx); c.enable_kernel_timing(True)
    res = F.aligner(c, F.params(error_probability=0.08)).align_reads(reads)
    out.append(dict(skipped=res.skipped.tolist(), records=res.records(), tracebacks=c.kernel_stats()['ed_traceback']['launches']))
    c.close()
print(json.dumps(out))
"""


def _root_stage_child(**env):
    """in a child (FLX_UNION_ALIGN_OWN is read once per process, the arena budget when a context is made): the batch on a context with the
    default trace arena and on one whose lanes hold 1 MB of trace planes each; per context records, skipped and ed_traceback launches, and
    the child's stderr (FLX_ALIGN_DEBUG's lines)"""
    child_env = {k: v for k, v in os.environ.items() if k not in ("FLX_TRACE_ARENA_MB", "FLX_TRACE_ARENA_KB", "FLX_NO_UNION", "FLX_UNION_ALIGN_OWN")}
    child_env.update(FLX_LANES="1", FLX_ALIGN_DEBUG="1", **env)
    out = subprocess.run([sys.executable, "-c", _ROOT_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=child_env, capture_output=True, text=True, check=True)
    return json.loads(out.stdout.strip().split("\n")[-1]), out.stderr


@pytest.fixture(scope="module")
def root_stage_expected():
    genome, reads = root_stage_inputs()
    exp = O.Index(genome).run(reads, O.params(error_probability=0.08), threads=8)
    return exp.skipped.tolist(), [list(r) for r in exp.records()]


def test_root_stage_unions_with_members_that_end_at_different_columns(root_stage_expected):
    """the union form as it is: equal to the oracle with the default arena and with an arena of 1 MB per lane, which holds about nine of
    the batch's union DPs (112 KB of trace planes each) at a time: several arena chunks, read off the ed_traceback launches (one per
    arena chunk with a path). FLX_TRACE_ARENA_MB, the knob of the existing union tests, cannot go below 128 MB per lane, which this
    batch never fills; FLX_TRACE_ARENA_KB is the same budget in KB without that floor. FLX_ALIGN_DEBUG's line tells that at least one
    union had two traceback jobs (members that end at different columns)."""
    skipped, records = root_stage_expected
    (default, small), err = _root_stage_child()
    lines = re.findall(r"\[root unions\] requests (\d+) distinct (\d+) unions (\d+) aligned on their own (\d+) traceback jobs (\d+) unions with several jobs (\d+)", err)
    print("root unions lines:", lines, "ed_traceback launches: default arena %d, small arena %d" % (default["tracebacks"], small["tracebacks"]))
    assert lines, err[-2000:]
    for requests, distinct, unions, own, tjobs, several in lines:
        assert int(unions) < int(distinct)                 # unions with several members
        assert int(several) >= 1                           # two traceback jobs for one union
    for run in (default, small):
        assert run["skipped"] == skipped
        assert run["records"] == records
    assert small["tracebacks"] >= default["tracebacks"] + 1 and small["tracebacks"] >= 2


def test_root_stage_every_member_aligned_on_its_own(root_stage_expected):
    """FLX_UNION_ALIGN_OWN: as if every union path left its members' windows (the `res.begin < shift` way out)"""
    skipped, records = root_stage_expected
    (default, small), err = _root_stage_child(FLX_UNION_ALIGN_OWN="1")
    lines = re.findall(r"\[root unions\] requests (\d+) distinct (\d+) unions (\d+) aligned on their own (\d+)", err)
    assert lines and all(int(own) > 0 for _, _, _, own in lines), err[-2000:]
    for run in (default, small):
        assert run["skipped"] == skipped
        assert run["records"] == records


# ---------------------------------------------------------------- 2b. the last row's ties and its threshold
TIE_PERIOD = 64          # <= k = 80 (1 kb @ 8 %): a window holds the ends of neighbouring copies, 64 columns apart: one lane of lastrow_min
TIE_K = 80


def last_row(window, query):
    """D[m][c], c = 0 .. n, of the semi-global matrix (the window's ends are free), row by row"""
    window, query = np.asarray(window, dtype=np.int64), np.asarray(query, dtype=np.int64)
    js = np.arange(len(window) + 1)
    row = np.zeros(len(window) + 1, dtype=np.int64)
    for i in range(1, len(query) + 1):
        cand = row + 1
        cand[1:] = np.minimum(cand[1:], row[:-1] + (window != query[i - 1]))
        cand[0] = i
        row = np.minimum.accumulate(cand - js) + js
    return row


def tie_inputs():
    """8 reads of 1 kb on a 200 kb text: six as they come, one out of a tandem array of 40 copies of a 64-base unit (2 % mismatches),
    one with exactly k = 80 substitutions, one every 12 or 13 bases. Returns (genome, reads, index of the tandem read, of the other,
    the other's locus)."""
    genome = S.make_genome(200000, 1, seed=741)
    rng = np.random.default_rng(742)
    array = np.tile(rng.integers(1, 5, size=TIE_PERIOD, dtype=np.uint8), 40)
    genome[0][80000: 80000 + len(array)] = array
    reads, _, _ = S.make_reads(genome, 6, 1000, 0.08, seed=743)
    r = array[10: 1010].copy()
    for p in rng.choice(1000, size=20, replace=False):
        r[p] = (r[p] % 4) + 1
    reads.append(np.ascontiguousarray(r))
    locus = 150000
    r = genome[0][locus: locus + 1000].copy()
    for p in (np.arange(TIE_K) * 12.5).astype(int) + 3:
        r[p] = (r[p] % 4) + 1
    reads.append(np.ascontiguousarray(r))
    return genome, reads, 6, 7, locus


def test_root_stage_takes_the_rightmost_of_two_minima_64_columns_apart_and_a_minimum_of_exactly_k():
    """lastrow_min at its two comparisons, through the only door it has (the union form of the root stage), against the oracle. A lane
    of its wave reads the columns c, c + 64, ..: two minima of a member's last row that lie 64 columns apart are one lane's, and the later
    one must win there before the wave's reduction sees either. And a member whose minimum is exactly its k has an alignment. Both
    situations are shown on the CPU first: on the last row of the matrix for the tandem read, by the oracle's own DP for the other."""
    genome, reads, tandem, at_k, locus = tie_inputs()
    exp = O.Index(genome).run(reads, O.params(error_probability=0.08), threads=8)
    rows = {i: [r for r in exp.records() if r[0] == i] for i in (tandem, at_k)}
    # the read with k substitutions: one record, NM == k, and no alignment within k - 1
    window = genome[0][locus - TIE_K: locus + 1000 + TIE_K]
    assert [(r[1] & 4, r[3], r[4]) for r in rows[at_k]] == [(0, locus, TIE_K)]
    assert O.align(window, reads[at_k], TIE_K, mode=0, algo=0)[0] == TIE_K and O.align(window, reads[at_k], TIE_K - 1, mode=0, algo=0) is None
    # the tandem read: behind its primary record's end the last row holds the same minimum 64 columns earlier
    primary = [r for r in rows[tandem] if not r[1] & (4 | 256)]
    assert len(primary) == 1 and len(rows[tandem]) > 1
    span = sum(int(n) for n, op in re.findall(r"(\d+)([=XID])", primary[0][5]) if op != "I")
    end = primary[0][3] + span
    strand = reads[tandem] if not primary[0][1] & 16 else O.revcomp(reads[tandem])
    row = last_row(genome[0][end - 1000 - 2 * TIE_K: end], strand)
    best = np.flatnonzero(row == row.min())
    assert row.min() == primary[0][4] <= TIE_K and best[-1] == len(row) - 1 and len(row) - 1 - TIE_PERIOD in best, (row.min(), best[-5:])
    with _env(FLX_LANES="1"):
        ctx = F.context(F.fmindex(genome))
    ctx.enable_kernel_timing(True)
    got = F.aligner(ctx, F.params(error_probability=0.08)).align_reads(reads)
    stats = ctx.kernel_stats()
    ctx.close()
    assert stats["ed_lastrow_min"]["launches"] >= 1 and stats["ed_lastrow_min"]["work_units"] > len(reads)      # the union form ran, over more windows than reads
    assert got.skipped.tolist() == exp.skipped.tolist()
    assert got.records() == exp.records()


# ---------------------------------------------------------------- 3. empty and degenerate chunks
def test_chunk_without_a_root_and_chunk_with_one_root(text_1mb, capfd):
    """a chunk none of whose reads reaches a root (random reads: no K4, no windows, no traceback job) and a chunk with exactly one root
    alignment (one 60-base read with two errors allowed: its PEX tree is the root alone, one copy in the text): what the oracle
    returns, on one lane that runs the empty chunk between two others."""
    genome, idx, oidx = text_1mb
    rng = np.random.default_rng(741)
    randoms = [rng.integers(1, 5, size=1000, dtype=np.uint8) for _ in range(8)]
    mapped = S.make_reads(genome, 5, 1000, 0.05, seed=742)[0]
    one = [np.ascontiguousarray(genome[0][123456: 123456 + 60])]
    with _env(FLX_LANES="1"):
        ctx = F.context(idx)
    al = F.aligner(ctx, F.params(error_probability=0.05))
    for batch in (mapped, randoms, mapped):
        exp = oidx.run(batch, O.params(error_probability=0.05), threads=8)
        got = al.align_reads(batch)
        assert got.skipped.tolist() == exp.skipped.tolist()
        assert got.records() == exp.records()
        if batch is randoms:
            assert all(r[1] & 4 for r in got.records())
    capfd.readouterr()
    exp = oidx.run(one, O.params(query_errors=2), threads=1)
    with _env(FLX_ALIGN_DEBUG="1"):
        got = F.aligner(ctx, F.params(query_errors=2)).align_reads(one)
    err = capfd.readouterr().err
    assert got.records() == exp.records()
    assert len(got.records()) == 1 and not got.records()[0][1] & 4
    jobs = [int(j) for j in re.findall(r"\[ed_align_trace\].* jobs (\d+) ", err)]
    print("K4 launches of the one-root chunk, jobs each:", jobs)
    assert sum(jobs) == 1, err[-2000:]
    ctx.close()


# ---------------------------------------------------------------- a context and its read batches
def test_context_refuses_to_go_while_a_read_batch_is_alive(text_1mb):
    """flx_ctx_destroy with a live flx_reads returns an error and leaves both usable; after flx_reads_free it succeeds"""
    genome, idx, oidx = text_1mb
    reads = S.make_reads(genome, 4, 1000, 0.05, seed=751)[0]
    exp = oidx.run(reads, O.params(error_probability=0.05), threads=4)
    ctx = F.context(idx)
    resident = F.resident_reads(ctx, reads)
    lib = capi.lib()
    assert lib.flx_ctx_destroy(ctx.h) < 0
    assert b"alive" in lib.flx_last_error()
    assert F.aligner(ctx, F.params(error_probability=0.05)).align_reads(resident).records() == exp.records()      # context and batch still work
    resident.close()
    h, ctx.h = ctx.h, None
    assert lib.flx_ctx_destroy(h) == 0
