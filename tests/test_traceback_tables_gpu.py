"""The traceback stage's result tables at every size of the lane's mapped result block, and its passes through both doors.

A lane's small result tables come back through a mapped block of 1 MiB (Lane::result_slot). With every option on a traced path asks it
for about 110 bytes, so no other test ever leaves the block: the copy branches of Traceback::run (the four tables a later pass reads
on the device are published together or not at all; cigar_realign's and cs_build's go on their own), of launch_by_shape, of the union
form's lastrow_min and of the seeding stage run here only. FLX_RESULT_BLOCK_BYTES (read when a lane's block is first made) bounds the
block; FLX_ALIGN_DEBUG's `[traceback]` line tells for every call which tables had a range of the block (1), which had none and were
copied (0) and which were not wanted (-). Whatever the block holds, records, strings, scores and every kernel's launches, bytes and
units are the same.

Then the batch door (flx_align_batch_cs) without a block, and every pass alone (flx_*_batch) against its host rule: a launch through
that door is accounted under the name the chain uses. Needs an MI355X (-m gpu)."""
import re

import numpy as np
import pytest

import floxer_amd as F
import align_corpus as AC
import realign_ref as R
from test_realign_gpu import corpus_cases
from test_tails_gpu import RATE, SPAN, build_batch

gpu = pytest.mark.gpu
KERNELS = ("ed_traceback", "cigar_realign", "cigar_left_align", "md_build", "cs_build", "cigar_tails")
LINE = re.compile(r"\[traceback\] jobs (\d+) block: outs md tails la ra cs = ([01-]) ([01-]) ([01-]) ([01-]) ([01-]) ([01-]) asked (\d+)")


def one_lane_context(monkeypatch, idx, block):
    """a context of one lane whose result block is bounded by `block` bytes (None: the default); the bound stays set: the block is made
    on first use"""
    monkeypatch.setenv("FLX_LANES", "1")
    if block is None:
        monkeypatch.delenv("FLX_RESULT_BLOCK_BYTES", raising=False)
    else:
        monkeypatch.setenv("FLX_RESULT_BLOCK_BYTES", str(block))
    ctx = F.context(idx)
    ctx.enable_kernel_timing(True)
    return ctx


def run_with_every_table(monkeypatch, capfd, idx, reads, block):
    """the batch with everything on that adds a table; returns what the run holds, the kernels' accounting and the [traceback] lines as
    (jobs, six flags, asked)"""
    ctx = one_lane_context(monkeypatch, idx, block)
    try:
        al = F.aligner(ctx, F.params(error_probability=RATE), F.output_options(max_alignments=1, mapq=True), md=True, gaps=F.gap_options(),
                       realign=F.realign_options(), cs=F.cs_options(long=True), partial=F.partial_options(min_query_span=SPAN),
                       extend=F.extend_options(), split=F.split_options())
        monkeypatch.setenv("FLX_ALIGN_DEBUG", "1")
        capfd.readouterr()
        run = al.align_reads(reads)
        err = capfd.readouterr().err
        monkeypatch.delenv("FLX_ALIGN_DEBUG")
        stats = ctx.kernel_stats()
    finally:
        ctx.close()
    lines = [(int(m.group(1)), tuple(m.group(i) for i in range(2, 8)), int(m.group(8))) for m in LINE.finditer(err)]
    held = dict(records=run.records(), skipped=run.skipped.tolist(), md=run.md, cs=run.cs, scores=run.scores.tolist(), mapq=run.mapq.tolist())
    counted = {k: (stats[k]["launches"], stats[k]["algorithmic_bytes"], stats[k]["work_units"]) for k in KERNELS}
    return held, counted, lines


@gpu
def test_every_block_size_gives_the_same_run_and_the_same_accounting(monkeypatch, capfd):
    chroms, reads, tailed, rescued = build_batch()
    idx = F.fmindex(chroms)
    base, base_counted, base_lines = run_with_every_table(monkeypatch, capfd, idx, reads, None)
    assert base_lines and all(f in "1-" for _, flags, _ in base_lines for f in flags), base_lines      # every wanted table has its range
    assert any(all(f == "1" for f in flags) for _, flags, _ in base_lines)                           # the root stage wants all six
    assert all(base_counted[k][0] >= 1 for k in KERNELS), base_counted
    # not vacuous: mapped, split and rescued records, each with its strings
    assert any("S" in r[5] for r in base["records"]) and any(r[1] & 2048 for r in base["records"])
    assert all((m is not None) == (c is not None) == (not r[1] & 4) for r, m, c in zip(base["records"], base["md"], base["cs"]))
    jobs, _, asked = max(base_lines, key=lambda l: l[2])
    # The seeding stage's 136 bytes fit into 136. Ranges start at multiples of 64 and K4's table, which is taken first, has at least 8
    # bytes per traced path: behind it not even the call's smallest table (8 bytes per path) fits, and K5's own 16 per path do not either.
    small = 136
    assert (8 * jobs + 63) // 64 * 64 + 8 * jobs > small and 16 * jobs > small
    # K4's two tables of the largest call (the unions' scores and their windows' minima, not in `asked`) lie in front of the traceback's.
    # The lines at asked // 2 and asked - 64 put them between 672 and 1024 bytes: at asked - 64 the tails' table has no room left, and
    # asked + 512 is the size at which the four tables the device reads fit behind them and cigar_realign's statistics do not.
    seen, shown = list(base_lines), []
    for block in (0, small, asked // 2, asked - 64, asked + 512):
        held, counted, lines = run_with_every_table(monkeypatch, capfd, idx, reads, block)
        for key in base:
            assert held[key] == base[key], (block, key)
        assert counted == base_counted, (block, counted, base_counted)
        assert [(n, a) for n, _, a in lines] == [(n, a) for n, _, a in base_lines], block             # the same calls asking for the same
        if block == 0:
            assert all(f in "0-" for _, flags, _ in lines for f in flags), lines
        if block == small:
            assert all(f in "0-" for n, flags, _ in lines if n == jobs for f in flags), lines
        seen += lines
        shown.append((block, lines))
    print("default block:", base_lines, base_counted)
    for block, lines in shown:
        print("block", block, ":", lines)
    wanted = lambda flags: [f for f in flags if f != "-"]
    device_read = lambda flags: wanted(flags[:4])
    assert any(set(wanted(flags)) == {"1"} for _, flags, _ in seen)
    assert any(set(wanted(flags)) == {"0"} for _, flags, _ in seen)
    # a range was taken and the tables the device reads are copied all the same: one of them had none
    assert any(flags[0] == "1" and "0" in flags[1:] for _, flags, _ in seen), seen
    # those four in the block, cigar_realign's statistics or cs_build's lengths copied on their own
    assert any(set(device_read(flags)) == {"1"} and "0" in flags[4:] for _, flags, _ in seen), seen


def words_and_jobs(what, results):
    """the words of a batch's results as the pools and jobs the doors of a pass alone take"""
    return R.pack_jobs([(R.parse(p[2]), c.ref, c.query, p[1]) for (c, _), p in zip(what, results)])


@gpu
def test_the_batch_door_without_a_block_and_every_pass_alone_under_the_chains_name(monkeypatch):
    cases = corpus_cases()
    rpool, qpool, jobs, what = AC.batch(cases, (2,))
    idx = F.fmindex([np.random.default_rng(5).integers(1, 5, size=2000).astype(np.uint8)])

    def batch_door(ctx):
        got = F.align_batch_cs(ctx, qpool, jobs, F.cs_options(long=True), reference_pool=rpool, md=True, gaps=F.gap_options(), realign=F.realign_options())
        stats = ctx.kernel_stats()
        assert all(stats[k]["launches"] >= 1 for k in KERNELS if k != "cigar_tails") and "cigar_tails" not in stats      # (this door has no tails)
        return got

    ctx = one_lane_context(monkeypatch, idx, 0)
    try:
        without = batch_door(ctx)
    finally:
        ctx.close()
    ctx = one_lane_context(monkeypatch, idx, None)
    try:
        assert batch_door(ctx) == without and all(g is not None and g[3] and g[5] for g in without)
        # the four doors of a pass alone on K5's words of this batch: what the host rule returns, and one more launch under the chain's name
        plain = F.align_batch(ctx, qpool, jobs, reference_pool=rpool)
        ref, qry, words, hjobs = words_and_jobs(what, plain)
        launches = lambda name: ctx.kernel_stats()[name]["launches"]
        before = launches("cigar_left_align")
        dev, host = F.left_align_batch(ctx, qry, words, hjobs, reference_pool=ref), F.left_align(ref, qry, words, hjobs)
        assert len(dev) == len(host) == len(jobs) and all(np.array_equal(a, b) for a, b in zip(dev, host))
        assert launches("cigar_left_align") == before + 1
        before = launches("cigar_realign")
        dev, host = F.realign_batch(ctx, qry, words, hjobs, F.realign_options(), reference_pool=ref), F.realign(ref, qry, words, hjobs, F.realign_options())
        assert len(dev) == len(host) == len(jobs)
        for a, b in zip(dev, host):
            assert np.array_equal(a["words"], b["words"]) and {k: v for k, v in a.items() if k != "words"} == {k: v for k, v in b.items() if k != "words"}
        assert launches("cigar_realign") == before + 1
        before = launches("cs_build")
        assert F.cs_batch(ctx, qry, words, hjobs, long=True, reference_pool=ref) == F.cs_string(ref, qry, words, hjobs, long=True)
        assert launches("cs_build") == before + 1
        assert "cigar_tails" not in ctx.kernel_stats()
        tjobs = [(j[0], j[1]) for j in hjobs]
        assert F.cigar_tails_batch(ctx, words, tjobs).tolist() == F.cigar_tails(words, tjobs).tolist()
        # its first launch on this context, priced as the chain prices it: job, DevTraceOut and result per job, and the words read
        st = ctx.kernel_stats()["cigar_tails"]
        assert (st["launches"], st["work_units"]) == (1, len(tjobs))
        assert st["algorithmic_bytes"] == len(tjobs) * (24 + 16 + 32) + 4 * sum(j[1] for j in tjobs)
    finally:
        ctx.close()
