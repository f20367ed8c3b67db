"""Depth of coverage on the GPU (flx_coverage: kernels coverage_add, the three-launch scan, the run heads, coverage_windows, the absorb's sum;
runs, the Python class and the CLI's --coverage outputs). Every expected value is the plain-numpy rule of tests/coverage_ref.py on the
same records and words; the shapes sit on the kernels' boundaries (64 CIGAR words per pass, the scan's tile and second level)."""
import ctypes as C
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import coverage_ref as R

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = (0, 1, 7, 1000)


def same(cov, lengths, want, report_zero, windows=WINDOWS):
    """depth, runs and windows of a finished object against the reference's on the expected depth"""
    starts = R.starts_of(lengths)
    got = np.concatenate([cov.depth(r, 0, n) for r, n in enumerate(lengths)]) if len(lengths) <= 16 else None
    if got is None:                                                       # many sequences: a few stretches, the runs cover the rest
        for r in (0, 1, len(lengths) // 2, len(lengths) - 1):
            assert (cov.depth(r, 0, lengths[r]) == want[starts[r]: starts[r + 1]]).all(), r
    else:
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    runs, exp = cov.runs(), R.runs(lengths, want, report_zero)
    assert len(runs) == len(exp) and (runs == exp).all()
    for w in windows:
        win, exp = cov.windows(w), R.windows(lengths, want, w)
        assert len(win) == len(exp) and (win == exp).all(), w


def measure(lengths, rec, words, o, windows=WINDOWS, adds=1):
    cov = F.coverage(lengths=lengths, options=R.c_options(o))
    try:
        for part in np.array_split(np.arange(len(rec)), adds):
            cov.add_records(rec[part], words)
        cov.finish()
        same(cov, lengths, R.depth(lengths, rec, words, o), o["report_zero"], windows)
    finally:
        cov.close()


# ------------------------------------------------------------------------------------------------ words and carries
@gpu
@pytest.mark.parametrize("n_words", [1, 63, 64, 65, 129, 4097])
def test_words_and_carries(n_words):
    rng = np.random.default_rng(n_words)
    lengths = [45_000, 33_000]
    eq = [R.word("=", int(n)) for n in rng.integers(1, 9, size=n_words)]
    mixed = R.random_words(rng, n_words, max_len=9)
    body = R.random_words(rng, max(1, n_words - 2), max_len=9, clips=False)
    d_first = ([R.word("S", 7)] if n_words >= 3 else []) + [R.word("D", 3)] + body[1:] + ([R.word("I", 2)] if n_words >= 3 else [])
    d_last = body[:-1] + [R.word("D", 4)] + ([R.word("S", 5)] if n_words >= 2 else [])
    rows = [(0, 0, 11, 0, eq), (16, 1, 0, 0, mixed), (0, 1, 5, 0, d_first), (2048, 0, 45_000 - R.span(d_last), 0, d_last)]
    assert len(eq) == len(mixed) == n_words and all(R.span(r[4]) <= 33_000 for r in rows)
    rec, words = R.records_of(rows)
    for dels in (False, True):
        measure(lengths, rec, words, R.options(count_deletions=dels))
    if n_words > 2:
        assert (R.depth(lengths, rec, words, R.options()) != R.depth(lengths, rec, words, R.options(count_deletions=True))).any()


# ------------------------------------------------------------------------------------------------ edges
def edge_cases():
    t, _ = F.coverage_geometry()
    rng = np.random.default_rng(3)
    small = [int(n) for n in rng.integers(1, 4, size=1000)]
    pad = t - sum(small) % t                                               # the sequences behind the small ones start on a tile boundary again
    lengths = [t, t] + small + [pad, t + 5]
    last = len(lengths) - 1
    cases = {
        "first": [(0, 0, 0, 0, [R.word("=", 1)])],
        "last": [(16, last, t + 4, 0, [R.word("X", 1)])],
        "spans": [(0, 1, 0, 0, [R.word("=", t)])],
        "neighbours": [(0, 0, 0, 0, [R.word("=", t)]), (0, 1, 0, 0, [R.word("=", t - 1), R.word("X", 1)]), (0, last - 1, 0, 0, [R.word("=", pad)]),
                       (0, last, 0, 0, [R.word("=", t + 5)])],
        "small": [(0, 2 + i, 0, 0, [R.word("=", n)]) for i, n in enumerate(small) if i % 3] + [(0, 2 + i, n - 1, 0, [R.word("=", 1)]) for i, n in enumerate(small) if i % 5 == 0],
    }
    cases["together"] = [row for rows in cases.values() for row in rows]
    return lengths, cases


@gpu
@pytest.mark.parametrize("name", ["first", "last", "spans", "neighbours", "small", "together"])
def test_edges(name):
    lengths, cases = edge_cases()
    t, _ = F.coverage_geometry()
    starts = R.starts_of(lengths)
    assert starts[1] % t == 0 and starts[2] % t == 0 and starts[-2] % t == 0 and min(lengths) == 1
    rec, words = R.records_of(cases[name])
    for zero in (False, True):
        measure(lengths, rec, words, R.options(report_zero=zero), windows=(0, 2, 1000))
    if name == "neighbours":                                             # equal depth on both sides: the run still breaks at the boundary
        runs = R.runs(lengths, R.depth(lengths, rec, words, R.options()))
        assert runs[["ref", "start", "end"]].tolist() == [(0, 0, t), (1, 0, t), (len(lengths) - 2, 0, lengths[-2]), (len(lengths) - 1, 0, t + 5)]


# ------------------------------------------------------------------------------------------------ scan geometry
def geometry_totals():
    t, b = F.coverage_geometry()
    return [1, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1, t * b + 1]


@gpu
@pytest.mark.parametrize("which", range(9))
def test_scan_geometry(which):
    t, b = F.coverage_geometry()
    total = geometry_totals()[which]
    assert t * b + 1 <= 1 << 28
    lengths = [total]
    windows = (0, 1000) if total > 1 << 20 else WINDOWS
    # depth 2, 1, 2, 1, ..: one record over everything and records that count every other column (a D between, not counted): every
    # position is a run head
    step = 8192
    words = np.concatenate([np.tile(np.array([R.word("=", 1), R.word("D", 1)], dtype=np.uint32), step // 2), [R.word("=", total)]]).astype(np.uint32)
    rec = np.zeros(1 + -(-total // step), dtype=R.REC)
    rec[0] = (0, 0, 0, 0, 0, step, 1, 0)
    for i, a in enumerate(range(0, total, step)):                         # (the records share the pool's first words)
        rec[1 + i] = (1 + i, 16, 0, a, 0, 0, min(step, total - a), 0)
    want = R.depth(lengths, rec, words, R.options())
    assert want[0] == 2 and (total < 2 or want[1] == 1) and (total < 2 or (want[1:] != want[:-1]).all())
    measure(lengths, rec, words, R.options(), windows)
    # all zero: no runs, or one with report_zero
    none = np.zeros(0, dtype=R.REC), np.zeros(1, dtype=np.uint32)
    for zero in (False, True):
        measure(lengths, none[0], none[1], R.options(report_zero=zero), windows)
    # one covered position per tile
    tiles = -(-total // t)
    rows = [(0, 0, min(k * t + (k * 7) % t, total - 1), 0, [R.word("X", 1)]) for k in range(tiles)]
    rec, words = R.records_of(rows)
    for zero in (False, True):
        measure(lengths, rec, words, R.options(report_zero=zero), windows)


# ------------------------------------------------------------------------------------------------ contention, filters
@gpu
def test_contention_on_one_interval():
    lengths = [300, 1000]
    rec = np.zeros(20_000, dtype=R.REC)
    rec["ref"], rec["pos"], rec["coff"], rec["clen"] = 1, 400, 1, 3                     # every record refers to the same three words
    words = np.array([R.word("=", 9), R.word("=", 60), R.word("X", 1), R.word("=", 39)], dtype=np.uint32)
    cov = F.coverage(lengths=lengths)
    cov.add_records(rec, words)
    cov.finish()
    assert (cov.depth(1, 400, 500) == 20_000).all() and cov.depth(1, 0, 400).max() == 0 and cov.depth(1, 500, 1000).max() == 0 and cov.depth(0, 0, 300).max() == 0
    assert cov.runs().tolist() == [(1, 20_000, 400, 500)]
    assert cov.windows(0).tolist() == [(0, 0, 0, 300, 0, 0), (1, 20_000, 0, 1000, 2_000_000, 100)]
    cov.close()


@gpu
@pytest.mark.parametrize("secondary", [False, True])
@pytest.mark.parametrize("min_mapq", [0, 1, 60])
def test_filters(secondary, min_mapq):
    lengths = [4000]
    rows, at = [], 0
    for flag in (0, 16, 256, 272, 2048, 2064, 4):
        for mapq in (0, 3, 60):
            rows.append((flag, 0, at, mapq, [R.word("=", 50), R.word("X", 2)]))
            at += 100
    rec, words = R.records_of(rows)
    o = R.options(count_secondary=secondary, min_mapq=min_mapq)
    want = R.depth(lengths, rec, words, o)
    counted = [(f, q) for f in (0, 16, 2048, 2064) + ((256, 272) if secondary else ()) for q in (0, 3, 60) if q >= min_mapq]
    assert int(want.sum()) == 52 * len(counted) and want.max() == 1
    measure(lengths, rec, words, o)


# ------------------------------------------------------------------------------------------------ order, lifetime
@gpu
def test_order_of_adds_threads_and_absorb():
    lengths = [5000, 12_345, 70, 9000]
    rng = np.random.default_rng(77)
    rec, words = R.random_records(rng, lengths, 3000, max_words=140)
    o = R.options(count_deletions=True, count_secondary=True)
    want = R.depth(lengths, rec, words, o)
    assert want.max() > 3

    def make():
        return F.coverage(lengths=lengths, options=R.c_options(o))
    one, ten, threaded, into, other = make(), make(), make(), make(), make()
    one.add_records(rec, words)
    for part in np.array_split(np.arange(len(rec)), 10):
        ten.add_records(rec[part], words)
    errors = []

    def work(part):
        try:
            for piece in np.array_split(part, 5):
                threaded.add_records(rec[piece], words)
        except Exception as e:          # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(part,)) for part in np.array_split(np.arange(len(rec)), 4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    into.add_records(rec[:1700], words)
    other.add_records(rec[1700:], words)
    into.absorb(other)
    results = []
    for cov in (one, ten, threaded, into):
        cov.finish()
        same(cov, lengths, want, False)
        results.append((cov.runs().tobytes(), [cov.windows(w).tobytes() for w in WINDOWS]))
    assert all(r == results[0] for r in results)
    other.finish()                                                        # absorbed: left cleared
    assert len(other.runs()) == 0 and int(other.windows(0)["depth_sum"].sum()) == 0
    for cov in (one, ten, threaded, into, other):
        cov.close()


@gpu
def test_absorb_across_pieces():
    """absorb moves an accumulator in pieces of 4 << 20 entries: here its total + 1 entries are one full piece and one piece of 6"""
    piece, tail = 4 << 20, 5
    lengths = [piece + tail]
    rec, words = R.records_across(np.random.default_rng(41), piece, tail)
    o = R.options(count_deletions=True, count_secondary=True)
    want = R.depth(lengths, rec, words, o)
    for half in (rec[::2], rec[1::2]):                                    # both objects hold depth at the ends and on both sides of the piece boundary
        assert R.depth(lengths, half, words, o)[[0, piece - 1, piece, piece + 1, -1]].min() > 0
    into, other = F.coverage(lengths=lengths, options=R.c_options(o)), F.coverage(lengths=lengths, options=R.c_options(o))
    into.add_records(rec[::2], words)
    other.add_records(rec[1::2], words)
    into.absorb(other)
    into.finish()
    same(into, lengths, want, False, windows=(0, 1000))
    other.finish()                                                        # absorbed: left cleared, in both pieces
    assert len(other.runs()) == 0 and int(other.windows(0)["depth_sum"].sum()) == 0 and other.depth(0, 0, lengths[0]).max() == 0
    into.close()
    other.close()


@gpu
def test_lifetime_and_refusals():
    L = capi.lib()
    lengths = [700, 300]
    rec, words = R.records_of([(0, 0, 10, 0, [R.word("=", 100)]), (16, 1, 0, 0, [R.word("=", 300)]), (0, 0, 600, 0, [R.word("=", 50), R.word("D", 50)])])
    cov, twin = F.coverage(lengths=lengths), F.coverage(lengths=lengths)
    cov.add_records(rec, words)
    # one bad record last in a batch of good ones: refused, the depth stays
    for bad in ([(0, 0, 650, 0, [R.word("=", 51)])], [(0, 1, 0, 0, [])], [(0, 2, 0, 0, [R.word("=", 1)])], [(0, 0, 0, 0, [R.word("M", 5)])]):
        rec2, words2 = R.records_of([(0, 0, 0, 0, [R.word("=", 700)])] * 3 + bad)
        with pytest.raises(F.FloxerError):
            cov.add_records(rec2, words2)
    # the copy calls work only behind finish
    with pytest.raises(F.FloxerError):
        cov.runs()
    with pytest.raises(F.FloxerError):
        cov.windows(0)
    with pytest.raises(F.FloxerError):
        cov.depth(0, 0, 10)
    assert L.flx_coverage_num_runs(cov.h) == 0 and L.flx_coverage_num_windows(cov.h, 100) == 7 + 3
    # absorb: other lengths, other options, itself
    for other in (F.coverage(lengths=[700, 301]), F.coverage(lengths=[1000]), F.coverage(lengths=lengths, options=F.coverage_options(count_deletions=True)),
                  F.coverage(lengths=lengths, options=F.coverage_options(report_zero=True))):
        with pytest.raises(F.FloxerError):
            cov.absorb(other)
        with pytest.raises(F.FloxerError):
            other.absorb(cov)
        other.close()
    with pytest.raises(F.FloxerError):
        cov.absorb(cov)
    cov.finish()
    same(cov, lengths, R.depth(lengths, rec, words, R.options()), False)
    # final: add, absorb (either way round) and finish are refused behind finish
    for call in (lambda: cov.add_records(rec, words), lambda: cov.add_records(rec[:0], words), lambda: cov.absorb(twin), lambda: twin.absorb(cov), cov.finish):
        with pytest.raises(F.FloxerError):
            call()
    same(cov, lengths, R.depth(lengths, rec, words, R.options()), False)
    n = L.flx_coverage_num_runs(cov.h)
    assert n == 3
    out = np.zeros(n, dtype=F.RUN_DTYPE)
    assert L.flx_coverage_copy_runs(cov.h, out.ctypes.data_as(C.POINTER(capi.DepthRun)), n - 1) == -3            # FLX_ERR_CAPACITY
    assert L.flx_coverage_copy_runs(cov.h, out.ctypes.data_as(C.POINTER(capi.DepthRun)), n) == 0
    win = np.zeros(2, dtype=F.WINDOW_DTYPE)
    assert L.flx_coverage_copy_windows(cov.h, 0, win.ctypes.data_as(C.POINTER(capi.DepthWindow)), 1) == -3
    with pytest.raises(F.FloxerError):
        cov.depth(0, 0, 701)
    with pytest.raises(F.FloxerError):
        cov.depth(2, 0, 1)
    bad = capi.CoverageOptions()
    bad.reserved[0] = 1
    for make in (lambda: F.coverage(lengths=lengths, options=bad), lambda: F.coverage(lengths=[5, 1 << 31]), lambda: F.coverage(lengths=[])):
        with pytest.raises(F.FloxerError):
            make()
    cov.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def planted():
    from test_md_gpu import RATE, _planted
    chroms, reads = _planted()
    ctx = F.context(F.fmindex(chroms))
    yield dict(chroms=chroms, reads=reads, ctx=ctx, rate=RATE)
    ctx.close()


def run_against_reference(ctx, lengths, runs, o):
    """coverage.add of every run against the reference on the runs' own records and words"""
    cov = F.coverage(ctx, R.c_options(o))
    want = np.zeros(sum(lengths), dtype=np.uint32)
    for run in runs:
        cov.add(run)
        want += R.depth(lengths, run.raw, run.cigars, o)
    cov.finish()
    same(cov, lengths, want, o["report_zero"])
    out = cov.runs().tobytes(), cov.windows(1000).tobytes()
    cov.close()
    return want, out


@gpu
@pytest.mark.parametrize("config", ["default", "selected", "indels"])
def test_pipeline_runs(planted, config):
    chroms, reads, ctx = planted["chroms"], planted["reads"], planted["ctx"]
    lengths = [len(c) for c in chroms]
    p = F.params(error_probability=planted["rate"])
    kw, o = {
        "default": (dict(), R.options()),
        "selected": (dict(output=F.output_options(True, 1, True)), R.options(min_mapq=1, count_deletions=True)),
        "indels": (dict(gaps=F.gap_options(), realign=F.realign_options()), R.options(count_secondary=True)),
    }[config]
    al = F.aligner(ctx, p, **kw)
    whole = al.align_reads(reads)
    half = len(reads) // 2
    want, out = run_against_reference(ctx, lengths, [whole], o)
    want2, out2 = run_against_reference(ctx, lengths, [al.align_reads(reads[:half]), al.align_reads(reads[half:])], o)
    assert (want == want2).all() and out == out2
    flags = {int(f) for f in whole.raw["flag"]}
    assert want.max() >= 2 and 4 in flags and (config == "selected" or 256 in flags or 272 in flags)
    if config == "selected":                                             # the repeats' reads have a small mapping quality: a higher bar leaves them out
        o60 = R.options(min_mapq=60)
        want60, _ = run_against_reference(ctx, lengths, [whole], o60)
        mapped = whole.raw["res"][whole.raw["flag"] & 4 == 0]
        assert (mapped < 60).any() and (mapped == 60).any() and 0 < int(want60.sum()) < int(R.depth(lengths, whole.raw, whole.cigars, R.options(min_mapq=1)).sum())


@gpu
def test_pipeline_raw_runs_and_refusals(planted, monkeypatch):
    chroms, reads, ctx = planted["chroms"], planted["reads"], planted["ctx"]
    lengths = [len(c) for c in chroms]
    L = capi.lib()
    p = F.params(error_probability=planted["rate"])
    pool, offs, n = F._pool_and_offsets(reads)
    monkeypatch.setenv("FLX_CHUNK_READS", "9")                            # several parts, each with its own word pool
    raw = {}
    for mapq in (False, True):
        run = C.c_void_p()
        out_opt = F.output_options(mapq=mapq)
        bundle = capi.RunOptions()
        bundle.output = C.pointer(out_opt)
        capi.check(L.flx_align_reads_opt(ctx.h, C.byref(p), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n, C.byref(bundle), C.byref(run)))
        raw[mapq] = run
    monkeypatch.delenv("FLX_CHUNK_READS")
    result = F.aligner(ctx, p, output=F.output_options(mapq=True)).align_reads(reads)
    for min_mapq in (0, 2):
        o = R.options(min_mapq=min_mapq)
        cov = F.coverage(ctx, R.c_options(o))
        if min_mapq:                                                      # a run made without mapq holds no mapping quality: refused
            with pytest.raises(F.FloxerError, match="mapq"):
                cov.add(raw[False])
        else:
            cov.add(raw[False])
            cov.add(raw[False])
        cov.add(raw[True])
        cov.finish()
        want = R.depth(lengths, result.raw, result.cigars, o)
        same(cov, lengths, want * (1 if min_mapq else 3), False)
        cov.close()
    for run in raw.values():
        L.flx_run_free(run)
    # the same refusal for a RunResult of a run made without mapq; one made with it is taken
    plain = F.aligner(ctx, p).align_reads(reads)
    assert plain.has_mapq is False and result.has_mapq is True
    cov = F.coverage(ctx, F.coverage_options(min_mapq=2))
    with pytest.raises(F.FloxerError, match="mapq"):
        cov.add(plain)
    cov.add(result)
    cov.finish()
    same(cov, lengths, R.depth(lengths, result.raw, result.cigars, R.options(min_mapq=2)), False)
    cov.close()
    # a run made without CIGARs has no depth
    bare = F.aligner(ctx, F.params(error_probability=planted["rate"], without_cigar=True)).align_reads(reads)
    cov = F.coverage(ctx)
    with pytest.raises(F.FloxerError, match="without_cigar"):
        cov.add(bare)
    cov.add(result)
    cov.finish()
    same(cov, lengths, R.depth(lengths, result.raw, result.cigars, R.options()), False)
    cov.close()


@gpu
def test_pipeline_partial_and_split_records():
    from test_tails_gpu import RATE as TAIL_RATE, SPAN, build_batch
    chroms, reads, tailed, rescued = build_batch()
    lengths = [len(c) for c in chroms]
    ctx = F.context(F.fmindex(chroms))
    p = F.params(error_probability=TAIL_RATE)
    al = F.aligner(ctx, p, output=F.output_options(max_alignments=1), partial=F.partial_options(min_query_span=SPAN), extend=F.extend_options(), split=F.split_options())
    whole = al.align_reads(reads)
    clipped = [int(f) for f, o, n in zip(whole.raw["flag"], whole.raw["coff"], whole.raw["clen"]) if n and (int(whole.cigars[o]) & 15) == 4]
    assert any(f & 2048 for f in whole.raw["flag"]) and clipped                                   # records with S and flag 2048
    half = len(reads) // 2
    want, out = run_against_reference(ctx, lengths, [whole], R.options())
    want2, out2 = run_against_reference(ctx, lengths, [al.align_reads(reads[:half]), al.align_reads(reads[half:])], R.options())
    assert (want == want2).all() and out == out2
    ctx.close()


# ------------------------------------------------------------------------------------------------ CLI
def depth_from_sam(text, names, lengths):
    """samtools depth's default filters on the SAM text: flag, POS and CIGAR alone"""
    starts = R.starts_of(lengths)
    diff = np.zeros(int(starts[-1]) + 1, dtype=np.int64)
    n = 0
    for line in text.splitlines():
        if line.startswith("@"):
            continue
        f = line.split("\t")
        if int(f[1]) & (4 | 256):
            continue
        p = int(starts[names.index(f[2])]) + int(f[3]) - 1
        n += 1
        for ln, op in re.findall(r"(\d+)([MIDNSHP=X])", f[5]):
            if op in "=XM":
                diff[p] += 1
                diff[p + int(ln)] -= 1
            if op in "=XMD":
                p += int(ln)
    assert n > 0
    return np.cumsum(diff[:-1]).astype(np.uint32)


def cli_files(planted, tmp_path, tag, *devices):
    from test_md_gpu import letters
    chroms = planted["chroms"]
    reads = [r for r in planted["reads"] if len(r) > 100]
    fasta, fastq = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq")
    with open(fasta, "w") as f:
        for i, c in enumerate(chroms):
            f.write(f">chr{i} planted\n" + "\n".join(letters(c[o: o + 80]) for o in range(0, len(c), 80)) + "\n")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    paths = {k: str(tmp_path / f"{tag}.{e}") for k, e in (("sam", "sam"), ("plain", "plain.sam"), ("bg", "bedgraph"), ("sum", "summary.tsv"), ("win", "windows.tsv"))}
    base = [exe, "--reference", fasta, "--queries", fastq, "--error-probability", str(planted["rate"]), "--threads", "1", "-D", "-N", "1", *devices]
    env = dict(os.environ, FLX_BATCH_READS="16")                          # several batches, dealt to the devices in turn
    for cmd in (base + ["--output", paths["plain"]],
                base + ["--output", paths["sam"], "--coverage", paths["bg"], "--coverage-summary", paths["sum"], "--coverage-windows", paths["win"], "--coverage-window", "100"]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    return {k: open(v, "rb").read() for k, v in paths.items()}


@gpu
def test_cli_coverage_files(planted, tmp_path):
    files = cli_files(planted, tmp_path, "one")
    assert files["sam"] == files["plain"]                                 # the alignment output does not change
    names, lengths = ["chr0", "chr1"], [len(c) for c in planted["chroms"]]
    want = depth_from_sam(files["sam"].decode(), names, lengths)

    def rows(key):
        return [tuple(l.split("\t")) for l in files[key].decode().splitlines()]
    runs = R.runs(lengths, want)
    assert rows("bg") == [(names[r], str(a), str(b), str(d)) for r, d, a, b in runs.tolist()] and len(runs) > 10
    assert rows("sum") == [(names[r], str(b), str(c), str(s), str(m)) for r, m, a, b, s, c in R.windows(lengths, want, 0).tolist()]
    assert rows("win") == [(names[r], str(a), str(b), str(s), str(c), str(m)) for r, m, a, b, s, c in R.windows(lengths, want, 100).tolist()]


@gpu
def test_cli_coverage_files_on_two_devices(planted, tmp_path):
    if capi.lib().flx_device_count() < 2:
        pytest.skip("one HIP device: nothing to sum across")
    one = cli_files(planted, tmp_path, "one")
    two = cli_files(planted, tmp_path, "two", "--devices", "0,1")
    assert one == two
