"""Error profile on the GPU (flx_errprof: kernel errprof_add, runs, the Python class and the CLI's --error-profile output). Every expected
table is the plain-numpy rule of tests/errprof_ref.py on the same text, records, words and reads, compared entry for entry; the shapes sit
on the kernel's boundaries: 64 CIGAR words per pass, 64 columns between a lane's word and the whole wave's, the flush between records."""
import ctypes as C
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
from floxer_amd import simulate as S
import errprof_cases as K
import errprof_ref as R

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = R.options()


def measure(text, lengths, rec, words, reads, o=NONE, adds=1, flush_threshold=0, want=None):
    p = F.errprof(text=text, lengths=lengths, options=R.c_options(o, flush_threshold))
    try:
        for part in np.array_split(np.arange(len(rec)), adds):
            p.add_records(rec[part], words, reads)
        got = p.table()
    finally:
        p.close()
    want = R.table(text, lengths, rec, words, reads, o) if want is None else want
    assert R.same(got, want)[:12] == []
    return got


# ------------------------------------------------------------------------------------------------ words and carries
def body_words(rng, n, max_len=9):
    """n words: = runs with X, I and D between them, words of each op on both sides of every pass boundary; the first and the last consume
    reference"""
    ws = [("=" if t % 2 == 0 else "XID"[int(rng.integers(0, 3))], int(rng.integers(1, max_len + 1))) for t in range(n)]
    for k, t in enumerate((62, 63, 64, 65, 126, 127, 128, 129, 4094, 4095, 4096)):
        if t < n:
            ws[t] = ("XIDX=IDX=ID"[k], ws[t][1])
    if ws[0][0] == "I":
        ws[0] = ("X", ws[0][1])
    if ws[-1][0] == "I":
        ws[-1] = ("X", ws[-1][1])
    return [(op, ln, None) for op, ln in ws]


@gpu
@pytest.mark.parametrize("n_words", [1, 63, 64, 65, 129, 4097])
def test_words_and_carries(n_words):
    rng = np.random.default_rng(n_words)
    lengths = [45_000, 33_000]
    text = R.random_text(rng, lengths)
    body = body_words(rng, n_words)
    inner = body_words(rng, max(1, n_words - 2))
    clipped = ([("S", 7, None)] + inner + [("S", 5, None)]) if n_words >= 3 else inner          # the row carry starts at 7
    d_inner = body_words(rng, max(1, n_words - 4))
    d_ends = ([("S", 3, None), ("D", 3, None)] + d_inner + [("D", 4, None), ("S", 2, None)]) if n_words >= 5 else [("D", 3, None)] + d_inner + [("D", 4, None)]
    span = lambda ops: sum(n for op, n, _ in ops if op in "=XD")  # noqa: E731
    cases = [(0, 0, 1011, body), (16, 0, 2000, body), (16, 1, 0, clipped), (0, 1, 5, clipped),
             (2048, 0, 45_000 - span(d_ends), d_ends),                                            # a D as first and as last reference word; ends on the sequence's last position
             (16, 1, 33_000 - span(body), body)]
    assert len(body) == n_words and (n_words < 3 or len(clipped) == n_words) and all(span(c[3]) <= 33_000 for c in cases)
    rec, words, reads = K._assemble(text, lengths, cases)
    got = measure(text, lengths, rec, words, reads)
    assert int(got["TOTALS"][0]) == 6 and int(got["PAIR_EQ"].sum()) == int(got["TOTALS"][1]) > 0
    if n_words >= 65:
        assert [op for op, _, _ in body[62:65]] == list("XID")             # words of other ops on both sides of a pass boundary
        assert int(got["HP_INS"].sum()) > 3 and int(got["HP_DEL"].sum()) > 3 and int(got["PAIR_X"].sum()) > 10
    measure(text, lengths, rec, words, reads, adds=3)


@gpu
@pytest.mark.parametrize("length", [63, 64, 65, 4097])
def test_word_lengths_on_both_sides_of_the_wave_path(length):
    """a word of 64 columns or more is walked by the whole wave, a shorter one by its own lane: every op at 63, 64, 65 and 4097, two long
    words in one pass, a long word as the last of a record, long words next to short ones"""
    rng = np.random.default_rng(length)
    lengths = [30_000, 9000]
    text = R.random_text(rng, lengths)
    text[20_000: 20_000 + 4200] = 3                                        # a run of G: a uniform D and a uniform I of every length
    n = length
    e = ("=", 5, None)
    cases = []
    for flag in (0, 16):
        cases += [(flag, 0, 100, [("=", n, None)]), (flag, 0, 300, [("X", n, None)]), (flag, 0, 500, [e, ("I", n, None), e]), (flag, 0, 700, [e, ("D", n, None), e]),
                  (flag, 1, 50, [("S", n, None), e, ("S", n, None)]),
                  (flag, 0, 20_000, [e, ("D", n, None), e]), (flag, 0, 19_990, [("=", 12, None), ("I", n, [3] * n), e]),      # uniform: bin 32; the I scans both sides
                  (flag, 0, 5000, [("=", n, None), ("X", n, None), ("I", n, None), ("D", n, None), ("S", n, None)]),            # several long words in one pass, the last one long
                  (flag, 0, 9000, [("S", 2, None), ("=", n, None), ("I", 1, None), ("X", n, None), ("D", 2, None), ("=", 3, None), ("X", n, None)]),
                  (flag, 1, 0, [("I", n, [1] * n), ("=", 4, None), ("I", n, [5] * n), ("D", 1, None), ("I", n, [1, 2] * (n // 2) + [1] * (n % 2))])]
    rec, words, reads = K._assemble(text, lengths, cases)
    got = measure(text, lengths, rec, words, reads)
    assert int(got["EQ_RUN"][min(n, 256) - 1]) >= 4 and int(got["INS_LEN"][min(n, 64) - 1]) >= 10 and int(got["DEL_LEN"][min(n, 64) - 1]) >= 6
    assert int(got["HP_DEL"][32]) >= 2 and int(got["HP_INS"][32]) >= 2 and int(got["HP_INS"][33]) >= 4


# ------------------------------------------------------------------------------------------------ the host test's cases
@gpu
@pytest.mark.parametrize("length", K.POSITION_LENGTHS)
def test_position_bins(length):
    text, lengths, rec, words, reads = K.position_case(length)
    K.check_position_case(length, measure(text, lengths, rec, words, reads))


@gpu
def test_homopolymer_bins():
    text, lengths, rec, words, reads, expected = K.homopolymer_case()
    got = measure(text, lengths, rec, words, reads)
    for section in ("HP_DEL", "HP_INS"):
        bins = [b for s, b in expected if s == section]
        assert [int(got[section][b]) for b in sorted(set(bins))] == [bins.count(b) for b in sorted(set(bins))]
    p = F.errprof(text=text, lengths=lengths)
    for i, (section, index) in enumerate(expected):                      # one record at a time: the table grows by that record's bin
        before = p.table()[section]
        p.add_records(rec[i: i + 1], words, reads)
        after = p.table()[section]
        assert int(after[index]) == int(before[index]) + 1 and int(after.sum()) == int(before.sum()) + 1, (i, section, index)
    p.close()


@gpu
def test_a_read_against_itself_and_its_reverse_complement():
    rng = np.random.default_rng(9)
    seq = rng.integers(1, 5, size=5000).astype(np.uint8)
    seq[100:103] = 5
    rc = R.oriented(seq, 16)
    w = [R.word("=", 5000)]
    for text, flag in ((seq, 0), (rc, 16)):
        rec, words = R.records_of([(flag, 0, 0, 0, w)])
        got = measure(text, [5000], rec, words, [seq])                    # flag 16: the read's reverse complement is walked against the reverse-complemented text
        diag = got["PAIR_EQ"].reshape(6, 6)
        assert int(np.trace(diag)) == 5000 == int(diag.sum()) and int(diag[5, 5]) == 3 and int(got["IDENTITY"][100]) == 1
        assert (got["POS_MATCH"] == 50).all() and int(got["EQ_RUN"][255]) == 1
    assert (measure(seq, [5000], *R.records_of([(0, 0, 0, 0, w)]), [seq])["PAIR_EQ"].reshape(6, 6) ==
            measure(rc, [5000], *R.records_of([(16, 0, 0, 0, w)]), [seq])["PAIR_EQ"].reshape(6, 6)[[0, 4, 3, 2, 1, 5]][:, [0, 4, 3, 2, 1, 5]]).all()


# ------------------------------------------------------------------------------------------------ contention, flushes, filters
def shared_record(n):
    """n records on the same words and the same read"""
    rng = np.random.default_rng(2)
    lengths = [300, 1000]
    text = R.random_text(rng, lengths)
    rec1, words, reads = K._assemble(text, lengths, [(16, 1, 400, [("S", 4, None), ("=", 70, None), ("I", 3, None), ("X", 1, None), ("D", 2, None), ("=", 39, None), ("I", 66, None), ("X", 2, None)])])
    rec = np.repeat(rec1, n)
    return text, lengths, rec, words, reads


@gpu
def test_contention_on_one_record():
    n = 20_000
    text, lengths, rec, words, reads = shared_record(n)
    one = R.table(text, lengths, rec[:1], words, reads, NONE)
    got = measure(text, lengths, rec, words, reads, want=R.times(one, n))          # (the table is a sum over the records)
    assert int(got["TOTALS"][0]) == n and int(got["PAIR_EQ"].sum()) == 109 * n


@gpu
def test_a_flush_between_every_two_records_changes_nothing():
    rng = np.random.default_rng(12)
    lengths = [5000, 12_345, 70, 9000]
    text = R.random_text(rng, lengths)
    rec, words = R.random_records(rng, lengths, 6000, max_words=40)          # more records than the grid has waves: a wave takes several
    reads = R.fitted_reads(rng, text, lengths, rec, words)
    want = R.table(text, lengths, rec, words, reads, NONE)
    default = measure(text, lengths, rec, words, reads, want=want)
    every = measure(text, lengths, rec, words, reads, want=want, flush_threshold=1)
    some = measure(text, lengths, rec, words, reads, want=want, flush_threshold=300)
    assert R.same(default, every) == [] and R.same(default, some) == []
    text, lengths, rec, words, reads = shared_record(20_000)
    want = R.times(R.table(text, lengths, rec[:1], words, reads, NONE), 20_000)
    measure(text, lengths, rec, words, reads, want=want, flush_threshold=1)


@gpu
@pytest.mark.parametrize("secondary", [False, True])
@pytest.mark.parametrize("min_mapq", [0, 1, 60])
def test_filters(secondary, min_mapq):
    lengths = [4000]
    text = R.random_text(np.random.default_rng(1), lengths)
    cases, mapqs = [], []
    for flag in (0, 16, 256, 272, 2048, 2064, 4):
        for mapq in (0, 3, 60):
            cases.append((flag, 0, 100 * len(cases), [("=", 50, None), ("X", 2, None), ("I", 1, None), ("D", 2, None)]))
            mapqs.append(mapq)
    rec, words, reads = K._assemble(text, lengths, cases)
    rec["res"] = mapqs
    o = R.options(count_secondary=secondary, min_mapq=min_mapq)
    got = measure(text, lengths, rec, words, reads, o)
    counted = [(f, q) for f in (0, 16, 2048, 2064) + ((256, 272) if secondary else ()) for q in (0, 3, 60) if q >= min_mapq]
    assert [int(x) for x in got["TOTALS"]] == [len(counted) * k for k in (1, 50, 2, 1, 1, 1, 2, 0)]


# ------------------------------------------------------------------------------------------------ order, threads, absorb, lifetime
@gpu
def test_order_of_adds_threads_and_absorb():
    lengths = [5000, 12_345, 70, 9000]
    rng = np.random.default_rng(77)
    text = R.random_text(rng, lengths)
    rec, words = R.random_records(rng, lengths, 3000, max_words=140)
    reads = R.fitted_reads(rng, text, lengths, rec, words)
    o = R.options(count_secondary=True)
    want = R.table(text, lengths, rec, words, reads, o)

    def make(flush=0):
        return F.errprof(text=text, lengths=lengths, options=R.c_options(o, flush))
    one, three, threaded, into, other = make(), make(), make(), make(), make(flush=50)
    one.add_records(rec, words, reads)
    for part in np.array_split(np.arange(len(rec)), 3):
        three.add_records(rec[part], words, reads)
    errors = []

    def work(part):
        try:
            for piece in np.array_split(part, 5):
                threaded.add_records(rec[piece], words, reads)
        except Exception as e:          # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(part,)) for part in np.array_split(np.arange(len(rec)), 4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors
    into.add_records(rec[:1700], words, reads)
    assert R.same(into.table(), R.table(text, lengths, rec[:1700], words, reads, o)) == []          # the sums so far, at any time
    other.add_records(rec[1700:], words, reads)
    into.absorb(other)
    for p in (one, three, threaded, into):
        assert R.same(p.table(), want)[:12] == []
    assert R.same(other.table(), R.empty()) == []                         # absorbed: left cleared
    other.add_records(rec[:5], words, reads)                              # .. and usable
    assert R.same(other.table(), R.table(text, lengths, rec[:5], words, reads, o)) == []
    # absorb: other lengths, other options, itself
    for bad in (F.errprof(text=text[:-1], lengths=lengths[:-1] + [lengths[-1] - 1]), F.errprof(text=text, lengths=lengths), F.errprof(text=text, lengths=lengths, options=R.c_options(dict(o, min_mapq=2)))):
        with pytest.raises(F.FloxerError):
            one.absorb(bad)
        with pytest.raises(F.FloxerError):
            bad.absorb(one)
        bad.close()
    with pytest.raises(F.FloxerError):
        one.absorb(one)
    # a refused add leaves the table as it was
    bad_rec, bad_words, bad_reads = K._assemble(text, lengths, [(0, 0, 0, [("=", 700, None)])] * 3 + [(0, 2, 60, [("=", 11, None)])])
    with pytest.raises(F.FloxerError, match="behind its sequence"):
        one.add_records(bad_rec, bad_words, bad_reads)
    assert R.same(one.table(), want) == []
    for make_bad in (lambda: F.errprof(text=np.array([1, 2, 6], dtype=np.uint8), lengths=[3]), lambda: F.errprof(text=text, lengths=lengths, options=F.errprof_options(flush_threshold=(1 << 31) + 1)),
                     lambda: F.errprof(text=text, lengths=[]), lambda: F.errprof()):
        with pytest.raises(F.FloxerError):
            make_bad()
    for p in (one, three, threaded, into, other):
        p.close()


# ------------------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def sample():
    chroms = S.make_genome(20_000, 2, seed=31)
    reads = S.make_reads(chroms, 240, 1000, 0.04, seed=32)[0]
    ctx = F.context(F.fmindex(chroms))
    yield dict(chroms=chroms, reads=reads, ctx=ctx, rate=0.05)
    ctx.close()


def raw_run(ctx, p, reads):
    """an unfreed flx_run handle of host reads or of a resident batch"""
    L = capi.lib()
    run = C.c_void_p()
    if isinstance(reads, F.resident_reads):
        capi.check(L.flx_align_reads_resident(ctx.h, C.byref(p), reads.h, C.byref(run)))
    else:
        pool, offs, n = F._pool_and_offsets(reads)
        capi.check(L.flx_align_reads(ctx.h, C.byref(p), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n, C.byref(run)))
    return run


@gpu
def test_pipeline_runs_host_and_resident_reads_and_both_creates(sample, monkeypatch):
    chroms, reads, ctx = sample["chroms"], sample["reads"], sample["ctx"]
    lengths = [len(c) for c in chroms]
    text = np.concatenate(chroms)
    L = capi.lib()
    p = F.params(error_probability=sample["rate"])
    result = F.aligner(ctx, p).align_reads(reads)
    want = R.table(text, lengths, result.raw, result.cigars, reads, NONE)
    assert int(want["TOTALS"][0]) >= len(reads) and int(want["TOTALS"][2]) > 0 and int(want["TOTALS"][3]) > 0 and int(want["TOTALS"][5]) > 0
    assert int(want["PAIR_EQ"].reshape(6, 6).sum() - np.trace(want["PAIR_EQ"].reshape(6, 6))) == 0          # this aligner's = columns hold equal letters
    resident = F.resident_reads(ctx, reads)
    monkeypatch.setenv("FLX_CHUNK_READS", "50")                           # several parts, each with its own word pool
    runs = [raw_run(ctx, p, reads), raw_run(ctx, p, resident)]
    monkeypatch.delenv("FLX_CHUNK_READS")
    for make in (lambda: F.errprof(ctx), lambda: F.errprof(text=chroms)):                              # the context's padded text in HBM, and a text of its own
        e = make()
        e.add(result, reads)
        assert R.same(e.table(), want)[:12] == []
        e.close()
        for run, given in ((runs[0], reads), (runs[1], resident), (runs[0], resident), (runs[1], reads)):
            e = make()
            if isinstance(given, F.resident_reads):
                e.add_resident(run, given)
            else:
                e.add(run, given)
            assert R.same(e.table(), want)[:12] == []
            e.close()
    # a read batch that does not fit the run's records is refused, the table stays; min_mapq needs a run made with mapq
    e = F.errprof(ctx)
    with pytest.raises(F.FloxerError):
        e.add(runs[0], reads[:-1] + [reads[-1][:-1]])
    with pytest.raises(F.FloxerError, match="read_index"):
        e.add(runs[0], reads[:5])
    assert R.same(e.table(), R.empty()) == []
    q = F.errprof(ctx, F.errprof_options(min_mapq=2))
    for run in (runs[0], result):
        with pytest.raises(F.FloxerError, match="mapq"):
            q.add(run, reads)
    q.close()
    # a run made without CIGARs has no profile
    bare = F.aligner(ctx, F.params(error_probability=sample["rate"], without_cigar=True)).align_reads(reads)
    with pytest.raises(F.FloxerError, match="without_cigar"):
        e.add(bare, reads)
    for run in runs:
        L.flx_run_free(run)
    resident.close()
    # the context stays while a profile object reads its text
    assert L.flx_ctx_destroy(ctx.h) == -1 and "error-profile" in L.flx_last_error().decode()
    e.close()


# ------------------------------------------------------------------------------------------------ CLI
def table_from_sam(sam, fasta_seqs, names, fastq_reads):
    """the rule on the run's files alone: FLAG, RNAME, POS, MAPQ and CIGAR from the SAM text, the reads from the FASTQ (as given: the walk
    orients them by flag bit 16), the text from the FASTA"""
    rows, reads = [], []
    for line in sam.splitlines():
        if line.startswith("@"):
            continue
        f = line.split("\t")
        flag = int(f[1])
        if flag & 4:
            continue
        assert "M" not in f[5]
        ws = [R.word(op, int(ln)) for ln, op in re.findall(r"(\d+)([MIDNSHP=X])", f[5])]
        rows.append((flag, names.index(f[2]), int(f[3]) - 1, int(f[4]), ws))
        reads.append(fastq_reads[f[0]])
    assert rows
    rec, words = R.records_of(rows)
    return R.table(np.concatenate(fasta_seqs), [len(s) for s in fasta_seqs], rec, words, reads, NONE), rec, words


@gpu
@pytest.mark.parametrize("partial", [False, True])
def test_cli_error_profile_file(tmp_path, partial):
    from test_md_gpu import letters
    if partial:
        from test_tails_gpu import RATE as rate, SPAN, build_batch
        chroms, reads = build_batch()[:2]
        more = ["--partial-alignments", "--partial-min-span", str(SPAN)]
    else:
        chroms = S.make_genome(20_000, 2, seed=41)
        reads = S.make_reads(chroms, 200, 1000, 0.04, seed=42)[0]
        rate, more = 0.05, []
    fasta, fastq = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq")
    with open(fasta, "w") as f:
        for i, c in enumerate(chroms):
            f.write(f">chr{i} sample\n" + "\n".join(letters(c[o: o + 80]) for o in range(0, len(c), 80)) + "\n")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    paths = {k: str(tmp_path / e) for k, e in (("sam", "with.sam"), ("plain", "plain.sam"), ("tsv", "profile.tsv"))}
    base = [exe, "--reference", fasta, "--queries", fastq, "--error-probability", str(rate), "--threads", "1", "-D", "-N", "1", *more]
    env = dict(os.environ, FLX_BATCH_READS="64")                          # several batches
    for cmd in (base + ["--output", paths["plain"]], base + ["--output", paths["sam"], "--error-profile", paths["tsv"]]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    files = {k: open(v, "rb").read() for k, v in paths.items()}
    assert files["sam"] == files["plain"]                                 # the alignment output does not change
    names = [f"chr{i}" for i in range(len(chroms))]
    by_name = {f"read{i}": np.asarray(r, dtype=np.uint8) for i, r in enumerate(reads)}
    want, rec, words = table_from_sam(files["sam"].decode(), [np.asarray(c, dtype=np.uint8) for c in chroms], names, by_name)
    assert files["tsv"] == R.tsv(want)
    lines = files["tsv"].decode().splitlines()
    assert lines[-1] == "summary\teq_columns_unequal\t0" and int(lines[-6].split("\t")[2]) > 10_000 and 0 < int(lines[-5].split("\t")[2]) < 200_000
    if partial:
        assert any(int(f) & 2048 for f in rec["flag"]) and int(want["TOTALS"][7]) > 0 and int(want["POS_CLIP"].sum()) > 0      # S words and supplementary records occur
