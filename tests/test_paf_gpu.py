"""PAF summaries on the GPU. The kernel alone (paf_summarise through flx_paf_summarize) against the host rule (flx_paf_summarize_host) and
tests/paf_ref.py on hand-built records around the 64-word pass boundaries and the grid's stride loop; then the records of whole runs in
the planted worlds of test_md_gpu.py, test_partial_gpu.py and test_tails_gpu.py; then the CLI's --paf file against the rule applied to
the SAM text alone. All comparisons are exact."""
import os
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import paf_ref as R

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY_LENS = [5000, 1 << 30, 40_000, 77]
W = R.word


@pytest.fixture(scope="module")
def dev():
    p = F.paf(device=0)
    yield p
    p.close()


def check(dev, rec, words, read_lengths, ref_lens=TOY_LENS):
    """device == host == reference, all fields of all records"""
    want = R.summarize(rec, words, read_lengths, ref_lens)
    host = F.paf_summarize_host(rec, words, read_lengths, ref_lens)
    got = dev.summarize(rec, words, read_lengths, ref_lens)
    assert host.tobytes() == want.tobytes()
    bad = [i for i in range(len(rec)) if got[i] != want[i]]
    assert not bad, (bad[:5], [tuple(got[i]) for i in bad[:5]], [tuple(want[i]) for i in bad[:5]])
    return got


def body(rng, n, max_len=9):
    """n words without S, neighbours with different ops, at least one reference column"""
    ops, prev = [], None
    for _ in range(n):
        op = "=XID"[int(rng.integers(0, 4))]
        while op == prev:
            op = "=XID"[int(rng.integers(0, 4))]
        ops.append(op)
        prev = op
    if not any(op in "=XD" for op in ops):
        ops[0] = "="
        if n > 1 and ops[1] == "=":
            ops[1] = "X"
    return [(op, int(rng.integers(1, max_len + 1))) for op in ops]


def rows_of(kinds):
    """kinds: (flag, ref, [(op, len)]) -> rows for R.records_of at position 3, one read per record, and the reads' lengths"""
    rows, lens = [], []
    for i, (flag, ref, ws) in enumerate(kinds):
        if flag & 4:
            rows.append((4, -1, 0, i, 0, []))
            lens.append(11)
            continue
        rows.append((flag, ref, 3, i, sum(n for op, n in ws if op in "XID"), [W(op, n) for op, n in ws], i % 61))
        lens.append(sum(n for op, n in ws if op in "=XIS"))
    return rows, lens


@gpu
@pytest.mark.parametrize("n_words", [1, 2, 63, 64, 65, 127, 128, 129, 1000])
def test_word_counts_around_the_passes(dev, n_words):
    rng = np.random.default_rng(n_words)
    kinds = []
    for flag in (0, 16, 256, 272, 2048, 2064):
        kinds.append((flag, 2, body(rng, n_words)))
        if n_words >= 2:
            kinds.append((flag, 2, [("S", 5)] + body(rng, n_words - 1)))
            kinds.append((flag, 2, body(rng, n_words - 1) + [("S", 7)]))
        if n_words >= 3:
            kinds.append((flag, 2, [("S", 2)] + body(rng, n_words - 2) + [("S", 13)]))
        kinds.append((4, -1, []))                                         # unmapped records between mapped ones
    rec, words = R.records_of(rows_of(kinds)[0])
    got = check(dev, rec, words, rows_of(kinds)[1])
    assert (got["ref_end"] > 3).sum() == sum(1 for k in kinds if not k[0] & 4) and not got[[i for i, k in enumerate(kinds) if k[0] & 4]].view(np.uint32).any()


@gpu
def test_pass_boundaries_clips_gaps_and_a_long_word(dev):
    eq = lambda n: [("=" if i % 2 == 0 else "X", 1 + i % 5) for i in range(n)]      # n words, = and X in turn
    long_word = (1 << 28) - 1
    kinds = [
        (0, 2, eq(64) + [("S", 9)]),                                     # a trailing S as word 64, alone in its pass
        (16, 2, eq(64) + [("S", 9)]),
        (0, 2, [("S", 4)] + eq(64)),                                     # a leading S followed by 64 words
        (16, 2, [("S", 4)] + eq(64)),
        (0, 2, [("S", 4)] + eq(63) + [("S", 6)]),                         # the trailing S as the second pass's only word, behind a lead
        (0, 2, eq(63) + [("D", 2), ("D", 3)] + eq(10)),                   # D at words 63 and 64: one gap open across the boundary
        (0, 2, eq(63) + [("D", 2), ("I", 3)] + eq(10)),                   # D at 63, I at 64: two
        (0, 2, eq(63) + [("I", 2), ("I", 3), ("D", 1), ("D", 1)]),        # I I D D from word 63 on: two
        (4, -1, []),
        (0, 2, eq(62) + [("D", 2), ("D", 3)] + eq(10)),                   # the same pair inside the first pass
        (0, 2, eq(127) + [("I", 2), ("I", 3)] + eq(3)),                   # and across the second boundary
        (16, 2, [("I", 3)] + eq(64)),                                    # I as first word
        (0, 2, [("S", 3), ("D", 3)] + eq(4)),                             # a gap right behind the lead
        (2064, 1, [("S", 7), ("=", long_word), ("D", 2), ("I", 5), ("X", long_word), ("S", 1)]),      # two words of 2^28 - 1: 64-bit sums
        (0, 1, [("=", long_word)]),
        (0, 3, [("=", 74)]),                                             # ends on its sequence's last base
    ]
    rows, lens = rows_of(kinds)
    rec, words = R.records_of(rows)
    got = check(dev, rec, words, lens)
    assert got["gap_opens"].tolist() == [0, 0, 0, 0, 0, 1, 2, 2, 0, 1, 1, 1, 1, 2, 0, 0]
    assert tuple(got[0])[:2] == (0, lens[0] - 9) and tuple(got[1])[:2] == (9, lens[1]) and tuple(got[2])[:2] == (4, lens[2]) and tuple(got[3])[:2] == (0, lens[3] - 4)
    assert tuple(got[4])[:2] == (4, lens[4] - 6)
    assert int(got[13]["ref_end"]) == 3 + 2 * long_word + 2 and int(got[13]["query_start"]) == 1 and int(got[13]["query_end"]) == lens[13] - 7
    assert int(got[15]["ref_end"]) == 77


@gpu
@pytest.mark.parametrize("n_records", [1, 2, F.grid_caps()["paf_summarise"] + 1])
def test_record_counts_and_the_stride_loop(dev, n_records):
    cap = F.grid_caps()["paf_summarise"]
    rng = np.random.default_rng(n_records)
    n_ops = rng.integers(1, 4, size=n_records)
    kinds = []
    for i in range(n_records):
        ws = body(rng, int(n_ops[i]))
        if i % 5 == 0 and len(ws) < 3:
            ws = [("S", 1 + i % 9)] + ws
        kinds.append(((0, 16, 256, 2048)[i % 4], i % 3, ws) if i % 97 != 96 else (4, -1, []))
    rows, lens = rows_of(kinds)
    rec, words = R.records_of(rows)
    got = check(dev, rec, words, lens)
    assert len(got) == n_records
    if n_records > cap:                                                   # the records behind the grid's waves
        assert got[cap:].view(np.uint32).any()


@gpu
def test_random_records_shared_words_and_a_pool_with_slack(dev):
    rng = np.random.default_rng(2000)
    rec, words, read_lengths = R.random_valid(rng, TOY_LENS[:1] + [3000, 977, 64], 2334, max_words=200)
    lens = TOY_LENS[:1] + [3000, 977, 64]
    assert sum(R.mapped(r) for r in rec) >= 2000 and int(rec["clen"].max()) > 128
    got = check(dev, rec, words, read_lengths, lens)
    # the same records twice over one pool, in another order, with unused words in front of and behind the ones in use
    order = rng.permutation(len(rec))
    rec2 = np.concatenate([rec[order], rec])
    rec2["coff"] += 1000
    words2 = np.concatenate([np.full(1000, W("M", 0), dtype=np.uint32), words, np.full(77, W("N", 3), dtype=np.uint32)])
    got2 = check(dev, rec2, words2, read_lengths, lens)
    assert got2.tobytes() == got[order].tobytes() + got.tobytes()
    assert len(dev.summarize(rec[:0], words, read_lengths, lens)) == 0    # no record: no launch


@gpu
def test_one_invalid_record_refuses_the_batch_and_leaves_the_output(dev):
    rng = np.random.default_rng(12)
    rec, words, read_lengths = R.random_valid(rng, [3000, 977], 300)
    out = np.full(len(rec) * 8, 0x5A5A5A5A, dtype=np.uint32).view(F.PAF_SUMMARY_DTYPE)
    before = out.tobytes()
    victim = [i for i, r in enumerate(rec) if R.mapped(r) and int(r["clen"]) >= 5][-1]
    for what, match in (("interior", "both sides"), ("op", "other than"), ("zero", "length 0"), ("length", "sum to"), ("span", "behind its sequence"), ("read", "read_index")):
        bad, w2, lens2 = rec.copy(), words.copy(), read_lengths.copy()
        at = int(bad[victim]["coff"]) + 2                                # (five words or more: the words on both sides of this one are no clips)
        if what == "interior":
            w2[at] = W("S", int(w2[at]) >> 4)
        elif what == "op":
            w2[at] = W("M", int(w2[at]) >> 4)
        elif what == "zero":
            w2[at] = int(w2[at]) & 15
        elif what == "length":
            lens2[int(bad[victim]["read"])] += 1
        elif what == "span":
            bad[victim]["pos"] = 3000
        else:
            bad[victim]["read"] = len(lens2)
        with pytest.raises(capi.FloxerError, match=match):
            dev.summarize(bad, w2, lens2, [3000, 977], out=out)
        assert out.tobytes() == before, what
    got = dev.summarize(rec, words, read_lengths, [3000, 977], out=out)   # the object is as good as before
    assert got.tobytes() == R.summarize(rec, words, read_lengths, [3000, 977]).tobytes() and out.tobytes() != before


@gpu
def test_calls_from_several_threads_and_a_second_object(dev):
    import threading
    rng = np.random.default_rng(31)
    batches = [R.random_valid(rng, [3000, 977], 200 + 50 * k, max_words=40 + 30 * k) for k in range(4)]
    want = [R.summarize(r, w, l, [3000, 977]).tobytes() for r, w, l in batches]
    other = F.paf(device=0)
    got = [None] * 8

    def work(k):
        r, w, l = batches[k % 4]
        got[k] = (dev if k < 4 else other).summarize(r, w, l, [3000, 977]).tobytes()

    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    other.close()
    assert got == want + want


# ------------------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def runs():
    """name -> (run, read lengths, reference lengths, realigned) over the planted worlds"""
    from test_md_gpu import RATE, _planted
    from test_partial_gpu import RATE as PARTIAL_RATE, mutate
    from test_tails_gpu import SPAN, build_batch
    out = {}
    chroms, reads = _planted()
    ctx = F.context(F.fmindex(chroms))
    lengths, rl = [len(c) for c in chroms], [len(r) for r in reads]
    p = F.params(error_probability=RATE)
    for name, kw in (("default", dict()), ("selected", dict(output=F.output_options(True, 1, True))), ("left_aligned", dict(gaps=F.gap_options())),
                     ("realigned", dict(realign=F.realign_options()))):
        out[name] = (F.aligner(ctx, p, **kw).align_reads(reads), rl, lengths, name == "realigned")
    ctx.close()
    chroms, reads, tailed, rescued = build_batch()
    # a body between two stretches of random letters: too many errors in full, and its partial record is clipped on both sides
    rng = np.random.default_rng(77)
    junk = lambda n: rng.integers(1, 5, size=n, dtype=np.uint8)
    reads = reads + [np.concatenate([junk(1000), mutate(rng, chroms[0][300_000: 304_000], 40), junk(1000)])]
    ctx = F.context(F.fmindex(chroms))
    lengths, rl = [len(c) for c in chroms], [len(r) for r in reads]
    p = F.params(error_probability=PARTIAL_RATE)
    one = F.output_options(max_alignments=1)
    out["partial"] = (F.aligner(ctx, p, output=one, partial=F.partial_options(min_query_span=SPAN)).align_reads(reads), rl, lengths, False)
    out["extended_split"] = (F.aligner(ctx, p, output=one, partial=F.partial_options(min_query_span=SPAN), extend=F.extend_options(), split=F.split_options()).align_reads(reads),
                             rl, lengths, False)
    ctx.close()
    return out


@gpu
@pytest.mark.parametrize("name", ["default", "selected", "left_aligned", "realigned", "partial", "extended_split"])
def test_pipeline_runs(dev, runs, name):
    run, read_lengths, lengths, realigned = runs[name]
    got = check(dev, run.raw, run.cigars, read_lengths, lengths)
    m = np.array([R.mapped(r) for r in run.raw])
    assert m.any() and not got[~m].view(np.uint32).any()
    g, raw = got[m], run.raw[m]
    assert (g["ref_end"].astype(np.int64) - raw["pos"] == g["matches"].astype(np.int64) + g["mismatches"] + g["del_bases"]).all()
    if not realigned:
        assert (raw["nm"] == g["mismatches"] + g["ins_bases"] + g["del_bases"]).all()
    assert (g["query_end"] > g["query_start"]).all() and (g["query_end"] <= np.asarray(read_lengths)[raw["read"].astype(np.int64)]).all()


@gpu
def test_the_runs_hold_every_kind_of_record(runs):
    flags, both = set(), 0
    for run, _, _, _ in runs.values():
        flags |= {int(f) for f in run.raw["flag"]}
        for r in run.raw:
            n, o = int(r["clen"]), int(r["coff"])
            both += n >= 3 and int(run.cigars[o]) & 15 == 4 and int(run.cigars[o + n - 1]) & 15 == 4
    assert any(f & 16 for f in flags) and any(f & 256 for f in flags) and any(f & 2048 for f in flags) and any(f & 4 for f in flags) and both >= 1


# ------------------------------------------------------------------------------------------------ CLI
@gpu
def test_cli_paf_file_from_the_sam_text_alone(tmp_path):
    from test_md_gpu import RATE, _planted, letters
    chroms, reads = _planted()
    reads = [r for r in reads if len(r) > 100]
    fasta, fastq = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq")
    with open(fasta, "w") as f:
        for i, c in enumerate(chroms):
            f.write(f">chr{i} planted\n" + "\n".join(letters(c[o: o + 80]) for o in range(0, len(c), 80)) + "\n")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    base = [exe, "--reference", fasta, "--queries", fastq, "--error-probability", str(RATE), "--threads", "1", "--cs-tag", "-Q", "-D"]
    env = dict(os.environ, FLX_BATCH_READS="16")                          # several batches

    def run(*extra):
        r = subprocess.run(base + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()

    x_sam, x_paf, plain, alone = (str(tmp_path / n) for n in ("x.sam", "x.paf", "plain.sam", "alone.paf"))
    run("--output", x_sam, "--paf", x_paf, "--paf-cigar")
    run("--output", plain)
    run("--paf", alone, "--paf-cigar")
    sam = open(x_sam, "rb").read()
    assert sam == open(plain, "rb").read()                                # the alignment output does not change
    names, lengths = ["chr0", "chr1"], [len(c) for c in chroms]
    want = R.from_sam(sam.decode(), names, lengths, R.options(write_cigar=True, mapq_from_records=True))
    got = open(x_paf, "rb").read()
    assert got == want and got == open(alone, "rb").read()
    lines = got.decode().splitlines()
    assert len(lines) >= 40 and all(l.count("\tcg:Z:") == 1 and l.count("\tcs:Z:") == 1 and "\tde:f:" in l for l in lines)
    assert {l.split("\t")[4] for l in lines} == {"+", "-"} and {l.split("\t")[12] for l in lines} == {"tp:A:P", "tp:A:S"}
    assert any(l.split("\t")[11] not in ("0", "255") for l in lines)      # -Q: the column comes from the records
    assert sorted(os.listdir(tmp_path)) == sorted(["ref.fasta", "reads.fastq", "x.sam", "x.paf", "plain.sam", "alone.paf"])
