"""Left-aligned indels on the GPU. The kernel alone (cigar_left_align through flx_left_align_batch) against the host rule (flx_left_align)
and the Python rule of leftalign_ref.py on the smallest shapes that can go wrong; then behind K5 on cases of the alignment corpus
(flx_align_batch_gaps with MD); then the whole path on a repeat-rich reference: option on = option off with the rule applied to every
CIGAR, MD following, off is off, every way the reads come in, a context without host text, and the CLI. Needs an MI355X (-m gpu)."""
import os
import random
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import simulate as S
import align_corpus as AC
import leftalign_ref as R
from leftalign_ref import D, EQ, I, X
from test_md_host import bam_records, cigar_words, md_from_cigar
from test_extend_gpu import sa_strings
from test_partial_gpu import check_record

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 0.08
LETTERS = "NACGTN"


def letters(r):
    return "".join(LETTERS[int(x)] for x in r)


# ------------------------------------------------------------------------------------------------ the kernel alone
def spell(path, ref_of, other, begin=0, tail=0):
    """letters that make the path true over a reference given by column: ref_of(col); = copies the column, X takes other(letter), I takes
    the letters of the columns it stands in front of (so a periodic reference gives a periodic query when the I is whole periods long)"""
    cols = begin + sum(ln for op, ln in path if op != I) + tail
    ref = [ref_of(c) for c in range(cols)]
    qry, r = [], begin
    for op, ln in path:
        if op == EQ:
            qry += ref[r: r + ln]
        elif op == X:
            qry += [other(x) for x in ref[r: r + ln]]
        elif op == I:
            qry += [ref_of(r + i) for i in range(ln)]
        if op != I:
            r += ln
    return path, np.array(ref, dtype=np.uint8), np.array(qry, dtype=np.uint8), begin


def mono(path, letter=1, **kw):
    return spell(path, lambda c: letter, lambda x: (x % 4) + 1 if x else 3, **kw)


def periodic(path, unit=(1, 2, 3), **kw):
    return spell(path, lambda c: unit[c % len(unit)], lambda x: 4, **kw)


def filler(n_words, gaps):
    """n_words words, = (2 columns) and X (1) in turn, with the gap words `gaps` {index: (op, length)} in place of what stood there"""
    return [gaps.get(t, (EQ, 2) if t % 2 == 0 else (X, 1)) for t in range(n_words)]


def kernel_cases():
    """[(class, name, (path, ref, qry, begin))]; every class but 'still' must move a gap"""
    c = []
    add = lambda cls, name, case: c.append((cls, name, case))
    add("homopolymer", "1-column D at the right end of 7 letters", (R.parse("7=1D2="), *map(np.array, (list(b"AAAAAAAACG"), list(b"AAAAAAACG"))), 0))
    add("homopolymer", "1-row I at the right end of 7 letters", (R.parse("7=1I2="), *map(np.array, (list(b"AAAAAAACG"), list(b"AAAAAAAACG"))), 0))
    add("period3", "D of 3", periodic(R.parse("1X9=3D2=1X")))
    add("period3", "D of 6", periodic(R.parse("1X9=6D2=1X")))
    add("period3", "a shift that is no multiple of the period", (R.parse("1X1=8=3D2="), *map(np.array, (list(b"TTCGACGACGACGAC"), list(b"GTCGACGACGAC"))), 0))
    add("consume_x", "the run consumed exactly, then X", mono(R.parse("2=1X3=1D1=")))
    add("consume_other", "the run consumed exactly, then the other kind", mono(R.parse("2=1I3=1D1=")))
    add("consume_other", "and the other way round", mono(R.parse("2=1D3=1I1=")))
    add("merge_stop", "same kind: merge and stop", mono(R.parse("1=1X1D2=1D1=")))
    add("merge_on", "same kind: merge and go on", mono(R.parse("3=1D2=1D1=")))
    add("merge_on", "three of a kind, then a first-word gap", mono(R.parse("2D3=1D2=1D1=")))
    add("first_word", "3= 2D", mono(R.parse("3=2D")))
    add("grow", "a gap followed by X", periodic(R.parse("5=2D1X"), unit=(1, 2)))
    add("grow", "a gap followed by another gap", mono(R.parse("4=1D1I2=")))
    add("grow", "an I followed by X", mono(R.parse("4=1I1X")))
    add("2nm1", "2 NM + 1 words before and after", periodic([(EQ, 2), (D, 1)] * 20 + [(EQ, 2)], unit=(1, 2, 2)))
    for n in (64, 65, 128, 129, 200):
        for at in (63, 64, 65):
            if at < n - 1:
                add("long_paths", f"{n} words, a gap word at index {at}", mono(filler(n, {at: (D if at % 2 else I, 2), at - 1: (EQ, 2), at + 1: (EQ, 2)})))
        add("long_paths", f"{n} words, gaps at 63, 64 and 65", mono(filler(max(n, 67), {62: (EQ, 3), 63: (D, 1), 64: (EQ, 3), 65: (I, 2), 66: (EQ, 2)})[:n]))
    add("chain", "= D = I = D = I ..., every shift bounded by the one before, over three passes", mono([(X, 1)] + [(EQ, 3), (D, 1), (EQ, 3), (I, 1)] * 40 + [(EQ, 2)]))
    add("chain", "the same with barriers", mono([(X, 1)] + ([(EQ, 3), (D, 1), (EQ, 3), (I, 1)] * 6 + [(EQ, 2), (X, 1)]) * 8))
    add("chain_merge", "= D = D = D ...: all merge into one, over three passes", mono([(X, 1)] + [(EQ, 3), (D, 1)] * 70 + [(EQ, 2)]))
    add("long_shift", "more than 64 columns", periodic(R.parse("1X70=3D5=1X")))
    add("long_shift", "more than 1100 columns in a 1500-column tandem region", periodic(R.parse("1X1200=6D290=1X")))
    add("long_shift", "two long shifts in one pass", periodic(R.parse("1X300=3D1X400=2I6=")))
    add("long_i", "I of 700 rows in a periodic query", periodic(R.parse("1X800=700I10=1X"), unit=(1, 2, 3, 4, 1, 1, 2)))
    add("ranks", "letters of rank 0", mono(R.parse("1X5=1D2=1I3="), letter=0))
    add("ranks", "letters of rank 5", mono(R.parse("1X5=1D2=1I3="), letter=5))
    # input that is not in normal form: neighbouring words of one op merge, in slabs that hold exactly what the rule can write
    add("same_op", "2=2=1X1X1D1D2=", (R.parse("2=2=1X1X1D1D2="), *map(np.array, (list(b"ACGTAAAAAA"), list(b"ACGTCCAA"))), 0))
    add("same_op", "= = then a gap that crosses both", mono(R.parse("1X2=3=1D2=")))
    add("same_op", "1D1D", mono(R.parse("1D1D")))
    add("same_op", "I I behind a run", mono(R.parse("4=1I2I1=")))
    add("same_op", "X X over the pass boundary, a gap behind", mono(filler(63, {}) + [(X, 1), (X, 2), (EQ, 3), (D, 1), (D, 1), (EQ, 1)]))
    add("still", "1X1X", mono(R.parse("1X1X")))
    add("still", "5=1X1X", mono(R.parse("5=1X1X")))
    add("still", "3=1X1X1X", mono(R.parse("3=1X1X1X")))
    add("still", "a one-word path", mono(R.parse("9=")))
    add("still", "a one-word path: a gap", mono(R.parse("3D")))
    add("still", "an all-I path", (R.parse("4I"), np.zeros(0, np.uint8), np.array([1, 1, 1, 1], np.uint8), 0))
    add("still", "nothing in front of the gap but X", mono(R.parse("1X2D4=")))
    return c


@pytest.fixture(scope="module")
def ctx():
    c = F.context(F.fmindex([np.random.default_rng(5).integers(1, 5, size=2000).astype(np.uint8)]))
    yield c
    c.close()


def run_kernel(ctx, cases):
    ref, qry, words, jobs = R.pack_jobs(cases)
    got = [R.path_of(w) for w in F.left_align_batch(ctx, qry, words, jobs, reference_pool=ref)]
    host = [R.path_of(w) for w in F.left_align(ref, qry, words, jobs)]
    return got, host


@gpu
def test_kernel_matches_the_rule_on_the_smallest_shapes_that_can_go_wrong(ctx):
    named = kernel_cases()
    cases = [c for _, _, c in named]
    got, host = run_kernel(ctx, cases)
    moved, grown = set(), 0
    for (cls, name, c), g, h in zip(named, got, host):
        want = R.left_align(*c)
        assert h == want, (name, R.show(h), R.show(want))
        assert g == want, (name, R.show(g)[:200], R.show(want)[:200])
        R.check_properties(*c, g)
        if g != c[0] and not (cls == "still" and R.normal_form(g) and not R.normal_form(c[0])):      # (still: words merge, no gap moves)
            moved.add(cls)
        grown += len(g) > len(c[0])
    # the data does what it is about: every class moves a gap, some path grows, the still ones stay
    assert moved == {cls for cls, _, _ in named} - {"still"}, moved
    assert grown >= 3
    by_name = {name: g for (_, name, _), g in zip(named, got)}
    assert R.show(by_name["1-column D at the right end of 7 letters"]) == "1=1D8=" and R.show(by_name["3= 2D"]) == "1=2D2="
    assert R.show(by_name["a gap followed by X"]) == "1=2D4=1X"
    assert R.show(by_name["= D = D = D ...: all merge into one, over three passes"]) == "1X70D212="
    assert R.show(by_name["more than 1100 columns in a 1500-column tandem region"]) == "1X6D1490=1X"
    assert R.show(by_name["I of 700 rows in a periodic query"]) == "1X700I810=1X"
    assert len(by_name["2 NM + 1 words before and after"]) == 41
    assert [R.show(by_name[n]) for n in ("1X1X", "5=1X1X", "3=1X1X1X", "1D1D", "2=2=1X1X1D1D2=")] == ["2X", "5=2X", "3=3X", "2D", "4=2X2D2="]


@gpu
def test_kernel_counts_the_gap_words_that_moved_or_merged(ctx):
    """the launch's work units are the gap words that moved or merged (DevLeftAlignStat::moved), counted here by the Python rule: a gap
    word counts when it shifts at least one column or joins a gap word of its kind in front of it. The cases hold gap words that merge
    without shifting (the word-by-word form of a pass), that shift without merging (both forms) and that do neither."""
    cases = [c for _, _, c in kernel_cases()]
    want, kinds = 0, set()
    for c in cases:
        gaps = []
        R.left_align(*c, gaps=gaps)
        assert len(gaps) == sum(op in (I, D) for op, _ in c[0])
        want += sum(1 for shift, merged in gaps if shift or merged)
        kinds |= {(shift > 0, merged) for shift, merged in gaps}
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}, kinds      # not vacuous, on the rule alone
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_stats()
    run_kernel(ctx, cases)
    st = ctx.kernel_stats()
    ctx.enable_kernel_timing(False)
    assert list(st) == ["cigar_left_align"] and st["cigar_left_align"]["launches"] == 1
    assert st["cigar_left_align"]["work_units"] == want, (st["cigar_left_align"]["work_units"], want)


@gpu
def test_kernel_random_paths_in_one_launch_and_bad_jobs_launch_nothing(ctx):
    cases = R.random_corpus(29, 3000) + R.random_corpus(37, 3000, repeats=True)      # the second half: neighbouring words of one op
    rng = random.Random(31)
    for n in (70, 130, 200, 260, 400):                                   # long ones among them: the fast and the serial form of a pass in turn
        cases.append(R.random_path(rng, n, alphabet=2, max_len=4))
        cases.append(R.random_path(rng, n, alphabet=4, max_len=5, unit=[1, 2]))
        cases.append(R.random_path(rng, n, alphabet=1, max_len=3))
        cases.append(R.random_path(rng, n, alphabet=2, max_len=3, repeats=True))
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_stats()
    got, host = run_kernel(ctx, cases)
    st = ctx.kernel_stats()
    assert list(st) == ["cigar_left_align"] and st["cigar_left_align"]["launches"] == 1
    n_moved = n_same_op = 0
    for c, g, h in zip(cases, got, host):
        assert g == h, (R.show(c[0])[:200], R.show(g)[:200], R.show(h)[:200])
        n_moved += g != c[0]
        n_same_op += not R.normal_form(c[0])
    assert n_moved > 1000 and n_same_op > 1000 and st["cigar_left_align"]["work_units"] > 1000 and st["cigar_left_align"]["algorithmic_bytes"] > 0
    # bad jobs are refused on the host and nothing is launched; an empty job list is an empty result
    ctx.reset_kernel_stats()
    ref, qry = np.array(list(b"AAAAAAAACG"), dtype=np.uint8), np.array(list(b"AAAAAAACG"), dtype=np.uint8)
    words = R.words_of(R.parse("7=1D2=") + [(4, 3), (7, 0)])
    good = (0, 3, 0, 10, 0, 0, 9)
    for bad in ((0, 6, 0, 10, 0, 0, 9), (0, 3, 1, 10, 0, 0, 9), (0, 3, 0, 10, 0, 1, 9), (3, 1, 0, 10, 0, 0, 9), (4, 1, 0, 10, 0, 0, 9), (0, 3, 0, 9, 0, 0, 9),
                (0, 3, 0, 10, 1, 0, 9), (0, 3, 0, 10, 0, 0, 8)):
        with pytest.raises(F.FloxerError):
            F.left_align_batch(ctx, qry, words, [good, bad], reference_pool=ref)
    assert F.left_align_batch(ctx, qry, words, [], reference_pool=ref) == []
    assert ctx.kernel_stats() == {}
    assert [R.show(R.path_of(w)) for w in F.left_align_batch(ctx, qry, words, [good, (0, 0, 0, 0, 0, 0, 0)], reference_pool=ref)] == ["1=1D8=", ""]
    ctx.enable_kernel_timing(False)


# ------------------------------------------------------------------------------------------------ behind K5
def corpus_cases():
    """a few dozen of the corpus: planted D and I runs, ties, 2 NM + 1 runs; the small ones of every class (one DP matrix <= 10^6 cells)"""
    picked = []
    for cls, n in (("gap", 16), ("ties", 20), ("runs", 12)):
        of_cls = sorted((c for c in AC.whole() if c.cls == cls and len(c.ref) * len(c.query) <= 10 ** 6), key=lambda c: c.name)
        step = max(1, len(of_cls) // n)
        picked += of_cls[::step][:n]
    return picked


@gpu
def test_behind_k5_words_are_the_rule_on_the_oracles_cigar_and_md_follows(ctx):
    cases = corpus_cases()
    assert len(cases) >= 36 and {c.cls for c in cases} == {"gap", "ties", "runs"}
    rpool, qpool, jobs, what = AC.batch(cases, (2,))
    plain = F.align_batch(ctx, qpool, jobs, reference_pool=rpool, md=True)
    off = F.align_batch(ctx, qpool, jobs, reference_pool=rpool, md=True, gaps=F.gap_options(left_align=False))
    assert off == plain                                               # a struct that is off is the call without it
    got = F.align_batch(ctx, qpool, jobs, reference_pool=rpool, md=True, gaps=F.gap_options())
    no_md = F.align_batch(ctx, qpool, jobs, reference_pool=rpool, gaps=F.gap_options())
    moved = full = 0
    for (c, _), g, p, g3 in zip(what, got, plain, no_md):
        exp = AC.expected(c, 2)
        assert p is not None and p[:3] == exp, c.name
        path = R.parse(exp[2])
        want = R.left_align(path, c.ref, c.query, exp[1])
        assert g is not None and (g[0], g[1]) == (exp[0], exp[1]), c.name            # NM and begin are the oracle's
        assert g[2] == R.show(want), (c.name, g[2][:200], R.show(want)[:200])
        assert g[3] == md_from_cigar(c.ref, exp[1], R.words_of(want)), c.name
        assert g3 == g[:3], c.name
        R.check_properties(path, c.ref, c.query, exp[1], want)
        moved += want != path
        full += len(want) == 2 * exp[0] + 1
    assert moved >= 8 and full >= 4, (moved, full)


# ------------------------------------------------------------------------------------------------ the whole path
N_READS, READ_LEN, CHROM = 300, 2000, 1_000_000


def oriented(read, flag):
    return S._COMP[read[::-1]] if flag & 16 else read


def core_of(cigar):
    """(leading clip, the = X I D words as a path, trailing clip) of a CIGAR string"""
    ops = [(int(n), op) for n, op in __import__("re").findall(r"(\d+)([=XIDS])", cigar)]
    lead = ops[0][0] if ops and ops[0][1] == "S" else 0
    trail = ops[-1][0] if len(ops) > 1 and ops[-1][1] == "S" else 0
    return lead, [("MIDNSHP=X".index(op), n) for n, op in ops if op != "S"], trail


def record_parts(chrom, read, rec):
    """(path, reference window, aligned part of the oriented read) of a mapped record"""
    _, flag, _, pos, _, cigar = rec
    lead, path, trail = core_of(cigar)
    q = oriented(read, flag)
    cols = sum(ln for op, ln in path if op != I)
    return path, chrom[pos: pos + cols], q[lead: len(q) - trail], lead, trail


def with_clips(lead, path, trail):
    return (f"{lead}S" if lead else "") + R.show(path) + (f"{trail}S" if trail else "")


def check_on_is_off_left_aligned(chrom, reads, on, off):
    """records = the option-off records with the rule applied to each CIGAR, every other field and the order equal, MD following"""
    a, b = on.records(), off.records()
    assert len(a) == len(b) and on.skipped.tolist() == off.skipped.tolist()
    changed = 0
    for j, (x, y) in enumerate(zip(a, b)):
        assert x[:5] == y[:5], (j, x[:5], y[:5])
        if y[1] & 4:
            assert x == y
            continue
        path, window, q, lead, trail = record_parts(chrom, reads[y[0]], y)
        want = R.left_align(path, window, q, 0)
        assert x[5] == with_clips(lead, want, trail), (j, x[5][:300], with_clips(lead, want, trail)[:300])
        assert on.md[j] == md_from_cigar(chrom, y[3], R.words_of(want)), j
        changed += x[5] != y[5]
    assert (on.mapq == off.mapq).all()
    return changed


@pytest.fixture(scope="module")
def world():
    pool, chroms = S.make_genome_fast(CHROM, 1, seed=61, repeat_rich=True)
    (rp, ro), _ = S.make_reads_fast(pool, [CHROM], N_READS, READ_LEN, RATE, seed=62)
    reads = [rp[int(ro[i]): int(ro[i + 1])].copy() for i in range(N_READS)]
    idx = F.fmindex(chroms)
    c = F.context(idx)
    runs, stats = {}, {}
    c.enable_kernel_timing(True)
    for name, kw in (("plain", {}), ("I", dict(interval_optimization=True))):
        p = F.params(error_probability=RATE, **kw)
        for on in (False, True):
            c.reset_kernel_stats()
            runs[name, on] = F.aligner(c, p, F.output_options(mapq=True), md=True, gaps=F.gap_options() if on else None).align_reads(reads)
            stats[name, on] = c.kernel_stats()
    c.enable_kernel_timing(False)
    yield dict(chroms=chroms, reads=reads, idx=idx, ctx=c, runs=runs, stats=stats)
    c.close()


@gpu
@pytest.mark.parametrize("name", ["plain", "I"])
def test_whole_path_on_is_off_with_the_rule_applied_to_every_cigar(world, name):
    on, off = world["runs"][name, True], world["runs"][name, False]
    mapped = sum(1 for r in off.records() if not r[1] & 4)
    assert mapped >= N_READS // 2
    changed = check_on_is_off_left_aligned(world["chroms"][0], world["reads"], on, off)
    assert changed >= mapped // 10, (changed, mapped)                 # (8 % errors over repeats: a gap that can move is common)
    st = world["stats"][name, True]["cigar_left_align"]
    assert st["launches"] >= 1 and st["device_ms"] > 0 and st["algorithmic_bytes"] > 0 and st["work_units"] > 0
    assert "cigar_left_align" not in world["stats"][name, False]


@gpu
def test_off_is_the_plain_call_and_launches_nothing(world):
    ctx, reads = world["ctx"], world["reads"]
    p = F.params(error_probability=RATE)
    off = world["runs"]["plain", False]
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_stats()
    for gaps in (F.capi.GapOptions(), F.gap_options(left_align=False)):
        got = F.aligner(ctx, p, F.output_options(mapq=True), md=True, gaps=gaps).align_reads(reads)
        # (every field of every record, the offsets into the pools included; what lies between the slabs of a pool is unspecified)
        assert got.records() == off.records() and got.md == off.md and (got.raw == off.raw).all()
        assert len(got.cigars) == len(off.cigars) and (got.md_refs == off.md_refs).all() and len(got.md_bytes) == len(off.md_bytes)
    assert "cigar_left_align" not in ctx.kernel_stats()
    ctx.enable_kernel_timing(False)
    with pytest.raises(F.FloxerError, match="without_cigar"):
        F.aligner(ctx, F.params(error_probability=RATE, without_cigar=True), gaps=F.gap_options()).align_reads(reads[:2])


@gpu
def test_partial_extend_and_split_records_replay_and_are_in_normal_form(world, tmp_path):
    """cigar_tails reads the normalised words, so cuts may differ from the option-off run: properties, not equality"""
    ctx, chrom = world["ctx"], world["chroms"][0]
    rng = np.random.default_rng(63)
    reads = list(world["reads"][:60])
    for i in range(12):                                               # chimeras and reads with a junk tail, so that all three stages have work
        a, b = world["reads"][100 + i], world["reads"][120 + i]
        reads.append(np.concatenate([a[:1200], b[:1200]]) if i % 2 else np.concatenate([a, rng.integers(1, 5, size=400, dtype=np.uint8)]))
    al = F.aligner(ctx, F.params(error_probability=RATE), F.output_options(max_alignments=1, mapq=True), md=True, partial=F.partial_options(min_query_span=300),
                   extend=F.extend_options(), split=F.split_options(), gaps=F.gap_options())
    run = al.align_reads(reads)
    recs = run.records()
    clipped = 0
    for j, rec in enumerate(recs):
        if rec[1] & 4:
            continue
        path, window, q, lead, trail = record_parts(chrom, reads[rec[0]], rec)
        cols, rows, nm = R.replay(path, window, q, 0)                  # = columns equal, X columns unequal
        assert rows == len(q) and lead + rows + trail == len(reads[rec[0]]) and nm == rec[4], (j, rec[:5])
        assert R.normal_form(path) and R.left_align(path, window, q, 0) == path, (j, rec[5][:300])
        assert run.md[j] == md_from_cigar(chrom, rec[3], R.words_of(path)), j
        clipped += bool(lead or trail)
    assert clipped >= 6, clipped
    # the project's own check of a record: the CIGAR consumes the whole read, NM = X + I + D and is the oracle's for the aligned part, MD
    for j, rec in enumerate(recs):
        if not rec[1] & 4:
            check_record([chrom], reads[rec[0]], rec, run.md[j])
    # the same run through the CLI: the SAM holds the library's records, MD and SA, and every line passes the same check
    fasta, fastq, sam = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq"), str(tmp_path / "out.sam")
    with open(fasta, "w") as f:
        f.write(">chr0\n" + "\n".join(letters(chrom[o: o + 100]) for o in range(0, len(chrom), 100)) + "\n")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
    r = subprocess.run([os.path.join(ROOT, "floxer_amd", "floxer"), "--reference", fasta, "--queries", fastq, "--output", sam, "--error-probability", str(RATE),
                        "--threads", "2", "-N", "1", "-Q", "--md-tag", "--partial-alignments", "--partial-min-span", "300", "--partial-extend", "--split-tails",
                        "--sa-tag", "--left-align-indels"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l.split("\t") for l in open(sam).read().splitlines() if not l.startswith("@")]
    got = []
    for f in lines:
        tags = dict((t[:2], t[5:]) for t in f[11:])
        rec = (int(f[0][4:]), int(f[1]), -1 if f[2] == "*" else 0, int(f[3]) - 1, int(tags.get("NM", 0)), "" if f[5] == "*" else f[5])
        got.append((rec, int(f[4]), tags.get("MD"), tags.get("SA")))
        if not rec[1] & 4:
            assert len(f[9]) == len(reads[rec[0]]) and f[2] == "chr0"
            check_record([chrom], reads[rec[0]], rec, tags["MD"].encode())
    assert [g[0] for g in got] == recs and [g[1] for g in got] == run.mapq.tolist()
    assert [g[2] for g in got] == [m.decode() if m else None for m in run.md]
    assert [g[3] for g in got] == sa_strings(recs, ["chr0"], run.mapq.tolist()) and any(g[3] for g in got)
    # and the option changes something here as well
    base = F.aligner(ctx, F.params(error_probability=RATE), F.output_options(max_alignments=1, mapq=True), md=True, partial=F.partial_options(min_query_span=300),
                     extend=F.extend_options(), split=F.split_options()).align_reads(reads)
    assert [r[:2] for r in base.records() if r[1] & 4] == [r[:2] for r in recs if r[1] & 4]
    assert any(R.left_align(*record_parts(chrom, reads[r[0]], r)[:3], 0) != record_parts(chrom, reads[r[0]], r)[0] for r in base.records() if not r[1] & 4)


@gpu
def test_resident_host_and_chunked_reads_give_the_same_words(world, monkeypatch):
    ctx, reads = world["ctx"], world["reads"]
    want = world["runs"]["plain", True]
    al = F.aligner(ctx, F.params(error_probability=RATE), F.output_options(mapq=True), md=True, gaps=F.gap_options())
    rr = F.resident_reads(ctx, reads)
    resident = al.align_reads(rr)
    rr.close()
    monkeypatch.setenv("FLX_CHUNK_READS", str(N_READS // 3 + 1))
    cut = al.align_reads(reads)
    monkeypatch.delenv("FLX_CHUNK_READS")
    for other in (resident, cut):
        assert other.records() == want.records() and other.md == want.md and (other.mapq == want.mapq).all()


@gpu
def test_context_without_host_text_gives_the_same_words():
    import torch
    pool, chroms = S.make_genome_fast(200_000, 1, seed=65, repeat_rich=True)
    (rp, ro), _ = S.make_reads_fast(pool, [200_000], 60, 1500, RATE, seed=66)
    idx = F.fmindex(chroms, device=0)
    base_ctx = F.context(idx)
    light = F.fmindex.from_meta(idx.meta())                          # no arrays: the host holds no text
    image = [torch.empty(n, dtype=torch.uint8, device="cuda:0") for n in idx.image_layout()]
    idx.image_upload(0, [b.data_ptr() for b in image])
    ctx = F.context(light, image=image)
    p = F.params(error_probability=RATE)
    base = F.aligner(base_ctx, p, md=True, gaps=F.gap_options()).align_reads((rp, ro))
    plain = F.aligner(base_ctx, p, md=True).align_reads((rp, ro))
    got = F.aligner(ctx, p, md=True, gaps=F.gap_options()).align_reads((rp, ro))
    assert got.records() == base.records() and got.md == base.md
    assert got.records() != plain.records() and [r[:5] for r in got.records()] == [r[:5] for r in plain.records()]
    ctx.close()
    base_ctx.close()


@gpu
def test_cli_left_align_indels_sam_and_bam(world, tmp_path):
    rng = np.random.default_rng(71)
    chrom = rng.integers(1, 5, size=30000).astype(np.uint8)
    chrom[15000: 15007] = 1                                           # AAAAAAA between two letters that are not A
    chrom[14999], chrom[15007] = 2, 3
    planted = np.concatenate([chrom[14500: 15006], chrom[15007: 15500]])      # one A of the run deleted
    reads = [planted] + [r for r in S.make_reads([chrom], 20, 1000, 0.06, seed=72)[0]]
    fasta, fastq = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq")
    with open(fasta, "w") as f:
        f.write(">chr0\n" + "\n".join(letters(chrom[o: o + 100]) for o in range(0, len(chrom), 100)) + "\n")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
    exe = os.path.join(ROOT, "floxer_amd", "floxer")

    def run(out, *extra):
        r = subprocess.run([exe, "--reference", fasta, "--queries", fastq, "--output", out, "--error-probability", "0.06", "--threads", "1", "--md-tag", *extra],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        return open(out, "rb").read()

    off = [l.split("\t") for l in run(str(tmp_path / "off.sam")).decode().splitlines() if not l.startswith("@")]
    on = [l.split("\t") for l in run(str(tmp_path / "on.sam"), "--left-align-indels").decode().splitlines() if not l.startswith("@")]
    assert len(on) == len(off) >= len(reads)
    changed = 0
    for x, y in zip(on, off):
        assert x[:5] == y[:5] and x[6:11] == y[6:11]
        if y[2] == "*":
            assert x == y
            continue
        read = reads[int(y[0][4:])]
        rec = (0, int(y[1]), 0, int(y[3]) - 1, 0, y[5])
        path, window, q, lead, trail = record_parts(chrom, read, rec)
        want = R.left_align(path, window, q, 0)
        assert x[5] == with_clips(lead, want, trail)
        assert x[-1] == "MD:Z:" + md_from_cigar(chrom, rec[3], R.words_of(want)).decode() and x[-2] == y[-2]
        changed += x[5] != y[5]
    assert changed >= 1
    # the planted read: the deletion at the homopolymer's last column without the option, at its first column with it
    first_off, first_on = [f for f in off if f[0] == "read0"][0], [f for f in on if f[0] == "read0"][0]
    assert first_off[5] == "506=1D493=" and first_on[5] == "500=1D499=" and int(first_on[3]) - 1 + 500 == 15000
    assert first_on[-1] == "MD:Z:500^A499"
    bam = bam_records(run(str(tmp_path / "on.bam"), "--left-align-indels"))
    assert [(r["flag"], r["pos"], r["n_cigar"]) for r in bam] == [(int(f[1]), int(f[3]) - 1, 0 if f[5] == "*" else len(cigar_words(f[5]))) for f in on]
    assert [dict((t, v) for t, _, v in r["tags"]).get("MD") for r in bam] == [f[-1][5:].encode() if f[-1].startswith("MD:Z:") else None for f in on]
    r = subprocess.run([exe, "--reference", fasta, "--queries", fastq, "--output", str(tmp_path / "w.sam"), "-e", "2", "--left-align-indels", "-w"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr
