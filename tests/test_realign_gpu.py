"""Affine-gap realignment on the GPU: the kernel alone (cigar_realign through flx_realign_batch) against the host rule (flx_realign) and
the Python rule of realign_ref.py, word for word and in score, NM and band, on the smallest shapes that can go wrong: row counts around
the 64-row stripes, bands whose cell count crosses the trace words of 8 cells and the 1024 cells of the hand-over row in LDS, gap runs
across one and several hand-overs, bands narrow enough to press against the optimum, references where only the ties decide, every score
set, and calls that cross a launch cut; then behind K5 on cases of the alignment corpus (flx_align_batch_realign with MD, and with
left-alignment on top); then whole runs (flx_align_reads_realign): the option on against the option off with flx_realign applied to
every record and the primary chosen again, off is off, resident / chunked reads, an index-image context, the partial, extend and split
stages, --stats, and the CLI's AS:i. Needs an MI355X (-m gpu)."""
import random

import numpy as np
import pytest

import floxer_amd as F
import align_corpus as AC
import leftalign_ref as LR
import realign_ref as R
from realign_ref import D, EQ, I, X
from test_md_host import md_from_cigar

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = F.context(F.fmindex([np.random.default_rng(5).integers(1, 5, size=2000).astype(np.uint8)]))
    yield c
    c.close()


def run(ctx, cases, scores=R.DEFAULT, band=16):
    """the kernel's and the host rule's results for the cases, each as (path, score, NM, lo, hi); kept == 0 asserted for both"""
    ref, qry, words, jobs = R.pack_jobs(cases)
    o = F.realign_options(True, *scores, band)
    got = F.realign_batch(ctx, qry, words, jobs, o, reference_pool=ref)
    host = F.realign(ref, qry, words, jobs, o)
    assert all(g["kept"] == 0 for g in got) and all(h["kept"] == 0 for h in host)
    flat = lambda r: (R.path_of(r["words"]), r["score"], r["num_errors"], r["diag_lo"], r["diag_hi"])
    return [flat(g) for g in got], [flat(h) for h in host]


def check(ctx, named, scores=R.DEFAULT, band=16, python_rule=True):
    cases = [c for _, c in named]
    got, host = run(ctx, cases, scores, band)
    for (name, c), g, h in zip(named, got, host):
        if python_rule:
            want = R.realign(*c, scores, band)
            assert h == want, (name, band, scores, R.show(h[0])[:200], R.show(want[0])[:200], h[1:], want[1:])
        assert g == h, (name, band, scores, R.show(c[0])[:200], R.show(g[0])[:200], R.show(h[0])[:200], g[1:], h[1:])
        R.check_properties(*c, g[0], g[1], scores, band)
    return got


def rows_case(m, seed):
    """a true path of exactly m rows with a deletion, an insertion and an X when there is room for them"""
    if m == 0:
        return R.spell([(D, 5)], R.noise(seed))
    if m < 6:
        return R.spell([(EQ, m)] if m < 2 else [(EQ, m - 1), (X, 1)], R.noise(seed))
    a = m // 3
    return R.spell([(EQ, a), (D, 2), (EQ, a), (I, 1), (X, 1), (EQ, m - 2 * a - 2)], R.noise(seed), begin=seed % 3, tail=2)


@gpu
def test_row_counts_around_the_stripes_and_empty_sides(ctx):
    named = [(f"{m} rows", rows_case(m, 10 + m)) for m in (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)]
    named.append(("no columns", (R.parse("4I"), np.zeros(0, np.uint8), np.array([1, 2, 3, 4], np.uint8), 0)))
    named.append(("no columns, 64 rows", (R.parse("64I"), np.zeros(0, np.uint8), np.arange(64, dtype=np.uint8) % 4 + 1, 0)))
    named.append(("empty", ([], np.zeros(0, np.uint8), np.zeros(0, np.uint8), 0)))
    got = check(ctx, named)
    assert R.show(got[0][0]) == "5D" and R.show(got[10][0]) == "4I" and got[12][0] == []
    # the last cell lies in every lane of a stripe's end in turn
    check(ctx, [(f"{m} rows, diagonal", R.spell([(EQ, m - 1), (X, 1)], R.noise(m))) for m in range(60, 70)], band=2)


@gpu
def test_band_widths_across_trace_words_and_stripe_steps(ctx):
    """a pure diagonal of 150 rows: B = 2 band + 1 = 3 ... 67 cells, so the cells of a row end inside, at the end of and behind a trace
    word, and a stripe's step count B + 126 crosses multiples of 8 and of 64"""
    path = [(EQ, 70), (X, 1), (EQ, 79)]
    for band in (1, 4, 16, 31, 32, 33):
        got = check(ctx, [("diagonal", R.spell(path, R.noise(3))), ("diagonal, begin 3", R.spell(path, R.noise(4), begin=3, tail=1))], band=band)
        assert got[0][0] == path and got[0][3:] == (-band, band)


@gpu
def test_gap_runs_across_hand_overs_and_a_band_beyond_lds(ctx):
    named = [("I of 70 rows from row 30", R.spell([(EQ, 30), (I, 70), (EQ, 60)], R.noise(1))),
             ("I of 700 rows", R.spell([(EQ, 30), (I, 700), (EQ, 40)], R.noise(2))),
             ("D of 1100 columns, one stripe", R.spell([(EQ, 20), (D, 1100), (EQ, 20)], R.noise(3))),
             ("D of 1100 columns, two stripes", R.spell([(EQ, 50), (D, 1100), (X, 1), (EQ, 49)], R.noise(4))),
             ("D of 995 columns: 1028 cells, just beyond LDS, three stripes", R.spell([(EQ, 70), (D, 995), (EQ, 70)], R.noise(5))),
             ("D of 991 columns: 1024 cells, the last band in LDS", R.spell([(EQ, 70), (D, 991), (EQ, 70)], R.noise(6)))]
    got = check(ctx, named)
    assert [R.show(g[0]) for g in got[:3]] == ["30=70I60=", "30=700I40=", "20=1100D20="]
    assert [g[4] - g[3] + 1 for g in got[2:]] == [1133, 1133, 1028, 1024]


@gpu
def test_narrow_bands_press_against_the_optimum(ctx):
    """random paths, and diagonal paths between unrelated two-letter sequences (= where the letters happen to agree, X elsewhere): there
    every shift the band allows pays, so the optimum runs along the band's edges"""
    rng = random.Random(33)
    cases = R.random_corpus(31, 120)
    for k in range(60):
        ref, qry = ([rng.randrange(2) for _ in range(rng.randint(2, 150))] for _ in range(2))
        n = min(len(ref), len(qry))
        path = []
        for a, b in zip(ref[:n], qry[:n]):
            op = EQ if a == b else X
            path.append((op, path.pop()[1] + 1) if path and path[-1][0] == op else (op, 1))
        cases.append((path, np.array(ref[:n], np.uint8), np.array(qry[:n], np.uint8), 0))
    pressed = 0
    for band in (1, 2):
        named = [(f"case {k}", c) for k, c in enumerate(cases[band - 1:: 2])]
        for g in check(ctx, named, band=band):
            ds = [j - i for i, j in R.cells(g[0])]
            pressed += min(ds) == g[3] or max(ds) == g[4]
    assert pressed >= 20, pressed


@gpu
def test_merge_still_ties_and_ranks(ctx):
    flank = b"TTGACCATCT", b"AATCGGCTAC"
    lit = lambda cigar, ref, qry, begin=0: (R.parse(cigar), np.array(list(ref), np.uint8), np.array(list(qry), np.uint8), begin)
    merge = [("scattered D", lit("10=1D2=1D1=1D10=", flank[0] + b"ACGCGT" + flank[1], flank[0] + b"CGG" + flank[1])),
             ("scattered I", lit("10=1I2=1I1=1I10=", flank[0] + b"CGG" + flank[1], flank[0] + b"ACGCGT" + flank[1])),
             ("scattered D, begin 2", lit("10=1D2=1D1=1D10=", b"GG" + flank[0] + b"ACGCGT" + flank[1] + b"T", flank[0] + b"CGG" + flank[1], 2))]
    got = check(ctx, merge)
    assert [R.show(g[0]) for g in got] == ["10=3D2=1X10=", "10=3I2=1X10=", "10=3D2=1X10="]
    assert all(R.gap_words(g[0]) < R.gap_words(c[0]) for (_, c), g in zip(merge, got))
    still = [("all =", R.spell([(EQ, 90)], R.noise(7))), ("one X", R.spell([(EQ, 40), (X, 1), (EQ, 40)], R.noise(8))),
             ("an optimal gap that cannot move right", lit("10=3D10=", flank[0] + b"CAG" + flank[1], flank[0] + flank[1])),
             ("an optimal I that cannot move right", lit("10=3I10=", flank[0] + flank[1], flank[0] + b"CAG" + flank[1]))]
    got = check(ctx, still)
    assert all(g[0] == c[0] for (_, c), g in zip(still, got))
    # only the ties decide: a homopolymer and a period-2 reference (the walk from the end takes a gap move as soon as one is as good)
    ties = [("homopolymer D", R.spell([(EQ, 40), (D, 2), (EQ, 40)], lambda c: 1)), ("homopolymer I", R.spell([(EQ, 40), (I, 2), (EQ, 40)], lambda c: 1, ins=lambda r: 1)),
            ("period 2 D", R.spell([(EQ, 41), (D, 2), (EQ, 40)], lambda c: 1 + c % 2)), ("period 2 D of 3", R.spell([(EQ, 41), (D, 3), (EQ, 40)], lambda c: 1 + c % 2)),
            ("period 2 I", R.spell([(EQ, 41), (I, 2), (EQ, 40)], lambda c: 1 + c % 2, ins=lambda r: 1 + (r + 1) % 2)),
            ("homopolymer I and D", R.spell([(EQ, 30), (I, 2), (EQ, 30), (D, 2), (EQ, 30)], lambda c: 1, ins=lambda r: 1))]
    got = check(ctx, ties)
    assert [R.show(g[0]) for g in got[:3]] == ["80=2D", "80=2I", "81=2D"] and R.show(got[5][0]) == "92="
    # ranks 0 and 5 are letters like any other
    for rank in (0, 5):
        path, ref, qry, begin = R.spell(R.parse("3=1D3=1I2=1D3=2X40=2D1=1D9="), R.noise(12), begin=1)
        ref[ref == 1] = rank
        qry[qry == 1] = rank
        assert (ref == rank).sum() > 5 and (qry == rank).sum() > 5
        check(ctx, [("ranks", (path, ref, qry, begin))])


@gpu
def test_every_score_set(ctx):
    rng = random.Random(41)
    named = [(f"random {k}", R.random_path(rng, rng.randint(1, 200), alphabet=4 if k % 2 else 2, rate=0.12)) for k in range(40)]
    named += [(f"{m} rows", rows_case(m, 70 + m)) for m in (63, 64, 65, 129)]
    changed = 0
    for scores in R.SCORE_SETS:
        changed += sum(g[0] != c[0] for (_, c), g in zip(named, check(ctx, named, scores=scores)))
    assert changed >= 40, changed


@gpu
def test_calls_that_cross_a_launch_cut_and_mixed_lengths(ctx):
    rng = random.Random(51)
    # 5000 jobs of eight rows: more than the 4096 jobs of one launch
    small = []
    while len(small) < 5000:
        c = R.random_path(rng, 8, alphabet=4, rate=0.2, max_indel=2)
        if len(c[2]) == 8:
            small.append(c)
    before = F.realign_counters(ctx)
    got, host = run(ctx, small)
    assert got == host
    for k in range(0, 5000, 25):
        assert got[k] == R.realign(*small[k]), k
    assert got[4095] == R.realign(*small[4095]) and got[4096] == R.realign(*small[4096]) and got[4999] == R.realign(*small[4999])
    after = F.realign_counters(ctx)
    assert after[0] - before[0] == 5000 and after[1] - before[1] == sum(g[0] != c[0] for g, c in zip(got, small)) and after[2] == before[2]
    # 64 jobs of mixed length in one call
    mixed = [(f"mixed {k}", R.random_path(rng, (1, 5, 30, 64, 100, 190, 260, 400)[k % 8], alphabet=4 if k % 3 else 2, rate=0.1)) for k in range(64)]
    check(ctx, mixed)
    ctx.path_counters(reset=True)
    assert F.realign_counters(ctx) == (0, 0, 0)


@gpu
def test_a_job_larger_than_the_trace_arena_keeps_its_path(tmp_path, monkeypatch):
    """FLX_TRACE_ARENA_KB sizes the lanes' arenas: with 64 KiB a 700-row path of 733 band cells (about 250 KiB of trace) is kept and
    flagged, its neighbours in the call are realigned, and the launches are cut so that every trace fits"""
    monkeypatch.setenv("FLX_TRACE_ARENA_KB", "64")
    c = F.context(F.fmindex([np.random.default_rng(5).integers(1, 5, size=2000).astype(np.uint8)]))
    try:
        rng = random.Random(61)
        cases = [R.random_path(rng, 150, rate=0.1) for _ in range(30)]        # about 150 rows x 40 cells / 2 = 3 to 6 KiB each: more than one launch
        cases.insert(5, R.spell([(EQ, 30), (I, 700), (EQ, 40)], R.noise(2)))
        ref, qry, words, jobs = R.pack_jobs(cases)
        got = F.realign_batch(c, qry, words, jobs, None, reference_pool=ref)
        host = F.realign(ref, qry, words, jobs, None)
        assert [g["kept"] for g in got] == [0] * 5 + [1] + [0] * 25 and F.realign_counters(c) == (30, sum(list(g["words"]) != list(R.words_of(k[0])) for g, k in zip(got, cases)), 1)
        big = got[5]
        assert R.path_of(big["words"]) == cases[5][0] and (big["score"], big["num_errors"], big["diag_lo"], big["diag_hi"]) == (0, 700, -716, 16)
        for k, (g, h) in enumerate(zip(got, host)):
            if k != 5:
                assert (list(g["words"]), g["score"], g["num_errors"]) == (list(h["words"]), h["score"], h["num_errors"]), k
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ behind K5
def corpus_cases():
    """a few dozen of the corpus: planted D and I runs (windows whose path begins behind column 0), ties, 2 NM + 1 runs; the small ones of
    every class (one DP matrix <= 10^6 cells)"""
    picked = []
    for cls, n in (("gap", 16), ("ties", 20), ("runs", 12)):
        of_cls = sorted((c for c in AC.whole() if c.cls == cls and len(c.ref) * len(c.query) <= 10 ** 6), key=lambda c: c.name)
        step = max(1, len(of_cls) // n)
        picked += of_cls[::step][:n]
    return picked


@gpu
def test_behind_k5_words_are_the_rule_on_k5s_words_and_left_align_and_md_follow(ctx):
    cases = corpus_cases()
    assert len(cases) >= 36 and {c.cls for c in cases} == {"gap", "ties", "runs"}
    rpool, qpool, jobs, what = AC.batch(cases, (2,))
    plain = F.align_batch(ctx, qpool, jobs, reference_pool=rpool, md=True)
    assert all(p is not None for p in plain) and any(p[1] > 0 for p in plain)
    off = F.align_batch_realign(ctx, qpool, jobs, F.realign_options(False), reference_pool=rpool, md=True)
    none = F.align_batch_realign(ctx, qpool, jobs, None, reference_pool=rpool, md=True)
    assert [o[:4] for o in off] == plain == [o[:4] for o in none] and all(o[4] == 0 for o in off + none)      # off is the call without it
    before = F.realign_counters(ctx)
    on = F.align_batch_realign(ctx, qpool, jobs, F.realign_options(), reference_pool=rpool, md=True)
    assert F.realign_counters(ctx)[0] - before[0] == len(jobs)
    no_md = F.align_batch_realign(ctx, qpool, jobs, F.realign_options(), reference_pool=rpool)
    both = F.align_batch_realign(ctx, qpool, jobs, F.realign_options(), reference_pool=rpool, md=True, gaps=F.gap_options())
    paths = [(R.parse(p[2]), c.ref, c.query, p[1]) for (c, _), p in zip(what, plain)]
    ref, qry, words, hjobs = R.pack_jobs(paths)
    host = F.realign(ref, qry, words, hjobs, F.realign_options())
    changed = fewer = moved = 0
    for (c, _), p, g, g3, b, h, path in zip(what, plain, on, no_md, both, host, paths):
        want = R.path_of(h["words"])
        assert h["kept"] == 0 and g is not None and g[1] == p[1], c.name                                  # begin is unchanged
        assert g[2] == R.show(want), (c.name, p[2][:200], g[2][:200], R.show(want)[:200])
        assert (g[0], g[4]) == (h["num_errors"], h["score"]), c.name
        assert g[3] == md_from_cigar(c.ref, p[1], R.words_of(want)), c.name
        assert g3[:3] == g[:3] and g3[3] is None and g3[4] == g[4], c.name
        R.check_properties(*path, want, g[4])
        la = LR.left_align(want, c.ref, c.query, p[1])
        assert b[2] == R.show(la) and (b[0], b[1], b[4]) == (g[0], g[1], g[4]), (c.name, b[2][:200], R.show(la)[:200])
        assert b[3] == md_from_cigar(c.ref, p[1], R.words_of(la)), c.name
        changed += want != path[0]
        fewer += R.gap_words(want) < R.gap_words(path[0])
        moved += la != want
    assert changed >= 1 and fewer >= 1 and moved >= 2, (changed, fewer, moved)       # (the corpus is edit-optimal over planted gaps: few paths change)


# ------------------------------------------------------------------------------------------------ the whole path
import os
import subprocess

from floxer_amd import simulate as S
from test_leftalign_gpu import letters, record_parts, with_clips

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE, CHROM_LEN = 0.08, 300_000


def rule_on_records(chrom, reads, recs, options=None, scores=R.DEFAULT):
    """flx_realign on the CIGAR of every mapped record: [(clipped CIGAR string, NM, score, path) | None]"""
    mapped = [j for j, r in enumerate(recs) if not r[1] & 4]
    parts = [record_parts(chrom, reads[recs[j][0]], recs[j]) for j in mapped]
    ref, qry, words, jobs = R.pack_jobs([(path, window, q, 0) for path, window, q, _, _ in parts])
    out = [None] * len(recs)
    for j, (_, _, _, lead, trail), g in zip(mapped, parts, F.realign(ref, qry, words, jobs, options)):
        assert g["kept"] == 0
        path = R.path_of(g["words"])
        assert g["score"] == R.path_score(path, scores)
        out[j] = (with_clips(lead, path, trail), g["num_errors"], g["score"], path)
    return out


def primary_rechosen(recs, nms):
    """flags with the primary chosen again by write_records' rule: a read's first record with its best NM, in output order"""
    flags, j = [], 0
    while j < len(recs):
        k = j
        while k < len(recs) and recs[k][0] == recs[j][0]:
            k += 1
        if recs[j][1] & 4:
            flags.append(recs[j][1])
        else:
            best = min(nms[j:k])
            first = j + nms[j:k].index(best)
            flags += [(recs[t][1] & ~256) | (0 if t == first else 256) for t in range(j, k)]
        j = k
    return flags


@pytest.fixture(scope="module")
def world():
    pool, chroms = S.make_genome_fast(CHROM_LEN, 1, seed=81, repeat_rich=True)
    reads = []
    for n, length, seed in ((24, 1000, 82), (24, 2000, 83)):
        (rp, ro), _ = S.make_reads_fast(pool, [CHROM_LEN], n, length, RATE, seed=seed)
        reads += [rp[int(ro[i]): int(ro[i + 1])].copy() for i in range(n)]
    c = F.context(F.fmindex(chroms))
    p = F.params(error_probability=RATE)
    runs, stats = {}, {}
    c.enable_kernel_timing(True)
    for on in (False, True):
        c.reset_kernel_stats()
        c.path_counters(reset=True)
        runs[on] = F.aligner(c, p, md=True, realign=F.realign_options() if on else None).align_reads(reads)
        stats[on] = c.kernel_stats()
    counters = F.realign_counters(c)
    c.enable_kernel_timing(False)
    yield dict(chrom=chroms[0], chroms=chroms, reads=reads, ctx=c, p=p, runs=runs, stats=stats, counters=counters)
    c.close()


@gpu
def test_whole_path_on_is_off_with_the_rule_applied_to_every_record_and_the_primary_chosen_again(world):
    on, off, chrom, reads = world["runs"][True], world["runs"][False], world["chrom"], world["reads"]
    a, b = on.records(), off.records()
    mapped = [j for j, r in enumerate(b) if not r[1] & 4]
    assert len(mapped) >= len(reads) // 2 and len(a) == len(b) and on.skipped.tolist() == off.skipped.tolist()
    want = rule_on_records(chrom, reads, b)
    nms = [w[1] if w else 0 for w in want]
    flags = primary_rechosen(b, nms)
    for j, (x, y) in enumerate(zip(a, b)):
        assert (x[0], x[2], x[3]) == (y[0], y[2], y[3]), (j, x[:5], y[:5])               # the order, the reference and the position
        assert x[1] == flags[j], (j, x[:5], y[:5], flags[j])
        if y[1] & 4:
            assert x == y and on.scores[j] == 0
            continue
        assert x[5] == want[j][0], (j, x[5][:300], want[j][0][:300])
        assert x[4] == want[j][1] >= y[4] and on.scores[j] == want[j][2], (j, x[4], want[j][1:3], on.scores[j])
        assert on.md[j] == md_from_cigar(chrom, y[3], R.words_of(want[j][3])), j
    changed = sum(x[5] != y[5] for x, y in zip(a, b))
    fewer = sum(R.gap_words(w[3]) < R.gap_words(record_parts(chrom, reads[y[0]], y)[0]) for w, y in zip(want, b) if w)
    assert changed >= len(mapped) // 2 and fewer >= len(mapped) // 3, (changed, fewer, len(mapped))      # (the issue's model: 54 and 52 of 60 paths)
    assert off.scores is None and on.scores.dtype == np.int32 and len(on.scores) == len(a)
    st = world["stats"][True]["cigar_realign"]
    assert st["launches"] >= 1 and st["device_ms"] > 0 and st["algorithmic_bytes"] > 0 and st["work_units"] > 0
    assert "cigar_realign" not in world["stats"][False]
    realigned, n_changed, kept = world["counters"]
    assert kept == 0 and realigned >= n_changed >= 1


@gpu
def test_off_is_the_plain_call_launches_nothing_and_has_no_scores(world):
    ctx, reads, p, off = world["ctx"], world["reads"], world["p"], world["runs"][False]
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_stats()
    ctx.path_counters(reset=True)
    for o in (F.capi.RealignOptions(), F.realign_options(enable=False, match=3, band=5)):
        got = F.aligner(ctx, p, md=True, realign=o).align_reads(reads)
        # (every field of every record, the offsets into the pools included; what lies between the slabs of a pool is unspecified)
        assert got.records() == off.records() and got.md == off.md and (got.raw == off.raw).all() and got.scores is None
        assert len(got.cigars) == len(off.cigars) and (got.md_refs == off.md_refs).all() and len(got.md_bytes) == len(off.md_bytes)
    assert "cigar_realign" not in ctx.kernel_stats() and F.realign_counters(ctx) == (0, 0, 0)
    ctx.enable_kernel_timing(False)
    # a run made without the option has no scores to copy
    pool, offs, n = F._pool_and_offsets(reads[:3])
    run = F.C.c_void_p()
    L, u8p, u64p = F.capi.lib(), F.capi.u8p, F.capi.u64p
    F.capi.check(L.flx_align_reads_realign(ctx.h, F.C.byref(p), F.capi.ptr(pool, u8p), F.capi.ptr(offs, u64p), n, None, None, None, None, F.C.byref(run)))
    assert L.flx_run_copy_scores(run, None) == -1 and b"without flx_realign_options.enable" in L.flx_last_error()
    L.flx_run_free(run)
    with pytest.raises(F.FloxerError, match="without_cigar"):
        F.aligner(ctx, F.params(error_probability=RATE, without_cigar=True), realign=F.realign_options()).align_reads(reads[:2])


@gpu
def test_resident_host_and_chunked_reads_give_the_same_records_and_scores(world, monkeypatch):
    ctx, reads, want = world["ctx"], world["reads"], world["runs"][True]
    al = F.aligner(ctx, world["p"], md=True, realign=F.realign_options())
    rr = F.resident_reads(ctx, reads)
    resident = al.align_reads(rr)
    rr.close()
    monkeypatch.setenv("FLX_CHUNK_READS", str(len(reads) // 3 + 1))
    cut = al.align_reads(reads)
    monkeypatch.delenv("FLX_CHUNK_READS")
    for other in (resident, cut):
        assert other.records() == want.records() and other.md == want.md and other.scores.tolist() == want.scores.tolist()


@gpu
def test_other_scores_and_left_alignment_on_top(world):
    ctx, reads, chrom, off = world["ctx"], world["reads"][:16], world["chrom"], world["runs"][False]
    scores, band = (5, 4, 10, 1), 4
    o = F.realign_options(True, *scores, band)
    base = [r for r in off.records() if r[0] < 16]
    want = rule_on_records(chrom, reads, base, o, scores)
    got = F.aligner(ctx, world["p"], md=True, realign=o).align_reads(reads)
    assert [r[5] for r in got.records()] == [w[0] if w else "" for w in want]
    assert got.scores.tolist() == [w[2] if w else 0 for w in want]
    # left-alignment reads the realigned words: its records are the rule of leftalign_ref on them, the scores stay
    la = F.aligner(ctx, world["p"], md=True, realign=o, gaps=F.gap_options()).align_reads(reads)
    for j, (x, g) in enumerate(zip(la.records(), got.records())):
        assert x[:5] == g[:5]
        if not g[1] & 4:
            path, window, q, lead, trail = record_parts(chrom, reads[g[0]], g)
            assert x[5] == with_clips(lead, LR.left_align(path, window, q, 0), trail), j
    assert la.scores.tolist() == got.scores.tolist()


@gpu
def test_context_on_an_index_image_gives_the_same_records():
    import torch
    pool, chroms = S.make_genome_fast(200_000, 1, seed=85, repeat_rich=True)
    (rp, ro), _ = S.make_reads_fast(pool, [200_000], 30, 1500, RATE, seed=86)
    idx = F.fmindex(chroms, device=0)
    base_ctx = F.context(idx)
    light = F.fmindex.from_meta(idx.meta())                          # no arrays: the host holds no text
    image = [torch.empty(n, dtype=torch.uint8, device="cuda:0") for n in idx.image_layout()]
    idx.image_upload(0, [b.data_ptr() for b in image])
    ctx = F.context(light, image=image)
    p = F.params(error_probability=RATE)
    base = F.aligner(base_ctx, p, md=True, realign=F.realign_options()).align_reads((rp, ro))
    plain = F.aligner(base_ctx, p, md=True).align_reads((rp, ro))
    got = F.aligner(ctx, p, md=True, realign=F.realign_options()).align_reads((rp, ro))
    assert got.records() == base.records() and got.md == base.md and got.scores.tolist() == base.scores.tolist()
    assert got.records() != plain.records() and [(r[0], r[2], r[3]) for r in got.records()] == [(r[0], r[2], r[3]) for r in plain.records()]
    ctx.close()
    base_ctx.close()


def check_realigned_record(chrom, read, rec, md, score, scores=R.DEFAULT):
    """What check_record (test_partial_gpu.py) asks of a record, clips, rows and letters, for a realigned one: the CIGAR consumes the whole
    read with its clips, every = column pairs equal letters and every X column unequal ones, NM = X + I + D, MD is the CIGAR's, and the
    score is the written path's. check_record's last line, NM = the edit distance of the aligned part, is what the rule gives up (its
    num_errors can exceed the edit distance), so it is not asked here."""
    path, window, q, lead, trail = record_parts(chrom, read, rec)
    cols, rows, nm = R.replay(path, window, q, 0)
    assert rows == len(q) and lead + rows + trail == len(read) and cols == len(window) and nm == rec[4], rec[:5]
    assert all(ln > 0 for _, ln in path) and all(x[0] != y[0] for x, y in zip(path, path[1:])), rec[5][:300]
    assert md == md_from_cigar(chrom, rec[3], R.words_of(path)) and score == R.path_score(path, scores), rec[:5]
    return bool(lead or trail)


@gpu
def test_partial_extend_and_split_tails_runs_write_sound_records(world):
    ctx, chrom, p = world["ctx"], world["chrom"], world["p"]
    rng = np.random.default_rng(87)
    reads = list(world["reads"][24:40])
    for i in range(10):                                               # chimeras and reads with a junk tail, so that every stage has work
        a, b = world["reads"][24 + i], world["reads"][36 + i]
        reads.append(np.concatenate([a[:1200], b[:1200]]) if i % 2 else np.concatenate([a, rng.integers(1, 5, size=400, dtype=np.uint8)]))
    partial = F.partial_options(min_query_span=300)
    for kw, out in ((dict(extend=F.extend_options()), F.output_options(mapq=True)), (dict(split=F.split_options()), F.output_options(max_alignments=1, mapq=True))):
        run = F.aligner(ctx, p, out, md=True, partial=partial, realign=F.realign_options(), **kw).align_reads(reads)
        base = F.aligner(ctx, p, out, md=True, partial=partial, **kw).align_reads(reads)
        recs = run.records()
        clipped = sum(check_realigned_record(chrom, reads[r[0]], r, run.md[j], int(run.scores[j])) for j, r in enumerate(recs) if not r[1] & 4)
        assert clipped >= 3, (kw, clipped)
        assert all(run.scores[j] == 0 for j, r in enumerate(recs) if r[1] & 4)
        assert sorted({r[0] for r in recs}) == list(range(len(reads))) and all(r[0] <= s[0] for r, s in zip(recs, recs[1:]))
        assert [r[:2] for r in recs if r[1] & 4] == [r[:2] for r in base.records() if r[1] & 4]
        for r in range(len(reads)):                                   # one primary per mapped read
            fl = [x[1] for x in recs if x[0] == r]
            assert fl == [4] or sum(1 for f in fl if not f & (256 | 2048)) == 1, (r, fl)


@gpu
def test_statistics_do_not_change_with_the_option(world):
    from test_gpu_parity import _parse_stats_toml
    reads, out = world["reads"][:24], {}
    idx = F.fmindex(world["chroms"])
    for on in (False, True):
        ctx = F.context(idx)
        st = F.statistics("simulated").attach(ctx)
        F.aligner(ctx, world["p"], realign=F.realign_options() if on else None).align_reads(reads)
        out[on] = _parse_stats_toml(st.format(toml=True))
        ctx.close()
    assert len(out[True]) >= 17 and out[True].keys() == out[False].keys()
    for sec in out[False]:
        if not sec.startswith("milliseconds_spent_in_"):           # wall-clock values
            assert out[True][sec] == out[False][sec], sec
    assert out[True]["alignments_per_query"]["num_values"] == 24
    # (and the records' NM does differ between the two: what the histograms hold is the edit distance, taken before the overwrite)
    assert any(x[4] > y[4] for x, y in zip(world["runs"][True].records(), world["runs"][False].records()))


@gpu
def test_cli_realign_affine_writes_the_librarys_records_with_as_in_sam_and_bam(world, tmp_path):
    from test_realign_host import _as_tags_of_bam
    chrom, reads = world["chrom"], world["reads"][:20]
    fasta, fastq = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq")
    with open(fasta, "w") as f:
        f.write(">chr0\n" + "\n".join(letters(chrom[o: o + 100]) for o in range(0, len(chrom), 100)) + "\n")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    for ext in ("sam", "bam"):
        out = str(tmp_path / f"on.{ext}")
        r = subprocess.run([exe, "--reference", fasta, "--queries", fastq, "--output", out, "--error-probability", str(RATE), "--threads", "2", "--md-tag",
                            "--realign-affine"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        lib = [(rec, int(s), m) for rec, s, m in zip(world["runs"][True].records(), world["runs"][True].scores, world["runs"][True].md) if rec[0] < 20]
        if ext == "sam":
            lines = [l.split("\t") for l in open(out).read().splitlines() if not l.startswith("@")]
            assert len(lines) == len(lib)
            for f, (rec, s, m) in zip(lines, lib):
                assert (int(f[0][4:]), int(f[1]), int(f[3]) - 1, "" if f[5] == "*" else f[5]) == (rec[0], rec[1], rec[3], rec[5])
                assert f[11:] == ([] if rec[1] & 4 else [f"NM:i:{rec[4]}", "MD:Z:" + m.decode(), f"AS:i:{s}"])
        else:
            tags = _as_tags_of_bam(open(out, "rb").read())
            assert len(tags) == len(lib)
            for t, (rec, s, m) in zip(tags, lib):
                assert [(a, v) for a, _, v in t] == ([] if rec[1] & 4 else [("NM", rec[4]), ("MD", m), ("AS", s)])
