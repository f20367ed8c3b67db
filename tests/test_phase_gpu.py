"""Phasing on the GPU (flx_phase: phase_observe, phase_links, phase_chain with the scan, phase_tags, phase_votes, phase_revote; runs, the
Python class and the floxer_phase tool). Every expected value is the plain-numpy rule of tests/phase_ref.py on the same sites, records,
words and reads, bit for bit; the shapes sit on the kernels' boundaries (64 CIGAR words per pass, the observe kernel's grid cap, the
tables' first sizes, the scan's tile)."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
from floxer_amd import simulate as S
import phase_ref as R
import coverage_ref
import pileup_ref as P
import variants_ref as V
from test_phase_host import SPECIAL_SITES, planted_truth_holds, same, sites_from_records, special_batch, special_rows

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
w = R.word


def device(text, lengths, sites, rec, words, reads, o, adds=1):
    """(results, tags) of the object over `adds` adds, and the add of every counted record"""
    c = F.phase(text=text, lengths=lengths, sites=sites, options=R.c_options(o))
    try:
        add_of = []
        for k, part in enumerate(np.array_split(np.arange(len(rec)), adds)):
            c.add_records(rec[part], words, reads)
            add_of += [k] * len(R.counted(rec[part], o))
        c.finish()
        return (c.results(), c.tags()), add_of
    finally:
        c.close()


def measure(text, lengths, sites, rec, words, reads, o, adds=1):
    got, add_of = device(text, lengths, sites, rec, words, reads, o, adds)
    return same(got, R.phase(lengths, sites, rec, words, reads, o, add_of))


# ------------------------------------------------------------------------------------------------ words and carries
def body_words(rng, n):
    """n words: = runs with X, I and D between them; word 63 is an = with an I in the next pass behind it, word 127 an = with a D behind
    it, word 191 an X with a D behind it; the first is an ="""
    ws = [("=" if t % 2 == 0 else "XID"[int(rng.integers(0, 3))], int(rng.integers(1, 10))) for t in range(n)]
    for t, op in ((62, "X"), (63, "="), (64, "I"), (126, "I"), (127, "="), (128, "D"), (191, "X"), (192, "D"), (193, "I")):
        if 0 < t < n:
            ws[t] = (op, min(ws[t][1], 4) if op == "I" else ws[t][1])
    return [w(op, ln) for op, ln in ws]


@gpu
@pytest.mark.parametrize("n_words", [1, 63, 64, 65, 128, 129, 200])
def test_words_and_carries(n_words):
    rng = np.random.default_rng(n_words)
    lengths = [3000, 2600]
    body = body_words(rng, n_words)
    inner = body_words(rng, max(1, n_words - 2))
    clipped = ([w("S", 7)] + inner + [w("S", 5)]) if n_words >= 3 else inner                  # the row carry starts at 7
    rows = [(0, 0, 1011, 0, body), (16, 0, 1011, 0, body), (16, 1, 0, 0, clipped), (0, 1, 5, 0, clipped), (16, 1, 2600 - R.span(body), 0, body),
            (0, 0, 2000, 0, [w("=", 30)])] + special_rows() * 3
    assert len(body) == n_words and (n_words < 3 or len(clipped) == n_words)
    rec, words, reads = R.records_with_reads(rng, rows)
    text = rng.integers(1, 5, size=sum(lengths)).astype(np.uint8)
    sp = special_batch(rng)
    k = len(rows) - 3 * len(special_rows())
    for i in range(k, len(rows)):                                          # the special rows keep the reads special_batch wrote for them
        reads[i] = sp[5][i - k]
    text[: 400] = sp[0][: 400]
    for read in reads[:k]:
        read[(read == 0) | (read == 5)] = 3                                # letters only: every I word of up to 32 letters behind a column can be a site
    o = R.options(min_link=1)
    # every X, I and D of the records is a site, plus SNVs on each record's first and last column and indels on its last
    extra = []
    for r in rec[:5]:
        first, last = int(r["pos"]), int(r["pos"]) + R.span(words[int(r["coff"]): int(r["coff"]) + int(r["clen"])]) - 1
        ref, base = int(r["ref"]), int(R.starts_of(lengths)[int(r["ref"])])
        extra += [(ref, first, R.SNV, 1 + int(text[base + first]) % 4, 1, ()), (ref, last, R.SNV, 1 + int(text[base + last]) % 4, 1, ()), (ref, last, R.INS, 0, 1, (2,))]
        if last + 1 < lengths[ref]:
            extra.append((ref, last, R.DEL, 0, 1, ()))
    found = {(int(s["ref"]), int(s["pos"]), int(s["kind"])): s for s in sites_from_records(rng, text, lengths, rec, words, reads, o, every=1, extra=30)}
    for s in R.sites_of(extra + [(r, p, kd, 1 + int(text[p]) % 4 if kd == R.SNV else 0, ln, le) for r, p, kd, a, ln, le in SPECIAL_SITES]):
        found.setdefault((int(s["ref"]), int(s["pos"]), int(s["kind"])), s)
    sites = np.array([found[key] for key in sorted(found)], dtype=F.PHASE_SITE_DTYPE)
    assert {R.SNV, R.DEL, R.INS} == {int(x) for x in sites["kind"]}
    res, tags = measure(text, lengths, sites, rec, words, reads, o)
    seen = set()
    for r in rec:
        seen |= {int(x) for x in R.observe(lengths, sites, r, words, reads)[1]}
    assert seen == {R.REF, R.ALT, R.NONE}
    first, obs = R.observe(lengths, sites, rec[0], words, reads)
    by_anchor = {(int(sites[first + j]["pos"]), int(sites[first + j]["kind"])): int(x) for j, x in enumerate(obs)}
    col = 1011 + np.cumsum([0] + [int(x) >> 4 if int(x) & 15 in (7, 8, 2) else 0 for x in body])      # the first column of every word
    if n_words >= 65:
        assert by_anchor[(int(col[64]) - 1, R.INS)] == R.ALT              # the last column of lane 63's word, its I word in the next pass
    if n_words >= 129:
        assert by_anchor[(int(col[128]) - 1, R.DEL)] == R.ALT
    if n_words >= 200:
        assert by_anchor[(int(col[192]) - 1, R.DEL)] == R.ALT and by_anchor[(int(col[193]) - 1, R.INS)] == R.ALT      # a D column with an I word behind it
    assert by_anchor[(1011, R.SNV)] == R.REF and by_anchor[(int(col[-1]) - 1, R.INS)] != R.REF       # the record's first column; an indel site on its last is never REF
    measure(text, lengths, sites, rec, words, reads, R.options(refine_rounds=2), adds=3)


@gpu
def test_sequence_boundaries():
    """sites on the last position of one sequence and the first of the next, and a sequence of one position: never connected"""
    rng = np.random.default_rng(5)
    lengths = [60, 50, 1, 40]
    text = rng.integers(1, 5, size=sum(lengths)).astype(np.uint8)
    alt = lambda ref, p: 1 + int(text[int(R.starts_of(lengths)[ref]) + p]) % 4      # noqa: E731
    sites = R.sites_of([(0, 50, R.SNV, alt(0, 50), 1, ()), (0, 59, R.SNV, alt(0, 59), 1, ()), (1, 0, R.SNV, alt(1, 0), 1, ()), (1, 49, R.SNV, alt(1, 49), 1, ()),
                        (2, 0, R.SNV, alt(2, 0), 1, ()), (3, 0, R.SNV, alt(3, 0), 1, ()), (3, 9, R.SNV, alt(3, 9), 1, ())])
    rows = [(0, 0, 45, 0, [w("=", 15)])] * 4 + [(0, 1, 0, 0, [w("=", 50)])] * 4 + [(16, 1, 0, 0, [w("X", 1), w("=", 48), w("X", 1)])] * 3 + [(0, 2, 0, 0, [w("=", 1)])] * 5 + \
        [(0, 3, 0, 0, [w("X", 1), w("=", 8), w("X", 1)])] * 3
    rec, words, reads = R.records_with_reads(rng, rows)
    for i, r in enumerate(rec):
        if int(r["ref"]) in (1, 3) and int(r["clen"]) == 3:
            seq = np.full(len(reads[i]), 1, dtype=np.uint8)
            seq[0], seq[-1] = alt(int(r["ref"]), 0), alt(int(r["ref"]), 49 if int(r["ref"]) == 1 else 9)
            reads[i] = P.oriented(seq, r["flag"])
    res, tags = measure(text, lengths, sites, rec, words, reads, R.options(min_link=1))
    assert [int(x) for x in res["phase_set"]] == [0, 0, 2, 2, 4, 5, 5] and [int(x) for x in res["phased"]] == [1, 1, 1, 1, 0, 1, 1]
    assert int(res["cis"][1]) == 0 and int(res["trans"][1]) == 0 and int(res["cis"][2]) == 7


# ------------------------------------------------------------------------------------------------ grid cap, growth, threads, contention
def dense(rng, n_records, n_sites=40, span=30):
    """one sequence with an SNV site every third position; records of `span` columns, each from one of two haplotypes with a few errors"""
    length = 3 * n_sites + span
    text = rng.integers(1, 5, size=length).astype(np.uint8)
    pos = np.arange(n_sites) * 3 + 2
    alt = 1 + text[pos] % 4
    hap_of = rng.integers(0, 2, size=n_sites)
    sites = R.sites_of([(0, int(p), R.SNV, int(a), 1, ()) for p, a in zip(pos, alt)])
    rows, reads = [], []
    for i in range(n_records):
        start = int(rng.integers(0, length - span + 1))
        hap = i % 2
        seq = text[start: start + span].copy()
        for j, p in enumerate(pos):
            if start <= p < start + span and (int(hap_of[j]) == hap) != (rng.random() < 0.1):
                seq[p - start] = alt[j]
        diff = seq != text[start: start + span]
        ws, k = [], 0
        while k < span:
            e = k
            while e < span and diff[e] == diff[k]:
                e += 1
            ws.append(w("X" if diff[k] else "=", e - k))
            k = e
        flag = 16 if i % 3 == 0 else 0
        rows.append((flag, 0, start, 0, ws))
        reads.append(P.oriented(seq, flag))
    rec, words = R.records_of(rows)
    rec["read"] = np.arange(len(rec))
    return text, [length], sites, rec, words, reads


@gpu
def test_more_records_than_the_grid():
    cap, waves, tile, longest = F.phase_geometry()
    rng = np.random.default_rng(11)
    text, lengths, sites, rec, words, reads = dense(rng, cap * waves + 700, n_sites=12, span=9)
    assert len(rec) > cap * waves
    res, tags = measure(text, lengths, sites, rec, words, reads, R.options())
    assert len(tags) == len(rec) and int(res["phased"].sum()) == 12 and {1, 2} <= {int(h) for h in tags["hap"]}


@gpu
def test_tables_grow_across_adds():
    """the same 3000 records added eleven times: more than 2^14 records and more than 2^20 slots. With min_link 1 the chain of the
    counts times eleven is the chain of the counts, so the reference is run once"""
    rng = np.random.default_rng(12)
    text, lengths, sites, rec, words, reads = dense(rng, 3000, n_sites=400, span=100)
    o = R.options(min_link=1, refine_rounds=2)
    want_res, want_tags = R.phase(lengths, sites, rec, words, reads, o)
    times = 11
    assert len(rec) * times > 1 << 14 and int(want_tags["n_slots"].sum()) * times > 1 << 20 and int(want_tags["n_slots"].sum()) * (times - 1) < 1 << 20
    c = F.phase(text=text, lengths=lengths, sites=sites, options=R.c_options(o))
    for _ in range(times):
        c.add_records(rec, words, reads)
    c.finish()
    res, tags = c.results(), c.tags()
    c.close()
    for name in ("cis", "trans", "keep", "swap"):
        want_res[name] *= times
    want = np.tile(want_tags, times)
    want["add"] = np.repeat(np.arange(times), len(want_tags))
    same((res, tags), (want_res, want))
    assert int(res["phased"].sum()) > 350


@gpu
def test_four_adding_threads_equal_one_add():
    rng = np.random.default_rng(77)
    text, lengths, sites, rec, words, reads = dense(rng, 2400, n_sites=300, span=60)
    o = R.options()
    want = R.phase(lengths, sites, rec, words, reads, o)
    same(device(text, lengths, sites, rec, words, reads, o)[0], want)
    c = F.phase(text=text, lengths=lengths, sites=sites, options=R.c_options(o))
    errors = []

    def work(part):
        try:
            for piece in np.array_split(part, 5):
                c.add_records(rec[piece], words, reads)
        except Exception as e:          # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(part,)) for part in np.array_split(np.arange(len(rec)), 4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors
    c.finish()
    res, tags = c.results(), c.tags()
    c.close()
    assert res.tobytes() == want[0].tobytes()
    assert sorted(int(a) for a in set(tags["add"])) == list(range(20))    # every add has its own serial
    key = lambda t: tuple(int(t[n]) for n in ("read", "hap", "phase_set", "h1", "h2", "n_slots", "reserved"))      # noqa: E731
    assert sorted(key(t) for t in tags) == sorted(key(t) for t in want[1])
    for a in range(20):                                                   # and the tags of one add stay together, in record order
        mine = tags[tags["add"] == a]["read"].astype(np.int64)
        assert (np.diff(mine) > 0).all()
        at = np.nonzero(tags["add"] == a)[0]
        assert (np.diff(at) == 1).all()


@gpu
def test_contention_on_one_pair_of_sites():
    rng = np.random.default_rng(13)
    text, lengths, sites, rec, words, reads = dense(rng, 5000, n_sites=2, span=6)
    keep = [i for i, r in enumerate(rec) if int(r["pos"]) <= 2 and int(r["pos"]) + 6 > 5]
    rec = rec[keep]
    assert len(rec) > 2000
    res, tags = measure(text, lengths, sites, rec, words, reads, R.options(refine_rounds=3))
    assert int(res["cis"][0]) + int(res["trans"][0]) == len(rec) and int(res["keep"][0]) + int(res["swap"][0]) > 1000


# ------------------------------------------------------------------------------------------------ chain geometry
@gpu
@pytest.mark.parametrize("n_sites", [4095, 4096, 4097, 2 * 4096 + 1])
def test_chain_geometry(n_sites):
    """set breaks on, before and behind the scan's tile borders; each record spans two or three sites"""
    rng = np.random.default_rng(n_sites)
    tile = F.phase_geometry()[2]
    length = 4 * n_sites + 8
    text = rng.integers(1, 5, size=length).astype(np.uint8)
    pos = np.arange(n_sites) * 4 + 1
    alt = 1 + text[pos] % 4
    sites = R.sites_of([(0, int(p), R.SNV, int(a), 1, ()) for p, a in zip(pos, alt)])
    hap_of = rng.integers(0, 2, size=n_sites)
    breaks = {b + d for b in range(tile, n_sites + tile, tile) for d in (-2, -1, 0, 1, 3) if b + d < n_sites} | {1, n_sites - 1} | {int(x) for x in rng.integers(2, n_sites - 1, size=40)}
    rows, reads = [], []
    i = 0
    while i < n_sites - 1:                                                # a record over sites i .. i + k - 1 that crosses no break
        k = 2 + int(rng.integers(0, 2))
        while k > 1 and any(j in breaks for j in range(i + 1, i + k)):
            k -= 1
        if k < 2 or i + k > n_sites:
            i += 1
            continue
        for hap in (0, 1):
            start, span = int(pos[i]) - 1, 4 * (k - 1) + 2
            seq = text[start: start + span].copy()
            for j in range(i, i + k):
                if int(hap_of[j]) == hap:
                    seq[int(pos[j]) - start] = alt[j]
            diff = seq != text[start: start + span]
            ws, q = [], 0
            while q < span:
                e = q
                while e < span and diff[e] == diff[q]:
                    e += 1
                ws.append(w("X" if diff[q] else "=", e - q))
                q = e
            rows.append((0, 0, start, 0, ws))
            reads.append(seq)
        i += k - 1
    rec, words = R.records_of(rows)
    rec["read"] = np.arange(len(rec))
    res, tags = measure(text, [length], sites, rec, words, reads, R.options(min_link=2, skip_refine=n_sites % 2 == 0))
    starts = sorted(set(int(s) for s in res["phase_set"]))
    assert set(starts) >= {b for b in breaks if b < n_sites} and all(s in breaks or s == 0 for s in starts)
    assert {b for b in (tile - 1, tile, tile + 1) if b < n_sites} <= set(starts) and int(res["phased"].sum()) > n_sites // 2 and (res["phased"] == 0).any()
    const = {}
    for j, r in enumerate(res):                                           # inside a set p is the planted haplotype up to one constant
        assert const.setdefault(int(r["phase_set"]), int(r["phase"]) ^ int(hap_of[j])) == int(r["phase"]) ^ int(hap_of[j])


# ------------------------------------------------------------------------------------------------ refinement
@gpu
def test_a_round_repairs_an_isolated_flip():
    """six SNV sites; the backbone records see sites 0 1 3 4 5 and a deleted column at site 2; three noisy records per haplotype see
    sites 1 2 3 with the wrong allele at 2, so both links of site 2 come out wrong; eight records per haplotype see site 2 rightly and
    a third letter at 1 and 3, so they add no link to it and outvote the three"""
    rng = np.random.default_rng(21)
    text = rng.integers(1, 5, size=80).astype(np.uint8)
    pos = [5, 15, 25, 35, 45, 55]
    alt = {p: 1 + int(text[p]) % 4 for p in pos}
    third = {p: next(x for x in range(1, 5) if x not in (int(text[p]), alt[p])) for p in pos}
    sites = R.sites_of([(0, p, R.SNV, alt[p], 1, ()) for p in pos])
    hap_of = [0, 1, 1, 0, 1, 0]                                           # the haplotype that carries each ALT
    rows, reads = [], []

    def add(hap, start, end, wrong=(), noise=(), deleted=(), copies=1):
        ops, letters = [], []
        for p in range(start, end):
            if p in deleted:
                ops.append("D")
                continue
            x = int(text[p])
            if p in pos:
                carries = (hap_of[pos.index(p)] == hap) != (p in wrong)
                x = third[p] if p in noise else alt[p] if carries else x
            ops.append("=" if x == int(text[p]) else "X")
            letters.append(x)
        ws, k = [], 0
        while k < len(ops):
            e = k
            while e < len(ops) and ops[e] == ops[k]:
                e += 1
            ws.append(w(ops[k], e - k))
            k = e
        for _ in range(copies):
            rows.append((0, 0, start, 0, ws))
            reads.append(np.array(letters, dtype=np.uint8))
    for hap in (0, 1):
        add(hap, 0, 70, deleted=(25,), copies=6)
        add(hap, 10, 40, wrong=(25,), copies=3)
        add(hap, 0, 70, noise=(15, 35), copies=8)
    rec, words = R.records_of(rows)
    rec["read"] = np.arange(len(rec))
    left, _ = measure(text, [80], sites, rec, words, reads, R.options(skip_refine=True))
    assert [int(x) for x in left["phase_set"]] == [0] * 6 and [int(p) ^ h for p, h in zip(left["phase"], hap_of)] == [0, 0, 1, 0, 0, 0]
    assert int(left["keep"].sum()) == 0 and int(left["swap"].sum()) == 0
    done, tags = measure(text, [80], sites, rec, words, reads, R.options())
    assert [int(p) ^ h for p, h in zip(done["phase"], hap_of)] == [0] * 6 and (int(done["keep"][2]), int(done["swap"][2])) == (6, 16)
    assert all(int(t["hap"]) == 1 + (i // 17) for i, t in enumerate(tags))      # p = 0: ALT on haplotype 1; hap_of counts from 0


# ------------------------------------------------------------------------------------------------ the pipeline
# Seed 31 was checked on the CPU oracle's records of this batch (tests/oracle_lib.py, default output, the primary records counted; the
# sites the 0/1 rows of variants_ref on those records): 62 of the 67 planted SNVs are sites and nothing else is, they fall into five
# phase sets with no unphased site, every p is the planted haplotype up to one constant per set, and none of the 973 tagged records
# (of 1000) with |h1 - h2| >= 2 sits on the wrong haplotype. Seed 32 gave the same picture (64 of 70, five sets). That is a property
# of the alignments, not of the kernels.
SAMPLE_SEED = 31
SAMPLE_RATE = 0.04


def diploid_batch():
    """two references of 20 kb; two haplotypes with het SNVs 300 to 800 apart, each on a random haplotype; 500 reads of 1000 letters
    from each haplotype on both strands with 1 % errors. Returns (chroms, reads, planted {(ref, pos): (alt rank, haplotype)}, the
    haplotype of every read)."""
    rng = np.random.default_rng(SAMPLE_SEED)
    chroms = S.make_genome(20_000, 2, seed=SAMPLE_SEED)
    haps = [[c.copy() for c in chroms], [c.copy() for c in chroms]]
    planted = {}
    for ref in range(2):
        p = 500
        while p < 19_500:
            hap = int(rng.integers(0, 2))
            rank = 1 + (int(chroms[ref][p]) - 1 + int(rng.integers(1, 4))) % 4
            haps[hap][ref][p] = rank
            planted[(ref, p)] = (rank, hap)
            p += int(rng.integers(300, 801))
    reads = S.make_reads(haps[0], 500, 1000, 0.01, seed=SAMPLE_SEED + 1)[0] + S.make_reads(haps[1], 500, 1000, 0.01, seed=SAMPLE_SEED + 2)[0]
    return chroms, reads, planted, [0] * 500 + [1] * 500


@pytest.fixture(scope="module")
def sample():
    chroms, reads, planted, hap_of_read = diploid_batch()
    ctx = F.context(F.fmindex(chroms))
    yield dict(chroms=chroms, reads=reads, ctx=ctx, rate=SAMPLE_RATE, planted=planted, hap_of_read=hap_of_read)
    ctx.close()


def aligner_of(sample, **kw):
    """the tool's alignment options: duplicates dropped, one alignment per read, indels left-aligned"""
    return F.aligner(sample["ctx"], F.params(error_probability=sample["rate"]), output=F.output_options(True, 1, False), gaps=F.gap_options(), **kw)


def het_sites(sample, runs):
    c = F.variants(sample["ctx"])
    for run, reads in runs:
        c.add(run, reads)
    c.finish()
    rows = c.rows()
    c.close()
    return F.phase_sites_from_rows(rows), rows


def run_against_reference(sample, sites, runs, o):
    chroms = sample["chroms"]
    c = F.phase(sample["ctx"], R.c_options(o), sites)
    parts, all_reads, add_of = [], [], []
    for k, (run, reads) in enumerate(runs):
        c.add(run, reads)
        raw = run.raw.copy()
        raw["read"] += len(all_reads)
        parts.append((raw, run.cigars))
        all_reads += list(reads)
        add_of += [k] * len(R.counted(raw, o))
    c.finish()
    got = c.results(), c.tags()
    c.close()
    rec, words = coverage_ref.joined(parts)
    want = R.phase([len(x) for x in chroms], sites, rec, words, all_reads, o, add_of)
    off = np.cumsum([0] + [len(reads) for _, reads in runs])
    want[1]["read"] -= off[want[1]["add"]].astype(np.uint32)             # (read counts inside its add)
    return same(got, want)


@gpu
def test_pipeline(sample):
    reads = sample["reads"]
    al = aligner_of(sample)
    whole = al.align_reads(reads)
    half = len(reads) // 2
    sites, rows = het_sites(sample, [(whole, reads)])
    o = R.options()
    one = run_against_reference(sample, sites, [(whole, reads)], o)
    two = run_against_reference(sample, sites, [(al.align_reads(reads[:half]), reads[:half]), (al.align_reads(reads[half:]), reads[half:])], o)
    assert one[0].tobytes() == two[0].tobytes()
    drop = lambda t: np.array([tuple(int(x[n]) for n in ("hap", "phase_set", "h1", "h2", "n_slots")) for x in t])      # noqa: E731
    assert (drop(one[1]) == drop(two[1])).all() and set(int(a) for a in two[1]["add"]) == {0, 1}
    assert {0, 16} <= {int(f) & 16 for f in whole.raw["flag"]}
    # the planted truth: most planted SNVs are sites; the sites that are planted carry their planted haplotype up to one constant per set
    planted = sample["planted"]
    mine = [(int(s["ref"]), int(s["pos"])) for s in sites]
    assert len(set(mine) & set(planted)) > 0.8 * len(planted) and all(int(s["alt_rank"]) == planted[k][0] for s, k in zip(sites, mine) if k in planted and int(s["kind"]) == R.SNV)
    res, tags = one
    const, wrong = {}, 0
    for s, k, r in zip(sites, mine, res):
        if k in planted and int(s["kind"]) == R.SNV and int(r["phased"]):
            c = int(r["phase"]) ^ planted[k][1]
            assert const.setdefault(int(r["phase_set"]), c) == c, (k, r)
    assert int(res["phased"].sum()) > 0.8 * len(sites) and len(const) <= 6
    for t in tags:
        if int(t["hap"]) and int(t["phase_set"]) in const and abs(int(t["h1"]) - int(t["h2"])) >= 2:
            wrong += ((int(t["hap"]) - 1) ^ const[int(t["phase_set"])]) != sample["hap_of_read"][int(t["read"])]
    assert wrong == 0 and int((tags["hap"] > 0).sum()) > 0.8 * len(tags)


@gpu
def test_lifetime_and_refusals(sample):
    L = capi.lib()
    rng = np.random.default_rng(1)
    text, lengths, sites, rec, words, reads = dense(rng, 60, n_sites=20, span=20)
    o = R.options()
    c = F.phase(text=text, lengths=lengths, sites=sites, options=R.c_options(o))
    c.add_records(rec, words, reads)
    n = lengths[0]
    # one bad record last in a batch of good ones: refused, the object stays as it was
    for bad, extra in (([(0, 0, n - 5, 0, [w("=", 6)])], 0), ([(0, 0, 0, 0, [])], 0), ([(0, 1, 0, 0, [w("=", 1)])], 0), ([(0, 0, 0, 0, [w("M", 5)])], 0), ([(0, 0, 0, 0, [w("=", 5)])], 1),
                       ([(0, 0, 0, 0, [w("S", 5), w("I", 1)])], 0)):
        rec2, words2, reads2 = R.records_with_reads(rng, [(0, 0, 0, 0, [w("=", 3), w("I", 2), w("D", 2), w("X", 20)])] * 3 + bad)
        if extra:
            reads2[-1] = np.ones(5 + extra, dtype=np.uint8)
        with pytest.raises(F.FloxerError):
            c.add_records(rec2, words2, reads2)
    rec2["read"][-1] = len(reads2)
    with pytest.raises(F.FloxerError, match="read_index"):
        c.add_records(rec2, words2, reads2)
    for call in (c.results, c.tags):
        with pytest.raises(F.FloxerError, match="flx_phase_finish"):
            call()
    assert L.flx_phase_num_tags(c.h) == 0 and L.flx_phase_num_sites(c.h) == 20
    c.finish()
    want = R.phase(lengths, sites, rec, words, reads, o)
    same((c.results(), c.tags()), want)
    for call in (lambda: c.add_records(rec, words, reads), lambda: c.add_records(rec[:0], words, reads), c.finish):
        with pytest.raises(F.FloxerError, match="finished"):
            call()
    out = np.zeros(20, dtype=F.PHASE_RESULT_DTYPE)
    assert L.flx_phase_copy_results(c.h, out.ctypes.data_as(C.POINTER(capi.PhaseResult)), 19) == -3 and "20 sites" in L.flx_last_error().decode()
    assert L.flx_phase_copy_results(c.h, out.ctypes.data_as(C.POINTER(capi.PhaseResult)), 20) == 0 and out.tobytes() == want[0].tobytes()
    tg = np.zeros(60, dtype=F.PHASE_TAG_DTYPE)
    assert L.flx_phase_copy_tags(c.h, tg.ctypes.data_as(C.POINTER(capi.PhaseTag)), 59) == -3 and "60 tags" in L.flx_last_error().decode()
    assert L.flx_phase_copy_tags(c.h, tg.ctypes.data_as(C.POINTER(capi.PhaseTag)), 60) == 0 and tg.tobytes() == want[1].tobytes()
    c.close()
    # an object without a site, and one without a record
    c = F.phase(text=text, lengths=lengths, sites=sites[:0])
    c.add_records(rec, words, reads)
    c.finish()
    assert len(c.results()) == 0 and len(c.tags()) == 60 and int(c.tags()["n_slots"].sum()) == 0
    c.close()
    c = F.phase(text=text, lengths=lengths, sites=sites)
    c.finish()
    assert len(c.tags()) == 0 and int(c.results()["phased"].sum()) == 0 and [int(x) for x in c.results()["phase_set"]] == list(range(20))
    c.close()
    # bad options, sites, lengths and texts
    bad = capi.PhaseOptions()
    bad.reserved[0] = 1
    wrong = sites.copy()
    wrong["alt_rank"][3] = text[int(wrong["pos"][3])]
    for make in (lambda: F.phase(text=text, lengths=lengths, sites=sites, options=bad), lambda: F.phase(text=text, lengths=lengths, sites=sites, options=F.phase_options(refine_rounds=9)),
                 lambda: F.phase(text=text, lengths=lengths, sites=wrong), lambda: F.phase(text=text, lengths=lengths, sites=sites[::-1]), lambda: F.phase(text=text, lengths=[n + 1], sites=sites),
                 lambda: F.phase(text=np.full(n, 6, dtype=np.uint8), lengths=lengths, sites=sites), lambda: F.phase(text=text, lengths=lengths, sites=sites, device=-1),
                 lambda: F.phase(sites=sites)):
        with pytest.raises(F.FloxerError):
            make()
    # for a context: flx_ctx_destroy waits for the object; a run without mapq under min_mapq; a run without CIGARs
    ctx = sample["ctx"]
    some = sample["reads"][:40]
    chrom_sites = R.sites_of([(0, 700, R.SNV, 1 + int(sample["chroms"][0][700]) % 4, 1, ())])
    with pytest.raises(F.FloxerError, match="site 0"):
        F.phase(ctx, None, R.sites_of([(0, 700, R.SNV, int(sample["chroms"][0][700]), 1, ())]))
    plain = aligner_of(sample).align_reads(some)
    c = F.phase(ctx, F.phase_options(min_mapq=2), chrom_sites)
    with pytest.raises(F.FloxerError, match="mapq"):
        c.add(plain, some)
    pool, offs, n_reads = F._pool_and_offsets(some)
    raw = C.c_void_p()
    capi.check(L.flx_align_reads(ctx.h, C.byref(F.params(error_probability=sample["rate"])), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n_reads, C.byref(raw)))
    with pytest.raises(F.FloxerError, match="mapq"):
        c.add(raw, some)
    L.flx_run_free(raw)
    with pytest.raises(F.FloxerError, match="phase"):
        capi.check(L.flx_ctx_destroy(ctx.h))
    c.close()
    bare = F.aligner(ctx, F.params(error_probability=sample["rate"], without_cigar=True)).align_reads(some)
    c = F.phase(ctx, None, chrom_sites)
    with pytest.raises(F.FloxerError, match="without_cigar"):
        c.add(bare, some)
    c.add(plain, some)                                                    # refused adds left the object as it was
    c.finish()
    same((c.results(), c.tags()), R.phase([len(x) for x in sample["chroms"]], chrom_sites, plain.raw, plain.cigars, some, R.options()))
    c.close()


# ------------------------------------------------------------------------------------------------ the tool
@gpu
def test_tool_files(sample, tmp_path):
    from test_md_gpu import letters
    chroms, reads = sample["chroms"], sample["reads"]
    work = tmp_path / "work"
    work.mkdir()
    fasta, fastq, calls = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq"), str(tmp_path / "calls.vcf")
    out, tsv = str(work / "phased.vcf"), str(work / "tags.tsv")
    with open(fasta, "w") as f:
        for i, c in enumerate(chroms):
            f.write(f">chr{i} sample\n" + "\n".join(letters(c[o: o + 80]) for o in range(0, len(c), 80)) + "\n")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
    whole = aligner_of(sample).align_reads(reads)
    sites, rows = het_sites(sample, [(whole, reads)])
    names = ["chr0", "chr1"]
    data = V.vcf_lines(rows, names, chroms)
    assert sum("\t0/1:" in l for l in data) == len(sites)
    # lines that pass through, among the tool's own: a comment with a tab, a homozygous call, a multi-allelic one, a symbolic one
    p0 = int(rows[0]["pos"])
    base_letter = letters(chroms[0][3: 4])
    extra = [f"chr0\t4\t.\t{base_letter}\t<DEL>\t9.00\t.\tDP=3\tGT\t0/1\n", f"chr0\t4\t.\t{base_letter}\t{'ACGT'.replace(base_letter, '')[0]},{'ACGT'.replace(base_letter, '')[1]}\t9.00\t.\tDP=3\tGT\t1/2\n",
             f"chr0\t4\t.\t{base_letter}\t{'ACGT'.replace(base_letter, '')[0]}\t9.00\t.\tDP=3\tGT\t1/1\n"]
    assert p0 > 4
    head = ["##fileformat=VCFv4.2\n", "##source=floxer_variants\n", "##note=a line\twith a tab\n", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"]
    lines = head + extra + data
    open(calls, "w").write("".join(lines))
    exe = os.path.join(ROOT, "floxer_amd", "floxer_phase")
    base = [exe, "--reference", fasta, "--queries", fastq, "--error-probability", str(sample["rate"]), "--variants", calls]
    env = dict(os.environ, FLX_BATCH_READS="64")                          # several batches
    r = subprocess.run(base + ["--output", out, "--haplotags", tsv], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    assert sorted(os.listdir(work)) == ["phased.vcf", "tags.tsv"] and sorted(os.listdir(tmp_path)) == ["calls.vcf", "reads.fastq", "ref.fasta", "work"]
    at, read_sites = R.vcf_sites(lines, names)
    assert read_sites.tobytes() == sites.tobytes() and at == [i for i, l in enumerate(lines) if "\t0/1:" in l]
    # the object over the same batches, one add per batch
    c = F.phase(sample["ctx"], None, sites)
    al = aligner_of(sample)
    for b in range(0, len(reads), 64):
        c.add(al.align_reads(reads[b: b + 64]), reads[b: b + 64])
    c.finish()
    res, tags = c.results(), c.tags()
    c.close()
    got = open(out).readlines()
    assert got == R.vcf_lines(lines, names, res) and got[3] == R.PS_HEADER and int(res["phased"].sum()) > 10
    assert sum("|" in l.split("\t")[9] for l in got if not l.startswith("#")) == int(res["phased"].sum())
    assert open(tsv).readlines() == R.tag_lines([f"read{i}" for i in range(len(reads))], tags, 64, sites) and len(tags) > 500
    # refused: an output that is no .vcf, the input as the output, a REF that is not the reference's: nothing is written
    for args, what in ((["--output", str(work / "other.bcf")], b"[vcf]"), (["--output", calls], b"the output is the input")):
        r = subprocess.run(base + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 255 and r.stderr.startswith(b"[CLI PARSER ERROR]\n") and what in r.stderr
    bad = str(tmp_path / "bad.vcf")
    open(bad, "w").write("".join(head + [data[0].replace("chr0", "chr9", 1)]))
    r = subprocess.run(base[:-1] + [bad, "--output", str(work / "other.vcf")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 255 and b"chr9" in r.stderr and r.stdout == b"" and sorted(os.listdir(work)) == ["phased.vcf", "tags.tsv"]
