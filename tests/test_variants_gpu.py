"""Variant calls on the GPU (flx_variants: pileup_add, variants_indel_keys, the key sort, consensus_allele_heads and _fill,
variants_anchor_winners, variants_call; runs, the Python class and the floxer_variants tool). Every expected value is the plain-numpy rule
of tests/variants_ref.py on the same text, records, words and reads; the shapes sit on the kernels' boundaries (64 CIGAR words per
pass, the key kernel's grid cap, the sort's tile, the scan's tile and second level)."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import variants_ref as R
import coverage_ref
import pileup_ref as P
from test_variants_host import COLUMNS, one_column
from test_pileup_gpu import sample_batch, special_rows

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one record is enough for a row: under priors of 1 a single alt read gives Q = (1574, 326, 37)
ANY = R.options(min_depth=1, min_qual=1, prior_het=1, prior_hom=1, max_del=6)


def results(c):
    return c.rows(), c.alleles()


def device(text, lengths, rec, words, reads, o, adds=1):
    c = F.variants(text=text, lengths=lengths, options=R.c_options(o))
    try:
        for part in np.array_split(np.arange(len(rec)), adds):
            c.add_records(rec[part], words, reads)
        c.finish()
        return results(c)
    finally:
        c.close()


def same(got, want):
    assert len(got[1]) == len(want[1]) and got[1].tobytes() == want[1].tobytes(), (got[1][:5], want[1][:5])
    if len(got[0]) == len(want[0]) and got[0].tobytes() != want[0].tobytes():
        bad = next(i for i in range(len(got[0])) if got[0][i] != want[0][i])
        assert False, (bad, got[0][bad], want[0][bad])
    assert len(got[0]) == len(want[0]), (len(got[0]), len(want[0]))
    return got


def measure(text, lengths, rec, words, reads, o, adds=1, times=1):
    return same(device(text, lengths, rec, words, reads, o, adds), R.variants(text, lengths, rec[: len(rec) // times], words, reads, o, times))


# ------------------------------------------------------------------------------------------------ words and carries
def body_words(rng, n):
    """n words: = runs with X, I and D between them, I and D words on both sides of every pass boundary (a D directly behind an I at 63 |
    64, an I directly behind a D at 127 | 128: one anchor each); the first is an ="""
    ws = [("=" if t % 2 == 0 else "XID"[int(rng.integers(0, 3))], int(rng.integers(1, 10))) for t in range(n)]
    for t, op in ((63, "I"), (64, "D"), (127, "D"), (128, "I")):
        if 0 < t < n:
            ws[t] = (op, ws[t][1])
    return [R.word(op, ln) for op, ln in ws]


@gpu
@pytest.mark.parametrize("n_words", [1, 63, 64, 65, 129])
def test_words_and_carries(n_words):
    rng = np.random.default_rng(n_words)
    lengths = [45_000, 33_000]
    body = body_words(rng, n_words)
    inner = body_words(rng, max(1, n_words - 2))
    clipped = ([R.word("S", 7)] + inner + [R.word("S", 5)]) if n_words >= 3 else inner        # the row carry starts at 7
    d_inner = body_words(rng, max(1, n_words - 4))
    # a D as the first reference word (void) and as the last one; the record ends on the sequence's last position
    d_ends = ([R.word("S", 3), R.word("D", 3)] + d_inner + [R.word("D", 4), R.word("S", 2)]) if n_words >= 5 else [R.word("D", 3)] + d_inner + [R.word("D", 4)]
    rows = [(0, 0, 1011, 0, body), (16, 0, 1011, 0, body), (16, 1, 0, 0, clipped), (0, 1, 5, 0, clipped), (0, 0, 45_000 - R.span(d_ends), 0, d_ends),
            (16, 1, 33_000 - R.span(body), 0, body)] + special_rows()
    assert len(body) == n_words and (n_words < 3 or len(clipped) == n_words)
    rec, words, reads = R.records_with_reads(rng, rows)
    for read in reads:
        read[(read == 0) | (read == 5)] = 3                                # letters only: every I word of up to 32 letters behind a column is an allele
    text = R.random_text(rng, sum(lengths))
    rows_got, al = measure(text, lengths, rec, words, reads, ANY)
    if n_words >= 65:
        ops = [int(x) & 15 for x in body]
        assert ops[63] == 1 and ops[64] == 2                               # an I and a D on the two sides of a pass boundary: the slot carry, one anchor
        assert len(al) >= 6 and {R.SNV, R.DEL, R.INS} <= {int(k) for k in rows_got["kind"]}
    if n_words >= 129:
        ops = [int(x) & 15 for x in body]
        assert ops[127] == 2 and ops[128] == 1
    # the deletion that ends the sequence: its anchor is the column in front of it, its columns reach 44 999
    last = [(int(a["pos"]), int(a["kind"]), int(a["length"])) for a in al if int(a["ref"]) == 0 and int(a["pos"]) == 45_000 - 5 and int(a["kind"]) == R.DEL]
    assert last == [(44_995, R.DEL, 4)]
    # the special rows: the I behind a leading S at 100 + 0 has no column in front and is void, as are the I that is the first word at 200,
    # the two of 70 letters at 500 and the D that is the first word at 0; the D of 4 at 300 + 9 and the I behind it share the anchor 309;
    # the I in front of the trailing S at 400 + 21 and the I at 0 + 1 are alleles
    mine = {(int(a["pos"]), int(a["kind"]), int(a["length"])) for a in al if int(a["ref"]) == 0 and int(a["pos"]) not in range(1011, 1011 + R.span(body)) and int(a["pos"]) < 44_000}
    assert mine == {(309, R.DEL, 4), (313, R.INS, 2), (421, R.INS, 4), (1, R.INS, 1)}, mine
    same(device(text, lengths, rec, words, reads, R.options(), adds=3), R.variants(text, lengths, rec, words, reads, R.options()))


# ------------------------------------------------------------------------------------------------ alleles
@gpu
def test_alleles():
    w = R.word
    rng = np.random.default_rng(12)
    lengths = [300, 50]
    rows, reads = [], []
    max_del = 7

    def add(flag, ref, pos, ws, read, copies=1):
        for _ in range(copies):
            rows.append((flag, ref, pos, 0, ws))
            reads.append(np.array(read, dtype=np.uint8))
    for k, n in enumerate((1, 2, 31, 32, 33)):                            # the insertion lengths round the key's 32 letters, two records each
        add(0, 0, 10 * k, [w("=", 5), w("I", n), w("=", 4)], [1] * 5 + [int(x) for x in rng.integers(1, 5, size=n)] + [2] * 4, copies=2)
    add(0, 0, 60, [w("=", 2), w("I", 3), w("=", 2)], [1, 1, 2, 5, 2, 1, 1], copies=2)      # a letter of rank 5, and of rank 0, inside an I: void
    add(0, 0, 70, [w("=", 2), w("I", 3), w("=", 2)], [1, 1, 0, 3, 2, 1, 1], copies=2)
    for k, n in enumerate((max_del - 1, max_del, max_del + 1)):           # the deletion lengths round max_del
        add(0, 0, 80 + 10 * k, [w("=", 1), w("D", n), w("=", 1)], [1, 1], copies=2)
    fw = [1, 2, 3, 4, 4, 1, 2, 2, 3]                                      # one read forward, and its reverse complement under flag 16: one allele
    add(0, 0, 200, [w("=", 3), w("I", 3), w("=", 3)], fw)
    add(16, 0, 200, [w("=", 3), w("I", 3), w("=", 3)], P.COMPLEMENT[np.array(fw, dtype=np.uint8)[::-1]])
    for ins in ([4, 1], [2, 3], [4, 1], [2, 3]):                          # equal counts at one anchor across letters, and across DEL and INS
        add(0, 0, 220, [w("=", 1), w("I", 2), w("=", 1)], [1] + ins + [1])
    for _ in range(2):
        add(0, 0, 220, [w("=", 1), w("D", 5), w("=", 1)], [1, 1])
        add(0, 0, 230, [w("=", 1), w("D", 2), w("=", 1)], [1, 1])
        add(0, 0, 230, [w("=", 1), w("I", 1), w("=", 1)], [1, 3, 1])
    for k in range(3):                                                    # three anchors on consecutive positions
        add(0, 0, 240 + k, [w("=", 1), w("I", 2), w("=", 3)], [1, 1 + k, 4, 1, 1, 1], copies=2)
    for ins, copies in (([4, 1], 5), ([1], 2)):                           # three alleles at one anchor: events is their sum
        add(0, 0, 260, [w("=", 1), w("I", len(ins)), w("=", 1)], [1] + ins + [1], copies=copies)
    add(0, 0, 260, [w("=", 1), w("D", 1), w("=", 1)], [1, 1], copies=3)
    add(0, 0, 297, [w("=", 3), w("I", 2)], [1, 1, 1, 3, 3], copies=2)      # an anchor on a sequence's last position
    add(0, 1, 0, [w("=", 4)], [1, 1, 1, 1], copies=2)
    rec, words = R.records_of(rows)
    text = rng.integers(1, 5, size=sum(lengths)).astype(np.uint8)
    o = R.options(min_depth=1, min_qual=1, prior_het=1, prior_hom=1, max_del=max_del)
    got, al = measure(text, lengths, rec, words, reads, o)
    table = [(int(a["ref"]), int(a["pos"]), int(a["kind"]), int(a["length"]), int(a["count"])) for a in al]
    assert table == [(0, 4, R.INS, 1, 2), (0, 14, R.INS, 2, 2), (0, 24, R.INS, 31, 2), (0, 34, R.INS, 32, 2), (0, 80, R.DEL, 6, 2), (0, 90, R.DEL, 7, 2), (0, 202, R.INS, 3, 2),
                     (0, 220, R.DEL, 5, 2), (0, 220, R.INS, 2, 2), (0, 220, R.INS, 2, 2), (0, 230, R.DEL, 2, 2), (0, 230, R.INS, 1, 2), (0, 240, R.INS, 2, 2), (0, 241, R.INS, 2, 2),
                     (0, 242, R.INS, 2, 2), (0, 260, R.DEL, 1, 3), (0, 260, R.INS, 1, 2), (0, 260, R.INS, 2, 5), (0, 299, R.INS, 2, 2)]
    assert [R.letters_of(a["letters"], a["length"]) for a in al if int(a["pos"]) == 220 and int(a["kind"]) == R.INS] == ["CG", "TA"]
    indel = {int(r["pos"]): r for r in got if int(r["kind"]) != R.SNV and int(r["ref"]) == 0}
    assert (int(indel[220]["kind"]), int(indel[220]["length"])) == (R.DEL, 5) and (int(indel[230]["kind"]), int(indel[230]["length"])) == (R.DEL, 2)      # the tie rule
    r = indel[260]                                                        # cov 10 = events: ref 0, alt 5, oth 5
    assert (int(r["kind"]), int(r["length"]), int(r["ref_count"]), int(r["alt_count"]), int(r["cov"]), R.letters_of(r["letters"], 2)) == (R.INS, 2, 0, 5, 10, "TA")
    assert R.letters_of(indel[202]["letters"], 3) == "TTA" and int(indel[299]["kind"]) == R.INS and 44 not in indel and 100 not in indel
    assert all(int(x["ref"]) == 0 for x in got)


# ------------------------------------------------------------------------------------------------ the call
@gpu
@pytest.mark.parametrize("case", COLUMNS, ids=[c[0] for c in COLUMNS])
def test_the_call_column_by_column(case):
    _, rank, planes, o, ins, dels, rows = case
    text, lengths, rec, words, reads = one_column(rank, planes, o, ins, dels)
    got = same(device(text, lengths, rec, words, reads, o), R.variants(text, lengths, rec, words, reads, o))
    mine = got[0][got[0]["pos"] == 1]
    assert [(int(c["kind"]), int(c["alt_rank"]), int(c["length"]), int(c["ref_count"]), int(c["alt_count"]), int(c["cov"]), int(c["gt"])) for c in mine] == rows


# ------------------------------------------------------------------------------------------------ contention, the grid cap, growth
@gpu
def test_contention_on_one_column_and_one_anchor():
    lengths = [300, 1000]
    n = 6000
    rec = np.zeros(n, dtype=R.REC)
    rec["ref"], rec["pos"], rec["coff"], rec["clen"] = 1, 400, 1, 5       # every record refers to the same five words and the same read
    words = np.array([R.word("=", 9), R.word("=", 60), R.word("I", 3), R.word("X", 1), R.word("D", 2), R.word("=", 39)], dtype=np.uint32)
    read = np.full(103, 2, dtype=np.uint8)
    read[63] = 3
    text = np.full(sum(lengths), 1, dtype=np.uint8)
    got, al = measure(text, lengths, rec, words, [read], R.options(), times=n)      # (the counts are sums over the records)
    assert [(int(a["ref"]), int(a["pos"]), int(a["kind"]), int(a["length"]), int(a["count"])) for a in al] == [(1, 459, R.INS, 3, n), (1, 460, R.DEL, 2, n)]
    at = [(int(c["pos"]), int(c["kind"]), int(c["alt_count"]), int(c["cov"]), int(c["gt"])) for c in got if 455 <= int(c["pos"]) <= 465]
    assert at == [(459, R.INS, n, n, R.AA), (460, R.SNV, n, n, R.AA), (460, R.DEL, n, n, R.AA)]


@gpu
def test_past_the_grid_cap():
    cap, waves, _, _ = F.variants_geometry()
    n = cap * waves + 1                                                   # one record more than a full grid of waves: a wave strides on to a second job
    rec = np.zeros(n, dtype=R.REC)
    rec["ref"], rec["pos"], rec["coff"], rec["clen"] = 0, 7, 0, 4
    words = np.array([R.word("=", 3), R.word("I", 1), R.word("D", 2), R.word("=", 1)], dtype=np.uint32)
    read = np.array([1, 1, 1, 4, 1], dtype=np.uint8)
    text = np.full(64, 1, dtype=np.uint8)
    got, al = measure(text, [64], rec, words, [read], R.options(), times=n)
    assert [(int(a["pos"]), int(a["kind"]), int(a["count"])) for a in al] == [(9, R.DEL, n), (9, R.INS, n)]
    assert [(int(c["pos"]), int(c["kind"]), int(c["alt_count"]), int(c["ref_count"])) for c in got] == [(9, R.DEL, n, 0)]      # the tie: the deletion; oth = n


@gpu
def test_key_buffer_growth_across_adds():
    """the table starts at 65 536 keys: three adds of 30 000 records with two events each grow it twice, and the first adds' keys stay"""
    n = 30_000
    words = np.array([R.word("=", 2), R.word("I", 1), R.word("=", 1), R.word("D", 1), R.word("=", 1)], dtype=np.uint32)
    reads = [np.array([1, 1, 2 + k, 1, 1], dtype=np.uint8) for k in range(3)]
    text = np.full(500, 1, dtype=np.uint8)
    one = np.zeros(3, dtype=R.REC)
    one["ref"], one["pos"], one["coff"], one["clen"], one["read"] = 0, [10, 100, 10], 0, 5, [0, 1, 2]
    c = F.variants(text=text, lengths=[500], options=R.c_options(R.options()))
    for k in range(3):
        c.add_records(np.repeat(one[k: k + 1], n), words, reads)
    c.finish()
    got = results(c)
    c.close()
    want = R.variants(text, [500], one, words, reads, R.options(), times=n)
    same(got, want)
    assert int(got[1]["count"].sum()) == 6 * n and len(got[1]) == 5


# ------------------------------------------------------------------------------------------------ sort and scan geometry
@gpu
@pytest.mark.parametrize("n_keys", [0, 1, 2047, 2048, 2049])
def test_key_counts_round_the_sort_tile(n_keys):
    lengths = [5000]
    # (records i and i + 1500 yield the same key: runs of one and of two keys; every third event is a deletion)
    rows = [(0, 0, (i % 500) * 7, 0, [R.word("=", 2), R.word("D", 1 + i % 2), R.word("=", 1)] if i % 3 == 2 else [R.word("=", 2), R.word("I", 1 + i % 3)]) for i in range(n_keys)]
    rows.append((0, 0, 4500, 0, [R.word("X", 2)]))
    rec, words = R.records_of(rows)
    reads = [np.array([1, 1, 1] if i % 3 == 2 else [1, 1] + [1 + (i % 3 + k) % 4 for k in range(1 + i % 3)], dtype=np.uint8) for i in range(n_keys)] + [np.array([2, 3], dtype=np.uint8)]
    text = np.full(5000, 1, dtype=np.uint8)
    got, al = measure(text, lengths, rec, words, reads, ANY)
    assert int(al["count"].sum()) == n_keys and int((got["kind"] == R.SNV).sum()) == 2


def geometry_totals():
    t, b = F.coverage_geometry()
    return [1, 64, t - 1, t, t + 1, 2 * t + 1, t * b + 1]


@gpu
@pytest.mark.parametrize("which", range(7))
def test_scan_and_call_geometry(which):
    """a text of A: one X column (C, G or T) per tile, on the first and on the last position, a two-letter insertion behind every tile's
    last position and, from two tiles on, a second tile in which every position yields two rows: an X word over the whole tile twice and
    one record of an X column and an I word per position (two words per position: 128 passes of the key kernel). Everything is compared
    with the reference; the largest total puts the row counts' scan on its second level."""
    t, b = F.coverage_geometry()
    total = geometry_totals()[which]
    assert t * b + 1 <= 1 << 28
    tiles = -(-total // t)
    full = total > 2 * t                                                  # the tile [t, 2t) is the one with two rows everywhere
    xs = {min(k * t + (k * 7) % (t - 1), total - 1): 2 + k % 3 for k in range(tiles) if not (full and k == 1)}
    xs.update({0: 3, total - 1: 2})
    anchors = sorted({min((k + 1) * t - 1, total - 1) for k in range(tiles) if not (full and k == 1)} - set(xs))      # (an X column and the = of an insertion's record would tie)
    rows = [(0, 0, p, 0, [R.word("X", 1)]) for p in sorted(xs)] + [(0, 0, p, 0, [R.word("=", 1), R.word("I", 2)]) for p in anchors]
    reads = [np.array([xs[p]], dtype=np.uint8) for p in sorted(xs)] + [np.array([1, 2, 3], dtype=np.uint8)] * len(anchors)
    if full:
        rows += [(0, 0, t, 0, [R.word("X", t)])] * 2 + [(0, 0, t, 0, [R.word("X", 1), R.word("I", 1)] * t)]
        reads += [np.full(t, 3, dtype=np.uint8)] * 2 + [np.tile(np.array([3, 4], dtype=np.uint8), t)]
    rec, words = R.records_of(rows)
    rec["read"] = np.arange(len(rec))
    text = np.full(total, 1, dtype=np.uint8)
    got, al = measure(text, [total], rec, words, reads, ANY)
    assert len(got) == len(xs) + len(anchors) + (2 * t if full else 0)
    if full:
        mine = got[(got["pos"] >= t) & (got["pos"] < 2 * t)]
        assert mine["pos"].tolist() == [t + k // 2 for k in range(2 * t)] and mine["kind"].tolist() == [R.SNV, R.INS] * t
        assert (mine["alt_count"] == np.tile([3, 1], t)).all() and (mine["cov"] == 3).all()


# ------------------------------------------------------------------------------------------------ sequence boundaries
@gpu
def test_sequence_boundaries():
    t, _ = F.coverage_geometry()
    rng = np.random.default_rng(3)
    small = [int(n) for n in rng.integers(1, 4, size=1000)]
    lengths = [t] + small + [t]
    last = len(lengths) - 1
    w = R.word
    rows = [(0, 0, t - 1, 0, [w("X", 1)]), (0, 0, t - 3, 0, [w("=", 3), w("I", 2)]),            # an anchor on a sequence's last position
            (16, last, 0, 0, [w("I", 1), w("X", 1), w("=", 5)]), (0, last, t - 2, 0, [w("D", 1), w("X", 1), w("I", 4)]), (0, last, 0, 0, [w("X", 1), w("D", 3), w("=", 1)])]
    for i, n in enumerate(small):
        r = 1 + i
        if i % 3 == 0:
            rows.append((0, r, n - 1, 0, [w("X", 1)]))                     # the last position of one sequence ..
        if i % 3 == 1:
            rows.append((16, r, 0, 0, [w("X", 1), w("I", 1)] if n == 1 else [w("X", 1), w("=", n - 1), w("I", 2)]))     # .. the first of the next, and an anchor on its last
        if i % 7 == 2:
            rows.append((0, r, 0, 0, [w("D", n)]))                         # a sequence deleted in full between its neighbours: no column in front, no allele
        if i % 7 == 3 and n >= 2:
            rows.append((0, r, 0, 0, [w("X", 1), w("D", n - 1)]))          # a deletion from a sequence's first position to its last
    rec, words, reads = R.records_with_reads(rng, rows)
    for read in reads:
        read[(read == 0) | (read == 5)] = 2
    text = R.random_text(rng, sum(lengths))
    got, al = measure(text, lengths, rec, words, reads, ANY)
    refs = got["ref"].tolist()
    assert refs == sorted(refs) and len(set(refs)) > 400 and refs[0] == 0 and refs[-1] == last
    assert all(int(c["pos"]) < lengths[int(c["ref"])] for c in got) and all(int(a["pos"]) + (int(a["length"]) if int(a["kind"]) == R.DEL else 0) < lengths[int(a["ref"])] for a in al)
    where = {(int(c["ref"]), int(c["pos"])) for c in got}
    assert (0, t - 1) in where and (last, 0) in where and (last, t - 1) in where
    firsts, lasts = {r for r, p in where if p == 0}, {r for r, p in where if p == lengths[r] - 1}
    assert sum(r in lasts and r + 1 in firsts for r in range(last)) > 20  # rows on the last position of one sequence and on the first of the next
    measure(text, lengths, rec, words, reads, R.options(min_depth=1, min_qual=1500, prior_het=1, prior_hom=1, max_del=1), adds=4)


# ------------------------------------------------------------------------------------------------ lifetime, refusals, threads
@gpu
def test_lifetime_and_refusals():
    L = capi.lib()
    lengths = [700, 300]
    rng = np.random.default_rng(1)
    text = R.random_text(rng, 1000)
    rec, words, reads = R.records_with_reads(rng, [(0, 0, 10, 0, [R.word("=", 100), R.word("X", 3)]), (16, 1, 0, 0, [R.word("X", 300)]),
                                                   (0, 0, 600, 0, [R.word("=", 50), R.word("I", 2), R.word("D", 5), R.word("=", 45)])])
    reads[2][50:52] = [2, 4]
    c = F.variants(text=text, lengths=lengths, options=R.c_options(ANY))
    c.add_records(rec, words, reads)
    # one bad record last in a batch of good ones: refused, the sums and the keys stay
    for bad, extra in (([(0, 0, 650, 0, [R.word("=", 51)])], 0), ([(0, 1, 0, 0, [])], 0), ([(0, 2, 0, 0, [R.word("=", 1)])], 0), ([(0, 0, 0, 0, [R.word("M", 5)])], 0),
                       ([(0, 0, 0, 0, [R.word("=", 5)])], 1), ([(0, 0, 0, 0, [R.word("=", 5)])], -1), ([(0, 0, 0, 0, [R.word("S", 5), R.word("I", 1)])], 0)):
        rec2, words2, reads2 = R.records_with_reads(rng, [(0, 0, 0, 0, [R.word("=", 3), R.word("I", 2), R.word("D", 2), R.word("X", 695)])] * 3 + bad)
        if extra:
            reads2[-1] = np.ones(5 + extra, dtype=np.uint8)
        with pytest.raises(F.FloxerError):
            c.add_records(rec2, words2, reads2)
    rec2["read"][-1] = len(reads2)
    with pytest.raises(F.FloxerError, match="read_index"):
        c.add_records(rec2, words2, reads2)
    # the copy calls work only behind finish
    for call in (c.rows, c.alleles):
        with pytest.raises(F.FloxerError, match="flx_variants_finish"):
            call()
    assert L.flx_variants_num_rows(c.h) == 0 and L.flx_variants_num_alleles(c.h) == 0
    c.finish()
    want = R.variants(text, lengths, rec, words, reads, ANY)
    got = same(results(c), want)
    assert len(got[1]) == 2 and len(got[0]) > 100
    # final: add and finish are refused behind finish
    for call in (lambda: c.add_records(rec, words, reads), lambda: c.add_records(rec[:0], words, reads), c.finish):
        with pytest.raises(F.FloxerError, match="finished"):
            call()
    same(results(c), want)
    # a capacity one too small
    n = L.flx_variants_num_rows(c.h)
    out = np.zeros(n, dtype=F.VARIANT_DTYPE)
    assert L.flx_variants_copy_rows(c.h, out.ctypes.data_as(C.POINTER(capi.Variant)), n - 1) == -3 and str(n) in L.flx_last_error().decode()
    assert L.flx_variants_copy_rows(c.h, out.ctypes.data_as(C.POINTER(capi.Variant)), n) == 0 and out.tobytes() == want[0].tobytes()
    al = np.zeros(2, dtype=F.VARIANT_ALLELE_DTYPE)
    assert L.flx_variants_copy_alleles(c.h, al.ctypes.data_as(C.POINTER(capi.VariantAllele)), 1) == -3 and "2 alleles" in L.flx_last_error().decode()
    assert L.flx_variants_copy_alleles(c.h, al.ctypes.data_as(C.POINTER(capi.VariantAllele)), 2) == 0 and al.tobytes() == want[1].tobytes()
    c.close()
    # bad options, lengths and texts
    bad = capi.VariantsOptions()
    bad.reserved[0] = 1
    for make in (lambda: F.variants(text=text, lengths=lengths, options=bad), lambda: F.variants(text=text, lengths=lengths, options=F.variants_options(cost_het=1574)),
                 lambda: F.variants(text=text, lengths=lengths, options=F.variants_options(cost_match=325)), lambda: F.variants(text=text, lengths=lengths, options=F.variants_options(max_del=1 << 28)),
                 lambda: F.variants(text=text, lengths=[700, 301]), lambda: F.variants(text=text[:0], lengths=[]), lambda: F.variants(text=np.full(1000, 6, dtype=np.uint8), lengths=lengths),
                 lambda: F.variants(text=text, lengths=lengths, device=-1), lambda: F.variants()):
        with pytest.raises(F.FloxerError):
            make()


@gpu
def test_four_adding_threads_equal_one_add():
    lengths = [5000, 12_345, 70, 9000]
    rng = np.random.default_rng(77)
    rec, words = P.random_records(rng, lengths, 3000, max_words=140)
    reads = P.attach_reads(rng, rec, words)
    for read in reads:
        read[:] = 1 + (np.arange(len(read)) // 3) % 4                      # alike reads: alleles repeat
    text = R.random_text(rng, sum(lengths))
    o = R.options(count_secondary=True, min_depth=2, min_qual=100, max_del=8, prior_het=300, prior_hom=400)      # (the depth is low: weak priors let indels through)
    want = R.variants(text, lengths, rec, words, reads, o)
    assert len(want[1]) > 100 and int(want[1]["count"].max()) > 1 and {R.SNV, R.DEL, R.INS} <= {int(k) for k in want[0]["kind"]} and {R.RA, R.AA} <= {int(g) for g in want[0]["gt"]}
    same(device(text, lengths, rec, words, reads, o), want)
    same(device(text, lengths, rec, words, reads, o, adds=7), want)       # several adds equal one add
    c = F.variants(text=text, lengths=lengths, options=R.c_options(o))
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
    same(results(c), want)
    c.close()


# ------------------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def sample():
    from test_pileup_gpu import SAMPLE_RATE
    chroms, reads, snvs, indels = sample_batch()
    ctx = F.context(F.fmindex(chroms))
    yield dict(chroms=chroms, reads=reads, ctx=ctx, rate=SAMPLE_RATE, snvs=snvs)
    ctx.close()


def aligner_of(sample, **kw):
    """the tool's alignment options: duplicates dropped, one alignment per read, indels left-aligned"""
    return F.aligner(sample["ctx"], F.params(error_probability=sample["rate"]), output=F.output_options(True, 1, False), gaps=F.gap_options(), **kw)


def run_against_reference(sample, runs, o):
    """variants.add of every (run, reads) against the reference on the runs' own records, words and reads, joined"""
    chroms = sample["chroms"]
    lengths = [len(c) for c in chroms]
    c = F.variants(sample["ctx"], R.c_options(o))
    parts, all_reads = [], []
    for run, reads in runs:
        c.add(run, reads)
        raw = run.raw.copy()
        raw["read"] += len(all_reads)
        parts.append((raw, run.cigars))
        all_reads += list(reads)
    c.finish()
    got = results(c)
    c.close()
    rec, words = coverage_ref.joined(parts)
    return same(got, R.variants(np.concatenate(chroms), lengths, rec, words, all_reads, o))


@gpu
def test_pipeline(sample):
    reads = sample["reads"]
    al = aligner_of(sample)
    whole = al.align_reads(reads)
    half = len(reads) // 2
    o = R.options()
    one = run_against_reference(sample, [(whole, reads)], o)
    two = run_against_reference(sample, [(al.align_reads(reads[:half]), reads[:half]), (al.align_reads(reads[half:]), reads[half:])], o)
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
    assert {0, 16} <= {int(f) & 16 for f in whole.raw["flag"]} and len(one[1]) > 10
    rows = {(int(c["ref"]), int(c["pos"]), int(c["kind"])): c for c in one[0]}
    for ref, pos, rank in sample["snvs"]:                                 # every planted SNV of the sample is homozygous
        c = rows.get((ref, pos, R.SNV))
        assert c is not None and int(c["alt_rank"]) == rank and int(c["gt"]) == R.AA, (ref, pos)


@gpu
def test_pipeline_refusals(sample):
    reads = sample["reads"][:40]
    ctx = sample["ctx"]
    plain = aligner_of(sample).align_reads(reads)
    c = F.variants(ctx, F.variants_options(min_mapq=2))
    with pytest.raises(F.FloxerError, match="mapq"):                     # a run made without mapq holds no mapping quality
        c.add(plain, reads)
    L = capi.lib()
    pool, offs, n = F._pool_and_offsets(reads)
    raw = C.c_void_p()
    capi.check(L.flx_align_reads(ctx.h, C.byref(F.params(error_probability=sample["rate"])), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n, C.byref(raw)))
    with pytest.raises(F.FloxerError, match="mapq"):
        c.add(raw, reads)
    L.flx_run_free(raw)
    with pytest.raises(F.FloxerError, match="variants"):                 # the context waits for its variants objects
        capi.check(L.flx_ctx_destroy(ctx.h))
    c.close()
    bare = F.aligner(ctx, F.params(error_probability=sample["rate"], without_cigar=True)).align_reads(reads)
    c = F.variants(ctx)
    with pytest.raises(F.FloxerError, match="without_cigar"):
        c.add(bare, reads)
    c.add(plain, reads)                                                   # refused adds left the object as it was
    c.finish()
    lengths = [len(x) for x in sample["chroms"]]
    same(results(c), R.variants(np.concatenate(sample["chroms"]), lengths, plain.raw, plain.cigars, reads, R.options()))
    c.close()


# ------------------------------------------------------------------------------------------------ the tool
@gpu
def test_tool_files(sample, tmp_path):
    from test_md_gpu import letters
    chroms, reads = sample["chroms"], sample["reads"]
    work = tmp_path / "work"
    work.mkdir()
    fasta, fastq, out = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq"), str(work / "calls.vcf")
    with open(fasta, "w") as f:
        for i, c in enumerate(chroms):
            f.write(f">chr{i} sample\n" + "\n".join(letters(c[o: o + 80]) for o in range(0, len(c), 80)) + "\n")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
    exe = os.path.join(ROOT, "floxer_amd", "floxer_variants")
    base = [exe, "--reference", fasta, "--queries", fastq, "--error-probability", str(sample["rate"])]
    env = dict(os.environ, FLX_BATCH_READS="64")                          # several batches
    r = subprocess.run(base + ["--output", out, "--min-qual", "10", "--sample", "S1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    assert os.listdir(work) == ["calls.vcf"] and sorted(os.listdir(tmp_path)) == ["reads.fastq", "ref.fasta", "work"]
    # the tool's costs for a read error of 0.04 (its --error-probability) and a heterozygosity of 0.001, through its own parse-only switch
    p = subprocess.run(base + ["--output", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, FLX_VARIANTS_PARSE_ONLY="1"))
    d = dict(l.split("=", 1) for l in p.stderr.decode().splitlines())
    costs = dict(cost_match=int(d["cost-match"]), cost_mismatch=int(d["cost-mismatch"]), cost_het=int(d["cost-het"]), prior_het=int(d["prior-het"]), prior_hom=int(d["prior-hom"]))
    assert costs == dict(cost_match=18, cost_mismatch=1875, cost_het=313, prior_het=3000, prior_hom=3301)      # -1000 log10 of 0.96, 0.04 / 3, 0.48 + 0.04 / 6
    c = F.variants(sample["ctx"], F.variants_options(min_qual=1000, **costs))
    c.add(aligner_of(sample).align_reads(reads), reads)
    c.finish()
    rows = c.rows()
    c.close()
    header = ["##fileformat=VCFv4.2\n", "##source=floxer_variants\n"] + [f"##contig=<ID=chr{i},length={len(x)}>\n" for i, x in enumerate(chroms)]
    got = open(out).readlines()
    assert got[: len(header)] == header and got[-len(rows) - 1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"
    meta = got[len(header): -len(rows) - 1]
    assert [l.split(",")[0] for l in meta] == ["##INFO=<ID=DP", "##FORMAT=<ID=GT", "##FORMAT=<ID=GQ", "##FORMAT=<ID=DP", "##FORMAT=<ID=AD", "##FORMAT=<ID=PL"]
    assert got[-len(rows):] == R.vcf_lines(rows, ["chr0", "chr1"], chroms) and len(rows) >= 8
    assert {R.SNV, R.DEL, R.INS} <= {int(k) for k in rows["kind"]}
    r = subprocess.run(base + ["--output", str(work / "other.bcf")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 255 and r.stderr.startswith(b"[CLI PARSER ERROR]\n") and b"[vcf]" in r.stderr and os.listdir(work) == ["calls.vcf"]
