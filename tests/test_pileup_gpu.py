"""Allele pileup on the GPU (flx_pileup: kernels pileup_add and pileup_sites behind coverage's scan and sum; runs, the Python class and the
CLI's --pileup output). Every expected value is the plain-numpy rule of tests/pileup_ref.py on the same records, words and reads; the
shapes sit on the kernels' boundaries (64 CIGAR words per pass, the scan's tile and second level)."""
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
import pileup_ref as R

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = R.options(min_depth=1, min_count=1, min_permille=1)               # every position with a letter, a deletion or an insertion is a site


def device_counts(p, lengths):
    return np.concatenate([p.counts(r, 0, n) for r, n in enumerate(lengths)], axis=1)


def same(p, lengths, want, o):
    """counts and sites of a finished object against the reference's on the expected counts"""
    got = device_counts(p, lengths)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (bad[:8], [(int(got[k, i]), int(want[k, i])) for k, i in bad[:8]])
    sites, exp = p.sites(), R.sites(lengths, want, o)
    assert len(sites) == len(exp) and sites.tobytes() == exp.tobytes()
    return got, sites


def measure(lengths, rec, words, reads, o, adds=1):
    p = F.pileup(lengths=lengths, options=R.c_options(o))
    try:
        for part in np.array_split(np.arange(len(rec)), adds):
            p.add_records(rec[part], words, reads)
        p.finish()
        return same(p, lengths, R.counts(lengths, rec, words, reads, o), o)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ words and carries
def body_words(rng, n, max_len=9):
    """n words: = runs with X, I and D between them, X on both sides of every pass boundary; the first and the last consume reference"""
    ws = [("=" if t % 2 == 0 else "XID"[int(rng.integers(0, 3))], int(rng.integers(1, max_len + 1))) for t in range(n)]
    for t in (63, 64, 127, 128, 4095, 4096):
        if t < n:
            ws[t] = ("X", ws[t][1])
    if ws[-1][0] == "I":
        ws[-1] = ("X", ws[-1][1])
    return [R.word(op, ln) for op, ln in ws]


def special_rows():
    """the anchor and row carries on their own: (flag, ref, pos, mapq, words)"""
    w = R.word
    return [
        (0, 0, 100, 0, [w("S", 5), w("I", 2), w("=", 30), w("X", 2), w("=", 4)]),            # an I directly behind the leading S
        (16, 0, 200, 0, [w("I", 3), w("=", 30), w("X", 1)]),                                  # an I as the very first word
        (0, 0, 300, 0, [w("=", 10), w("D", 4), w("I", 2), w("X", 3), w("=", 5)]),            # an I directly behind a D
        (16, 0, 400, 0, [w("S", 9), w("=", 20), w("X", 2), w("I", 4), w("S", 6)]),           # an I as the last word in front of a trailing S
        (0, 0, 500, 0, [w("=", 3), w("X", 70), w("=", 2), w("I", 70), w("X", 1)]),           # an X word and an I word of 70 columns each
        (16, 0, 500, 0, [w("S", 1), w("X", 70), w("I", 70), w("=", 6), w("S", 2)]),
        (0, 0, 0, 0, [w("D", 2), w("I", 1), w("X", 2)]),                                      # starts at position 0 of a sequence, with a D, an I on it
    ]


@gpu
@pytest.mark.parametrize("n_words", [1, 63, 64, 65, 129, 4097])
def test_words_and_carries(n_words):
    rng = np.random.default_rng(n_words)
    lengths = [45_000, 33_000]
    body = body_words(rng, n_words)
    inner = body_words(rng, max(1, n_words - 2))
    clipped = ([R.word("S", 7)] + inner + [R.word("S", 5)]) if n_words >= 3 else inner        # the row carry starts at 7
    d_inner = body_words(rng, max(1, n_words - 4))
    d_ends = ([R.word("S", 3), R.word("D", 3)] + d_inner + [R.word("D", 4), R.word("S", 2)]) if n_words >= 5 else [R.word("D", 3)] + d_inner + [R.word("D", 4)]
    rows = [(0, 0, 1011, 0, body), (16, 0, 2000, 0, body), (16, 1, 0, 0, clipped), (0, 1, 5, 0, clipped),
            (2048, 0, 45_000 - R.span(d_ends), 0, d_ends),                                    # a D as first and as last reference word; ends on the sequence's last position
            (16, 1, 33_000 - R.span(body), 0, body)] + special_rows()
    assert len(body) == n_words and (n_words < 3 or len(clipped) == n_words) and all(R.span(r[4]) <= 33_000 for r in rows)
    rec, words, reads = R.records_with_reads(rng, rows)
    got, sites = measure(lengths, rec, words, reads, ANY)
    assert got[R.INS].sum() >= 7 and got[R.DEL].sum() >= 13 and got[R.A:R.T + 1].sum() > 70 and len(sites) > 20
    assert got[R.INS][100] == 1 and got[R.INS][200] == 1                                      # an I in front of every column sits on the record's first column
    assert got[R.INS][1] == 1 and got[R.DEL][0] == 1 and got[R.DEL][45_000 - 1] == 1
    if n_words >= 65:
        ops = [int(x) & 15 for x in body]
        assert ops[63] == ops[64] == 8                                     # X words on both sides of a pass boundary
    measure(lengths, rec, words, reads, R.options(), adds=3)


# ------------------------------------------------------------------------------------------------ letters
@gpu
def test_letters_and_strands():
    lengths = [40, 40]
    read = np.array([1, 2, 3, 4, 5, 0, 1, 1, 4, 2], dtype=np.uint8)
    ws = [R.word("X", 10)]
    rec, words = R.records_of([(0, 0, 3, 0, ws), (16, 1, 3, 0, ws)])
    rec["read"] = 0                                                        # the same read, forward and reverse complemented
    got, _ = measure(lengths, rec, words, [read], ANY)
    fw, rv = got[:, 3:13], got[:, 43:53]
    assert (fw[R.DEPTH] == 1).all() and (rv[R.DEPTH] == 1).all()
    assert fw[R.A:R.T + 1].sum() == 8 and fw[R.A:R.T + 1, 4:6].sum() == 0   # ranks 5 and 0 count in DEPTH only
    assert (fw[R.A:R.T + 1] == rv[R.A:R.T + 1][::-1, ::-1]).all()           # complementary planes at mirrored columns
    assert fw[R.A].tolist() == [1, 0, 0, 0, 0, 0, 1, 1, 0, 0] and rv[R.T].tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 0, 1]


# ------------------------------------------------------------------------------------------------ contention, filters
@gpu
def test_contention_on_one_column_and_one_anchor():
    lengths = [300, 1000]
    n = 20_000
    rec = np.zeros(n, dtype=R.REC)
    rec["ref"], rec["pos"], rec["coff"], rec["clen"] = 1, 400, 1, 3       # every record refers to the same three words and the same read
    words = np.array([R.word("=", 9), R.word("=", 60), R.word("I", 3), R.word("X", 1), R.word("=", 39)], dtype=np.uint32)
    read = np.full(64, 2, dtype=np.uint8)
    read[63] = 3
    p = F.pileup(lengths=lengths)
    p.add_records(rec, words, [read])
    p.finish()
    want = R.counts(lengths, rec[:1], words, [read], R.options()).astype(np.int64) * n           # (the counts are sums over the records)
    got, sites = same(p, lengths, want.astype(np.uint32), R.options())
    p.close()
    at = 300 + 400
    assert got[R.G][at + 60] == n and got[R.G].sum() == n and got[R.INS][at + 59] == n and got[R.INS].sum() == n
    assert got[[R.A, R.C, R.T, R.DEL]].sum() == 0 and (got[R.DEPTH][at: at + 61] == n).all() and got[R.DEPTH].sum() == 61 * n
    assert sites[["ref", "pos", "depth", "ins"]].tolist() == [(1, 459, n, n), (1, 460, n, 0)] and sites["alt"].tolist() == [[0, 0, 0, 0], [0, 0, n, 0]]


@gpu
@pytest.mark.parametrize("secondary", [False, True])
@pytest.mark.parametrize("min_mapq", [0, 1, 60])
def test_filters(secondary, min_mapq):
    lengths = [4000]
    rows, at = [], 0
    for flag in (0, 16, 256, 272, 2048, 2064, 4):
        for mapq in (0, 3, 60):
            rows.append((flag, 0, at, mapq, [R.word("=", 50), R.word("X", 2), R.word("I", 1), R.word("D", 2)]))
            at += 100
    rec, words = R.records_of(rows)
    reads = [np.array([1] * 50 + [2, 3, 4], dtype=np.uint8)] * len(rows)
    rec["read"] = np.arange(len(rows))
    o = dict(ANY, count_secondary=secondary, min_mapq=min_mapq)
    got, sites = measure(lengths, rec, words, reads, o)
    counted = [(f, q) for f in (0, 16, 2048, 2064) + ((256, 272) if secondary else ()) for q in (0, 3, 60) if q >= min_mapq]
    assert int(got[R.DEPTH].sum()) == 52 * len(counted) and int(got[R.INS].sum()) == len(counted) and int(got[R.DEL].sum()) == 2 * len(counted)
    assert len(sites) == 4 * len(counted)                                # (the anchor is the second X column)


# ------------------------------------------------------------------------------------------------ scan and site geometry
def geometry_totals():
    t, b = F.coverage_geometry()
    return [1, 64, t - 1, t, t + 1, 2 * t + 1, t * b + 1]


def expected_sites(total, dels, xs):
    """the sites (thresholds 1, 1, 1) of one sequence with `dels` records of one D word over everything and X columns xs = {position: rank}"""
    at = np.arange(total) if dels else np.array(sorted(xs), dtype=np.int64)
    out = np.zeros(len(at), dtype=F.SITE_DTYPE)
    out["pos"], out["del"] = at, dels
    for p, r in xs.items():
        i = p if dels else int(np.searchsorted(at, p))
        out["depth"][i] = 1
        out["alt"][i][r - 1] = 1
    return out


@gpu
@pytest.mark.parametrize("which", range(7))
def test_scan_and_site_geometry(which):
    t, b = F.coverage_geometry()
    total = geometry_totals()[which]
    assert t * b + 1 <= 1 << 28
    lengths = [total]
    small = total <= 2 * t + 1                                            # the whole count array is compared there; beyond, the sites and stretches
    tiles = -(-total // t)
    per_tile = {min(k * t + (k * 7) % t, total - 1): 1 + k % 4 for k in range(tiles)}
    ends = {0: 3, total - 1: 2}
    cases = [("every position a site", 1, per_tile), ("one site per tile", 0, per_tile), ("the first and the last position", 0, ends), ("no site", 0, {})]
    for name, dels, xs in cases:
        rows = [(0, 0, 0, 0, [R.word("D", total)])] * dels + [(16 if p % 2 else 0, 0, p, 0, [R.word("X", 1)]) for p in sorted(xs)]
        rec, words = R.records_of(rows) if rows else (np.zeros(0, dtype=R.REC), np.zeros(1, dtype=np.uint32))
        reads = [np.zeros(0, np.uint8)] * dels + [np.array([5 - xs[p] if p % 2 else xs[p]], dtype=np.uint8) for p in sorted(xs)]      # (flag 16: the complement goes in)
        rec["read"] = np.arange(len(rec))
        exp = expected_sites(total, dels, xs)
        p = F.pileup(lengths=lengths, options=R.c_options(ANY))
        p.add_records(rec, words, reads)
        p.finish()
        if small:
            want = R.counts(lengths, rec, words, reads, ANY)
            assert R.sites(lengths, want, ANY).tobytes() == exp.tobytes(), name                  # the closed form is pileup_ref's
            same(p, lengths, want, ANY)
        sites = p.sites()
        assert len(sites) == len(exp), (name, len(sites), len(exp))
        for field in ("ref", "pos", "depth", "del", "ins", "alt", "res"):
            assert (sites[field] == exp[field]).all(), (name, field)
        for a in sorted({0, max(0, total - 70), max(0, min(total - 70, t * b - 30))}):           # stretches: the start, the end, across the second level
            c = p.counts(0, a, min(total, a + 70))
            assert (c[R.DEL] == dels).all() and c[R.INS].sum() == 0 and c[R.DEPTH].sum() == sum(1 for q in xs if a <= q < a + 70), (name, a)
        p.close()
        # the same records under the default thresholds (4, 2, 200): depth 2 at the most, so no site
        p = F.pileup(lengths=lengths)
        p.add_records(rec, words, reads)
        p.finish()
        assert len(p.sites()) == 0, name
        p.close()


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
            (16, last, 0, 0, [w("I", 1), w("X", 1), w("=", 5)]), (0, last, t - 2, 0, [w("D", 1), w("X", 1), w("I", 4)])]
    for i, n in enumerate(small):
        r = 1 + i
        if i % 3 == 0:
            rows.append((0, r, n - 1, 0, [w("X", 1)]))                     # the last position of one sequence ..
        if i % 3 == 1:
            rows.append((16, r, 0, 0, [w("X", 1), w("I", 1)] if n == 1 else [w("X", 1), w("=", n - 1), w("I", 2)]))     # .. the first of the next, and an anchor on its last
        if i % 7 == 2:
            rows.append((0, r, 0, 0, [w("D", n)]))
    rec, words, reads = R.records_with_reads(rng, rows)
    for read in reads:
        read[(read == 0) | (read == 5)] = 2                                # letters only: every X column is a site
    got, sites = measure(lengths, rec, words, reads, ANY)
    starts = R.starts_of(lengths)
    assert got[R.INS][t - 1] == 1 and got[R.INS][t] == 0 and got[R.INS][starts[last]] == 1 and got[R.INS][-1] == 1
    refs = sites["ref"].tolist()
    assert refs == sorted(refs) and len(set(refs)) > 600 and refs[0] == 0 and refs[-1] == last
    assert all(int(s["pos"]) < lengths[int(s["ref"])] for s in sites)
    measure(lengths, rec, words, reads, R.options(min_depth=1, min_count=1, min_permille=1000), adds=4)


# ------------------------------------------------------------------------------------------------ order, lifetime
@gpu
def test_order_of_adds_threads_and_absorb():
    lengths = [5000, 12_345, 70, 9000]
    rng = np.random.default_rng(77)
    rec, words = R.random_records(rng, lengths, 3000, max_words=140)
    reads = R.attach_reads(rng, rec, words)
    o = R.options(count_secondary=True, min_depth=2, min_count=1, min_permille=100)
    want = R.counts(lengths, rec, words, reads, o)
    assert want[R.DEPTH].max() > 3 and len(R.sites(lengths, want, o)) > 100

    def make():
        return F.pileup(lengths=lengths, options=R.c_options(o))
    one, ten, threaded, into, other = make(), make(), make(), make(), make()
    one.add_records(rec, words, reads)
    for part in np.array_split(np.arange(len(rec)), 10):
        ten.add_records(rec[part], words, reads)
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
    other.add_records(rec[1700:], words, reads)
    into.absorb(other)
    results = []
    for p in (one, ten, threaded, into):
        p.finish()
        got, sites = same(p, lengths, want, o)
        results.append((got.tobytes(), sites.tobytes()))
    assert all(r == results[0] for r in results)
    other.finish()                                                        # absorbed: left cleared
    assert len(other.sites()) == 0 and int(device_counts(other, lengths).sum()) == 0
    for p in (one, ten, threaded, into, other):
        p.close()


@gpu
def test_absorb_across_pieces():
    """absorb moves every plane in pieces of 4 << 20 entries: here a plane's total + 1 entries are one full piece and one piece of 6"""
    piece, tail = 4 << 20, 5
    lengths = [piece + tail]
    rng = np.random.default_rng(43)
    rec, words = R.records_across(rng, piece, tail)
    reads = R.attach_reads(rng, rec, words)
    o = dict(ANY, count_secondary=True)
    want = R.counts(lengths, rec, words, reads, o)
    stretches = [(0, 300), (piece - 300, piece + tail)]                   # the two ends and both sides of the piece boundary
    for half in (rec[::2], rec[1::2]):                                    # both objects hold counts there
        part = R.counts(lengths, half, words, reads, o)
        assert part[R.DEPTH][[0, piece - 1, piece, -1]].min() > 0 and part[R.INS][piece - 1] > 0 and part[R.DEL][piece + 1] > 0
        assert all((part[:, a:b].sum(axis=1) > 0).all() for a, b in stretches)
    into, other = F.pileup(lengths=lengths, options=R.c_options(o)), F.pileup(lengths=lengths, options=R.c_options(o))
    into.add_records(rec[::2], words, reads)
    other.add_records(rec[1::2], words, reads)
    into.absorb(other)
    into.finish()
    for a, b in stretches:
        got = into.counts(0, a, b)
        bad = np.argwhere(got != want[:, a:b])
        assert len(bad) == 0, (a, bad[:8])
    sites, exp = into.sites(), R.sites(lengths, want, o)
    assert len(sites) == len(exp) and sites.tobytes() == exp.tobytes() and len(exp) > 300
    other.finish()                                                        # absorbed: left cleared, in both pieces of every plane
    assert len(other.sites()) == 0 and all(int(other.counts(0, a, b).sum()) == 0 for a, b in stretches)
    into.close()
    other.close()


@gpu
def test_lifetime_and_refusals():
    L = capi.lib()
    lengths = [700, 300]
    rng = np.random.default_rng(1)
    rec, words, reads = R.records_with_reads(rng, [(0, 0, 10, 0, [R.word("=", 100), R.word("X", 3)]), (16, 1, 0, 0, [R.word("X", 300)]),
                                                   (0, 0, 600, 0, [R.word("=", 50), R.word("I", 2), R.word("D", 50)])])
    p, twin = F.pileup(lengths=lengths, options=R.c_options(ANY)), F.pileup(lengths=lengths, options=R.c_options(ANY))
    p.add_records(rec, words, reads)
    # one bad record last in a batch of good ones: refused, the counts stay
    for bad, extra in (([(0, 0, 650, 0, [R.word("=", 51)])], 0), ([(0, 1, 0, 0, [])], 0), ([(0, 2, 0, 0, [R.word("=", 1)])], 0), ([(0, 0, 0, 0, [R.word("M", 5)])], 0),
                       ([(0, 0, 0, 0, [R.word("=", 5)])], 1), ([(0, 0, 0, 0, [R.word("=", 5)])], -1), ([(0, 0, 0, 0, [R.word("S", 5), R.word("I", 1)])], 0)):
        rec2, words2, reads2 = R.records_with_reads(rng, [(0, 0, 0, 0, [R.word("X", 700)])] * 3 + bad)
        if extra:
            reads2[-1] = np.ones(5 + extra, dtype=np.uint8)
        with pytest.raises(F.FloxerError):
            p.add_records(rec2, words2, reads2)
    rec2["read"][-1] = len(reads2)
    with pytest.raises(F.FloxerError, match="read_index"):
        p.add_records(rec2, words2, reads2)
    # the copy calls work only behind finish
    with pytest.raises(F.FloxerError):
        p.sites()
    with pytest.raises(F.FloxerError):
        p.counts(0, 0, 10)
    assert L.flx_pileup_num_sites(p.h) == 0
    # absorb: other lengths, other options, itself
    for other in (F.pileup(lengths=[700, 301]), F.pileup(lengths=[1000]), F.pileup(lengths=lengths), F.pileup(lengths=lengths, options=F.pileup_options(True, 0, 1, 1, 1)),
                  F.pileup(lengths=lengths, options=F.pileup_options(False, 0, 1, 1, 2))):
        with pytest.raises(F.FloxerError):
            p.absorb(other)
        with pytest.raises(F.FloxerError):
            other.absorb(p)
        other.close()
    with pytest.raises(F.FloxerError):
        p.absorb(p)
    p.finish()
    want = R.counts(lengths, rec, words, reads, ANY)
    same(p, lengths, want, ANY)
    # final: add, absorb (either way round) and finish are refused behind finish
    for call in (lambda: p.add_records(rec, words, reads), lambda: p.add_records(rec[:0], words, reads), lambda: p.absorb(twin), lambda: twin.absorb(p), p.finish):
        with pytest.raises(F.FloxerError):
            call()
    _, sites = same(p, lengths, want, ANY)
    n = L.flx_pileup_num_sites(p.h)
    assert n == len(sites) and n > 200
    out = np.zeros(n, dtype=F.SITE_DTYPE)
    assert L.flx_pileup_copy_sites(p.h, out.ctypes.data_as(C.POINTER(capi.PileupSite)), n - 1) == -3            # FLX_ERR_CAPACITY, one slot too few
    assert str(n) in L.flx_last_error().decode()
    assert L.flx_pileup_copy_sites(p.h, out.ctypes.data_as(C.POINTER(capi.PileupSite)), n) == 0 and out.tobytes() == sites.tobytes()
    with pytest.raises(F.FloxerError):
        p.counts(0, 0, 701)
    with pytest.raises(F.FloxerError):
        p.counts(2, 0, 1)
    bad = capi.PileupOptions()
    bad.reserved[0] = 1
    for make in (lambda: F.pileup(lengths=lengths, options=bad), lambda: F.pileup(lengths=lengths, options=F.pileup_options(min_permille=1001)),
                 lambda: F.pileup(lengths=[5, 1 << 31]), lambda: F.pileup(lengths=[])):
        with pytest.raises(F.FloxerError):
            make()
    p.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ pipeline
# Seed 29 was checked: on the CPU oracle's records of this batch (default output, and with the secondaries counted) pileup_ref's sites
# satisfy planted_variants_found under the default thresholds and at 300 permille. That is a property of the alignments, not of the kernels.
SAMPLE_SEED = 29
SAMPLE_RATE = 0.04


def sample_batch():
    """two references of about 20 kb, a sample copy with planted SNVs, one 3-base deletion and one 2-base insertion, and reads drawn
    from the sample on both strands at about twelve-fold depth with 1 % errors. Returns (chroms, reads, snvs, indels): snvs =
    [(ref, position, planted rank)], indels = [(ref, position, plane)] in reference coordinates."""
    rng = np.random.default_rng(SAMPLE_SEED)
    chroms = S.make_genome(20_000, 2, seed=SAMPLE_SEED)
    sample = [c.copy() for c in chroms]
    snvs = []
    for ref, pos in ((0, 1500), (0, 7321), (0, 15_000), (1, 2222), (1, 9000), (1, 18_111)):
        sample[ref][pos] = 1 + (int(chroms[ref][pos]) - 1 + int(rng.integers(1, 4))) % 4
        snvs.append((ref, pos, int(sample[ref][pos])))
    sample[0] = np.concatenate([sample[0][:11_000], sample[0][11_003:]])                        # the deletion
    sample[1] = np.concatenate([sample[1][:12_500], np.array([1, 3], dtype=np.uint8), sample[1][12_500:]])      # the insertion
    reads = S.make_reads(sample, 480, 1000, 0.01, seed=SAMPLE_SEED + 1)[0]
    return chroms, reads, snvs, [(0, 11_000, R.DEL), (1, 12_500, R.INS)]


def planted_variants_found(lengths, cnt, snvs, indels, o):
    """every planted SNV is a site whose largest plane is the planted letter; a DEL or INS site lies within three positions of each indel"""
    sites = R.sites(lengths, cnt, o)
    by_pos = {(int(s["ref"]), int(s["pos"])): s for s in sites}
    for ref, pos, rank in snvs:
        s = by_pos.get((ref, pos))
        assert s is not None, (ref, pos)
        planes = [int(s["del"])] + [int(x) for x in s["alt"]] + [int(s["ins"])]
        assert planes.index(max(planes)) == rank and planes.count(max(planes)) == 1, (ref, pos, planes)
    for ref, pos, plane in indels:
        near = [s for s in sites if int(s["ref"]) == ref and abs(int(s["pos"]) - pos) <= 3]
        assert any(int(s["del" if plane == R.DEL else "ins"]) >= max([int(s["del"])] + [int(x) for x in s["alt"]] + [int(s["ins"])]) for s in near), (ref, pos)
    return sites


@pytest.fixture(scope="module")
def planted():
    from test_md_gpu import RATE, _planted
    chroms, reads = _planted()
    ctx = F.context(F.fmindex(chroms))
    yield dict(chroms=chroms, reads=reads, ctx=ctx, rate=RATE)
    ctx.close()


@pytest.fixture(scope="module")
def sample():
    chroms, reads, snvs, indels = sample_batch()
    ctx = F.context(F.fmindex(chroms))
    yield dict(chroms=chroms, reads=reads, ctx=ctx, rate=SAMPLE_RATE, snvs=snvs, indels=indels)
    ctx.close()


def run_against_reference(ctx, lengths, runs, o):
    """pileup.add of every (run, reads) against the reference on the runs' own records, words and reads"""
    p = F.pileup(ctx, R.c_options(o))
    want = np.zeros((7, sum(lengths)), dtype=np.uint32)
    for run, reads in runs:
        p.add(run, reads)
        want += R.counts(lengths, run.raw, run.cigars, reads, o)
    p.finish()
    got, sites = same(p, lengths, want, o)
    p.close()
    return want, (got.tobytes(), sites.tobytes())


CONFIGS = {
    "default": (dict(), R.options()),
    "selected": (dict(output=F.output_options(True, 1, True)), R.options(min_mapq=1)),
    "secondary": (dict(), R.options(count_secondary=True, min_depth=2)),
    "left_aligned": (dict(gaps=F.gap_options()), R.options()),
    "realigned": (dict(gaps=F.gap_options(), realign=F.realign_options()), R.options(count_secondary=True)),
}


@gpu
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("world", ["planted", "sample"])
def test_pipeline_runs(request, world, config):
    w = request.getfixturevalue(world)
    chroms, reads, ctx = w["chroms"], w["reads"], w["ctx"]
    lengths = [len(c) for c in chroms]
    kw, o = CONFIGS[config]
    al = F.aligner(ctx, F.params(error_probability=w["rate"]), **kw)
    whole = al.align_reads(reads)
    half = len(reads) // 2
    want, out = run_against_reference(ctx, lengths, [(whole, reads)], o)
    want2, out2 = run_against_reference(ctx, lengths, [(al.align_reads(reads[:half]), reads[:half]), (al.align_reads(reads[half:]), reads[half:])], o)
    assert (want == want2).all() and out == out2
    assert want[R.DEPTH].max() >= 2 and want[R.A:R.T + 1].sum() > 0 and want[R.DEL].sum() > 0 and want[R.INS].sum() > 0
    assert {0, 16} <= {int(f) & 16 for f in whole.raw["flag"]}
    if world == "sample":
        planted_variants_found(lengths, want, w["snvs"], w["indels"], o)


def raw_run(ctx, p, reads, output=None, gaps=None, realign=None):
    """an unfreed flx_run handle of host reads or of a resident batch"""
    L = capi.lib()
    run = C.c_void_p()
    bundle = capi.RunOptions()
    if output is not None:
        bundle.output = C.pointer(output)
    g = C.byref(gaps) if gaps is not None else None
    r = C.byref(realign) if realign is not None else None
    if isinstance(reads, F.resident_reads):
        capi.check(L.flx_align_reads_resident_realign(ctx.h, C.byref(p), reads.h, C.byref(bundle), None, g, r, C.byref(run)))
    else:
        pool, offs, n = F._pool_and_offsets(reads)
        capi.check(L.flx_align_reads_realign(ctx.h, C.byref(p), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n, C.byref(bundle), None, g, r, C.byref(run)))
    return run


@gpu
@pytest.mark.parametrize("indels", [False, True])
def test_pipeline_raw_runs_host_and_resident_reads(sample, monkeypatch, indels):
    chroms, reads, ctx = sample["chroms"], sample["reads"], sample["ctx"]
    lengths = [len(c) for c in chroms]
    L = capi.lib()
    p = F.params(error_probability=sample["rate"])
    kw = dict(gaps=F.gap_options(), realign=F.realign_options()) if indels else {}
    o = R.options()
    result = F.aligner(ctx, p, **kw).align_reads(reads)
    want = R.counts(lengths, result.raw, result.cigars, reads, o)
    resident = F.resident_reads(ctx, reads)
    monkeypatch.setenv("FLX_CHUNK_READS", "50")                           # several parts, each with its own word pool
    runs = [raw_run(ctx, p, reads, **kw), raw_run(ctx, p, resident, **kw)]
    monkeypatch.delenv("FLX_CHUNK_READS")
    outs = []
    for run, given in ((runs[0], reads), (runs[1], resident), (runs[0], resident), (runs[1], reads)):
        pile = F.pileup(ctx)
        pile.add(run, given)
        pile.finish()
        got, sites = same(pile, lengths, want, o)
        outs.append((got.tobytes(), sites.tobytes()))
        pile.close()
    assert all(x == outs[0] for x in outs)
    # a read batch that does not fit the run's records is refused, the counts stay
    pile = F.pileup(ctx)
    with pytest.raises(F.FloxerError):
        pile.add(runs[0], reads[:-1] + [reads[-1][:-1]])
    with pytest.raises(F.FloxerError, match="read_index"):
        pile.add(runs[0], reads[:5])
    pile.finish()
    assert len(pile.sites()) == 0 and int(device_counts(pile, lengths).sum()) == 0
    pile.close()
    for run in runs:
        L.flx_run_free(run)
    resident.close()


@gpu
def test_pipeline_refusals(planted):
    chroms, reads, ctx = planted["chroms"], planted["reads"], planted["ctx"]
    lengths = [len(c) for c in chroms]
    L = capi.lib()
    p = F.params(error_probability=planted["rate"])
    raw = {mapq: raw_run(ctx, p, reads, output=F.output_options(mapq=mapq)) for mapq in (False, True)}
    result = F.aligner(ctx, p, output=F.output_options(mapq=True)).align_reads(reads)
    for min_mapq in (0, 2):
        o = R.options(min_mapq=min_mapq)
        pile = F.pileup(ctx, R.c_options(o))
        if min_mapq:                                                      # a run made without mapq holds no mapping quality: refused
            with pytest.raises(F.FloxerError, match="mapq"):
                pile.add(raw[False], reads)
        else:
            pile.add(raw[False], reads)
        pile.add(raw[True], reads)
        pile.finish()
        want = R.counts(lengths, result.raw, result.cigars, reads, o)
        same(pile, lengths, want * (1 if min_mapq else 2), o)
        pile.close()
    for run in raw.values():
        L.flx_run_free(run)
    plain = F.aligner(ctx, p).align_reads(reads)
    pile = F.pileup(ctx, F.pileup_options(min_mapq=2))
    with pytest.raises(F.FloxerError, match="mapq"):
        pile.add(plain, reads)
    pile.close()
    # a run made without CIGARs has no pileup
    bare = F.aligner(ctx, F.params(error_probability=planted["rate"], without_cigar=True)).align_reads(reads)
    bare_raw = C.c_void_p()
    pool, offs, n = F._pool_and_offsets(reads)
    pw = F.params(error_probability=planted["rate"], without_cigar=True)
    capi.check(L.flx_align_reads(ctx.h, C.byref(pw), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n, C.byref(bare_raw)))
    pile = F.pileup(ctx)
    with pytest.raises(F.FloxerError, match="without_cigar"):
        pile.add(bare, reads)
    with pytest.raises(F.FloxerError, match="without_cigar"):
        pile.add(bare_raw, reads)
    L.flx_run_free(bare_raw)
    pile.add(result, reads)
    pile.finish()
    same(pile, lengths, R.counts(lengths, result.raw, result.cigars, reads, R.options()), R.options())
    pile.close()


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
    assert any(f & 2048 for f in whole.raw["flag"]) and clipped                                   # records with S and flag 2048 are walked
    half = len(reads) // 2
    o = R.options(min_depth=1, min_count=1, min_permille=500)
    want, out = run_against_reference(ctx, lengths, [(whole, reads)], o)
    want2, out2 = run_against_reference(ctx, lengths, [(al.align_reads(reads[:half]), reads[:half]), (al.align_reads(reads[half:]), reads[half:])], o)
    assert (want == want2).all() and out == out2 and want[R.A:R.T + 1].sum() > 0
    ctx.close()


# ------------------------------------------------------------------------------------------------ CLI
def pileup_from_sam(text, names, lengths, o):
    """the rule on the SAM text alone: FLAG, POS, CIGAR and SEQ. This writer keeps floxer's convention (output.cpp:69-72): SEQ is the read
    as given whatever the strand, so the walk orients it by flag bit 16 as it does a read of the batch."""
    rows, reads = [], []
    for line in text.splitlines():
        if line.startswith("@"):
            continue
        f = line.split("\t")
        flag = int(f[1])
        if flag & 4:
            continue
        assert "M" not in f[5] and f[9] != "*"
        ws = [R.word(op, int(ln)) for ln, op in re.findall(r"(\d+)([MIDNSHP=X])", f[5])]
        rows.append((flag, names.index(f[2]), int(f[3]) - 1, int(f[4]), ws))
        reads.append(np.array(["$ACGTN".index(c) for c in f[9]], dtype=np.uint8))
    assert rows
    rec, words = R.records_of(rows)
    return R.counts(lengths, rec, words, reads, o)


def cli_files(sample, tmp_path, tag, *devices):
    from test_md_gpu import letters
    chroms, reads = sample["chroms"], sample["reads"]
    fasta, fastq = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq")
    with open(fasta, "w") as f:
        for i, c in enumerate(chroms):
            f.write(f">chr{i} sample\n" + "\n".join(letters(c[o: o + 80]) for o in range(0, len(c), 80)) + "\n")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    paths = {k: str(tmp_path / f"{tag}.{e}") for k, e in (("sam", "sam"), ("plain", "plain.sam"), ("sites", "sites.tsv"))}
    base = [exe, "--reference", fasta, "--queries", fastq, "--error-probability", str(sample["rate"]), "--threads", "1", "-D", "-N", "1", *devices]
    env = dict(os.environ, FLX_BATCH_READS="64")                          # several batches, dealt to the devices in turn
    for cmd in (base + ["--output", paths["plain"]], base + ["--output", paths["sam"], "--pileup", paths["sites"], "--pileup-min-fraction", "0.3"]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    return {k: open(v, "rb").read() for k, v in paths.items()}


@gpu
def test_cli_pileup_file(sample, tmp_path):
    files = cli_files(sample, tmp_path, "one")
    assert files["sam"] == files["plain"]                                 # the alignment output does not change
    names, lengths = ["chr0", "chr1"], [len(c) for c in sample["chroms"]]
    o = R.options(min_permille=300)
    want = pileup_from_sam(files["sam"].decode(), names, lengths, o)
    sites = planted_variants_found(lengths, want, sample["snvs"], sample["indels"], o)
    rows = [tuple(l.split("\t")) for l in files["sites"].decode().splitlines()]
    exp = [(names[int(s["ref"])], str(int(s["pos"]) + 1), "NACGTN"[int(sample["chroms"][int(s["ref"])][int(s["pos"])])], str(int(s["depth"])),
            *(str(int(x)) for x in s["alt"]), str(int(s["del"])), str(int(s["ins"]))) for s in sites]
    assert rows == exp and len(rows) >= 8


@gpu
def test_cli_pileup_file_on_two_devices(sample, tmp_path):
    if capi.lib().flx_device_count() < 2:
        pytest.skip("one HIP device: nothing to sum across")
    one = cli_files(sample, tmp_path, "one")
    two = cli_files(sample, tmp_path, "two", "--devices", "0,1")
    assert one == two
