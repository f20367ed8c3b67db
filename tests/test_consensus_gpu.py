"""Consensus on the GPU (flx_consensus: pileup_add, consensus_ins_keys, the key sort, consensus_allele_*, consensus_call, consensus_emit;
runs, the Python class and the floxer_consensus tool). Every expected value is the plain-numpy rule of tests/consensus_ref.py on the same
text, records, words and reads; the shapes sit on the kernels' boundaries (64 CIGAR words per pass, the key kernel's grid cap, the
sort's tile, the scan's tile and second level)."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import consensus_ref as R
import coverage_ref
import pileup_ref as P
from test_consensus_host import COLUMNS, column_inputs
from test_pileup_gpu import sample_batch, special_rows

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = R.options(min_depth=1, min_count=1, min_permille=1)               # one record is enough for a change


def results(c, n_refs):
    return [c.letters(r) for r in range(n_refs)], c.changes(), c.alleles()


def device(text, lengths, rec, words, reads, o, adds=1):
    c = F.consensus(text=text, lengths=lengths, options=R.c_options(o))
    try:
        for part in np.array_split(np.arange(len(rec)), adds):
            c.add_records(rec[part], words, reads)
        c.finish()
        return results(c, len(lengths))
    finally:
        c.close()


def same(got, want):
    assert [len(s) for s in got[0]] == [len(s) for s in want[0]]
    bad = [(r, next(i for i in range(len(a)) if a[i] != b[i])) for r, (a, b) in enumerate(zip(got[0], want[0])) if a != b]
    assert not bad, bad[:4]
    assert len(got[2]) == len(want[2]) and got[2].tobytes() == want[2].tobytes(), (got[2][:5], want[2][:5])
    assert len(got[1]) == len(want[1]) and got[1].tobytes() == want[1].tobytes(), (got[1][:5], want[1][:5])
    return got


def measure(text, lengths, rec, words, reads, o, adds=1, times=1):
    return same(device(text, lengths, rec, words, reads, o, adds), R.consensus(text, lengths, rec[: len(rec) // times], words, reads, o, times))


# ------------------------------------------------------------------------------------------------ words and carries
def body_words(rng, n):
    """n words: = runs with X, I and D between them, I words on both sides of every pass boundary (an I may be the last word); the first is an ="""
    ws = [("=" if t % 2 == 0 else "XID"[int(rng.integers(0, 3))], int(rng.integers(1, 10))) for t in range(n)]
    for t in (63, 64, 127, 128):
        if 0 < t < n:
            ws[t] = ("I", ws[t][1])
    return [R.word(op, ln) for op, ln in ws]


@gpu
@pytest.mark.parametrize("n_words", [1, 63, 64, 65, 129])
def test_words_and_carries(n_words):
    rng = np.random.default_rng(n_words)
    lengths = [45_000, 33_000]
    body = body_words(rng, n_words)
    inner = body_words(rng, max(1, n_words - 2))
    clipped = ([R.word("S", 7)] + inner + [R.word("S", 5)]) if n_words >= 3 else inner        # the row carry starts at 7
    rows = [(0, 0, 1011, 0, body), (16, 0, 1011, 0, body), (16, 1, 0, 0, clipped), (0, 1, 5, 0, clipped), (16, 1, 33_000 - R.span(body), 0, body)] + special_rows()
    assert len(body) == n_words and (n_words < 3 or len(clipped) == n_words)
    rec, words, reads = R.records_with_reads(rng, rows)
    for read in reads:
        read[(read == 0) | (read == 5)] = 3                                # letters only: every I word of up to 32 letters behind a column is an allele
    text = R.random_text(rng, sum(lengths))
    _, changes, al = measure(text, lengths, rec, words, reads, ANY)
    if n_words >= 65:
        ops = [int(x) & 15 for x in body]
        assert ops[63] == ops[64] == 1                                     # I words on both sides of a pass boundary: the slot carry
        assert len(al) >= 6 and {R.SUB, R.DEL, R.INS} <= {int(k) for k in changes["kind"]}
    # the special rows: an I behind a leading S at 100 + 0 has no column in front and is void, as is the I that is the first word at 200
    # and the two of 70 letters at 500; the I behind the D at 300 + 13, in front of the trailing S at 400 + 21 and at 0 + 1 are alleles
    mine = {(int(a["pos"]), int(a["length"])) for a in al if int(a["ref"]) == 0 and int(a["pos"]) not in range(1011, 1011 + R.span(body))}
    assert mine == {(313, 2), (421, 4), (1, 1)}, mine
    same(device(text, lengths, rec, words, reads, R.options(), adds=3), R.consensus(text, lengths, rec, words, reads, R.options()))


# ------------------------------------------------------------------------------------------------ alleles
@gpu
def test_alleles():
    w = R.word
    rng = np.random.default_rng(12)
    lengths = [200, 50]
    rows, reads = [], []

    def add(flag, ref, pos, ws, read, copies=1):
        for _ in range(copies):
            rows.append((flag, ref, pos, 0, ws))
            reads.append(np.array(read, dtype=np.uint8))
    for k, n in enumerate((1, 2, 31, 32, 33)):                            # the lengths round the key's 32 letters, two records each
        add(0, 0, 10 * k, [w("=", 5), w("I", n), w("=", 4)], [1] * 5 + [int(x) for x in rng.integers(1, 5, size=n)] + [2] * 4, copies=2)
    add(0, 0, 60, [w("=", 2), w("I", 3), w("=", 2)], [1, 1, 2, 5, 2, 1, 1], copies=2)      # a letter of rank 5, and of rank 0, inside an I: void
    add(0, 0, 70, [w("=", 2), w("I", 3), w("=", 2)], [1, 1, 0, 3, 2, 1, 1], copies=2)
    fw = [1, 2, 3, 4, 4, 1, 2, 2, 3]                                      # one read forward, and its reverse complement under flag 16: one allele
    add(0, 0, 100, [w("=", 3), w("I", 3), w("=", 3)], fw)
    add(16, 0, 100, [w("=", 3), w("I", 3), w("=", 3)], P.COMPLEMENT[np.array(fw, dtype=np.uint8)[::-1]])
    for ins in ([4, 1], [2, 3], [4, 1], [2, 3]):                          # two alleles with equal counts at one anchor: C G is the smaller key
        add(0, 0, 120, [w("=", 1), w("I", 2), w("=", 1)], [1] + ins + [1])
    for k in range(3):                                                    # three anchors on consecutive positions
        add(0, 0, 140 + k, [w("=", 1), w("I", 2), w("=", 3)], [1, 1 + k, 4, 1, 1, 1], copies=2)
    add(0, 0, 197, [w("=", 3), w("I", 2)], [1, 1, 1, 3, 3], copies=2)      # an anchor on a sequence's last position
    add(0, 1, 0, [w("=", 4)], [1, 1, 1, 1], copies=2)
    rec, words = R.records_of(rows)
    text = rng.integers(1, 5, size=sum(lengths)).astype(np.uint8)
    o = R.options(min_depth=1, min_count=2, min_permille=1)
    letters, changes, al = measure(text, lengths, rec, words, reads, o)
    got = {(int(a["ref"]), int(a["pos"])): (int(a["length"]), int(a["count"])) for a in al if int(a["pos"]) != 120}
    assert got == {(0, 4): (1, 2), (0, 14): (2, 2), (0, 24): (31, 2), (0, 34): (32, 2), (0, 102): (3, 2), (0, 140): (2, 2), (0, 141): (2, 2), (0, 142): (2, 2), (0, 199): (2, 2)}
    at_120 = [(F.consensus_letters_of(a["letters"], a["length"]), int(a["count"])) for a in al if int(a["pos"]) == 120]
    assert at_120 == [("CG", 2), ("TA", 2)]
    ins = {int(c["pos"]): F.consensus_letters_of(c["letters"], c["length"]) for c in changes if int(c["kind"]) == R.INS and int(c["ref"]) == 0}
    assert ins[120] == "CG" and ins[102] == "TTA" and ins[140] == "AT" and ins[141] == "CT" and ins[142] == "GT" and ins[199] == "GG" and 44 not in ins
    assert all(int(c["ref"]) == 0 for c in changes) and len(letters[1]) == 50 and letters[0].endswith("GG")
    assert len(letters[0]) == 200 + sum(len(s) for s in ins.values())


# ------------------------------------------------------------------------------------------------ the call
@gpu
@pytest.mark.parametrize("case", COLUMNS, ids=[c[0] for c in COLUMNS])
def test_the_call_column_by_column(case):
    _, rank, planes, o, ins, letters, rows = case
    text, rec, words, reads = column_inputs(rank, planes, ins)
    got = same(device(text, [3], rec, words, reads, o), R.consensus(text, [3], rec, words, reads, o))
    assert got[0][0][1:-1] == letters
    mine = got[1][got[1]["pos"] == 1]
    assert [(int(c["kind"]), int(c["alt_rank"]), int(c["count"]), int(c["cov"])) for c in mine] == rows


@gpu
def test_a_sequence_deleted_in_full():
    lengths = [4, 3, 5]
    rec, words = R.records_of([(0, 1, 0, 0, [R.word("D", 3)])] * 3 + [(0, 0, 0, 0, [R.word("=", 4)])] * 3)
    reads = [np.zeros(0, dtype=np.uint8)] * 3 + [np.ones(4, dtype=np.uint8)] * 3
    text = np.array([1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4], dtype=np.uint8)
    letters, changes, _ = measure(text, lengths, rec, words, reads, R.options())
    assert letters == ["ACGT", "", "TACGT"]                               # (the third sequence is not covered and keeps its letters)
    assert [(int(c["ref"]), int(c["pos"]), int(c["kind"]), int(c["count"])) for c in changes] == [(1, 0, R.DEL, 3), (1, 1, R.DEL, 3), (1, 2, R.DEL, 3)]


# ------------------------------------------------------------------------------------------------ contention, the grid cap
@gpu
def test_contention_on_one_column_and_one_anchor():
    lengths = [300, 1000]
    n = 20_000
    rec = np.zeros(n, dtype=R.REC)
    rec["ref"], rec["pos"], rec["coff"], rec["clen"] = 1, 400, 1, 3       # every record refers to the same three words and the same read
    words = np.array([R.word("=", 9), R.word("=", 60), R.word("I", 3), R.word("X", 1), R.word("=", 39)], dtype=np.uint32)
    read = np.full(64, 2, dtype=np.uint8)
    read[63] = 3
    text = np.full(sum(lengths), 1, dtype=np.uint8)
    letters, changes, al = measure(text, lengths, rec, words, [read], R.options(), times=n)      # (the counts are sums over the records)
    assert [(int(a["ref"]), int(a["pos"]), int(a["length"]), int(a["count"])) for a in al] == [(1, 459, 3, n)]
    assert [(int(c["pos"]), int(c["kind"]), int(c["count"]), int(c["cov"])) for c in changes] == [(459, R.INS, n, n), (460, R.SUB, n, n)]
    assert letters[1][458:465] == "AACCCGA"


@gpu
def test_past_the_grid_cap():
    cap, waves, _ = F.consensus_geometry()
    n = cap * waves + 1                                                   # one record more than a full grid of waves: a wave strides on to a second job
    rec = np.zeros(n, dtype=R.REC)
    rec["ref"], rec["pos"], rec["coff"], rec["clen"] = 0, 7, 0, 3
    words = np.array([R.word("=", 3), R.word("I", 1), R.word("=", 1)], dtype=np.uint32)
    read = np.array([1, 1, 1, 4, 1], dtype=np.uint8)
    text = np.full(64, 1, dtype=np.uint8)
    letters, changes, al = measure(text, [64], rec, words, [read], R.options(), times=n)
    assert [(int(a["pos"]), int(a["count"])) for a in al] == [(9, n)] and len(changes) == 1 and letters[0] == "A" * 10 + "T" + "A" * 54


# ------------------------------------------------------------------------------------------------ sort and scan geometry
@gpu
@pytest.mark.parametrize("n_keys", [0, 1, 2047, 2048, 2049])
def test_key_counts_round_the_sort_tile(n_keys):
    lengths = [5000]
    # (records i and i + 1500 yield the same key: runs of one and of two keys)
    rows = [(0, 0, (i % 500) * 7, 0, [R.word("=", 2), R.word("I", 1 + i % 3)]) for i in range(n_keys)] + [(0, 0, 4500, 0, [R.word("X", 2)])]
    rec, words = R.records_of(rows)
    reads = [np.array([1, 1] + [1 + (i % 3 + k) % 4 for k in range(1 + i % 3)], dtype=np.uint8) for i in range(n_keys)] + [np.array([2, 3], dtype=np.uint8)]
    text = np.full(5000, 1, dtype=np.uint8)
    _, changes, al = measure(text, lengths, rec, words, reads, ANY)
    assert int(al["count"].sum()) == n_keys and int((changes["kind"] == R.SUB).sum()) == 2


def geometry_totals():
    t, b = F.coverage_geometry()
    return [1, 64, t - 1, t, t + 1, 2 * t + 1, t * b + 1]


@gpu
@pytest.mark.parametrize("which", range(7))
def test_scan_and_call_geometry(which):
    """a text of A: one X column (C, G or T) per tile, on the first and on the last position, and a two-letter insertion behind every
    tile's last position. Up to two tiles and one position everything is compared with the reference; at the largest total the changes,
    the lengths and stretches of letters round the tile and second-level boundaries against the closed form."""
    t, b = F.coverage_geometry()
    total = geometry_totals()[which]
    assert t * b + 1 <= 1 << 28
    tiles = -(-total // t)
    xs = {min(k * t + (k * 7) % (t - 1), total - 1): 2 + k % 3 for k in range(tiles)}
    xs.update({0: 3, total - 1: 2})
    anchors = sorted({min((k + 1) * t - 1, total - 1) for k in range(tiles)} - set(xs))      # (an X column and the = of an insertion's record would tie)
    rows = [(0, 0, p, 0, [R.word("X", 1)]) for p in sorted(xs)] + [(0, 0, p, 0, [R.word("=", 1), R.word("I", 2)]) for p in anchors]
    rec, words = R.records_of(rows)
    reads = [np.array([xs[p]], dtype=np.uint8) for p in sorted(xs)] + [np.array([1, 2, 3], dtype=np.uint8)] * len(anchors)
    text = np.full(total, 1, dtype=np.uint8)
    if total <= 2 * t + 1:
        measure(text, [total], rec, words, reads, ANY)
        return
    c = F.consensus(text=text, lengths=[total], options=R.c_options(ANY))
    c.add_records(rec, words, reads)
    c.finish()
    letters, changes, al = c.letters(0), c.changes(), c.alleles()
    c.close()
    exp = np.zeros(len(xs) + len(anchors), dtype=F.CHANGE_DTYPE)
    for i, p in enumerate(sorted(set(xs) | set(anchors))):
        exp[i] = (0, p, R.SUB, 1, xs[p], 1, 1, 1, 0) if p in xs else (0, p, R.INS, 1, 0, 2, 1, 1, R.pack([2, 3]))
    assert len(changes) == len(exp) and changes.tobytes() == exp.tobytes()
    assert al["pos"].tolist() == anchors and (al["count"] == 1).all() and len(letters) == total + 2 * len(anchors)
    before = np.array(anchors, dtype=np.int64)
    behind = set(anchors)
    for a in sorted({0, t - 40, 2 * t - 40, t * (b - 1) - 40, total - 60, t * b - 40}):      # stretches: the start, tile boundaries, the second level, the end
        z = min(total, a + 80)
        want = "".join(("NACGT"[xs[p]] if p in xs else "A") + ("CG" if p in behind else "") for p in range(a, z))
        at = a + 2 * int(np.searchsorted(before, a))
        assert letters[at: at + len(want)] == want, a


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
            rows.append((0, r, 0, 0, [w("D", n)]))                         # a sequence deleted in full between its neighbours
    rec, words, reads = R.records_with_reads(rng, rows)
    for read in reads:
        read[(read == 0) | (read == 5)] = 2
    text = R.random_text(rng, sum(lengths))
    letters, changes, al = measure(text, lengths, rec, words, reads, ANY)
    refs = changes["ref"].tolist()
    assert refs == sorted(refs) and len(set(refs)) > 500 and refs[0] == 0 and refs[-1] == last
    assert all(int(c["pos"]) < lengths[int(c["ref"])] for c in changes) and all(int(a["pos"]) < lengths[int(a["ref"])] for a in al)
    assert (0, t - 1) in {(int(a["ref"]), int(a["pos"])) for a in al} and "" in letters and len(letters[0]) == t + 2
    measure(text, lengths, rec, words, reads, R.options(min_depth=1, min_count=1, min_permille=1000, mask_low_depth=True), adds=4)


# ------------------------------------------------------------------------------------------------ lifetime, refusals, threads
@gpu
def test_lifetime_and_refusals():
    L = capi.lib()
    lengths = [700, 300]
    rng = np.random.default_rng(1)
    text = R.random_text(rng, 1000)
    rec, words, reads = R.records_with_reads(rng, [(0, 0, 10, 0, [R.word("=", 100), R.word("X", 3)]), (16, 1, 0, 0, [R.word("X", 300)]),
                                                   (0, 0, 600, 0, [R.word("=", 50), R.word("I", 2), R.word("D", 50)])])
    reads[2][50:52] = [2, 4]
    c = F.consensus(text=text, lengths=lengths, options=R.c_options(ANY))
    c.add_records(rec, words, reads)
    # one bad record last in a batch of good ones: refused, the sums stay
    for bad, extra in (([(0, 0, 650, 0, [R.word("=", 51)])], 0), ([(0, 1, 0, 0, [])], 0), ([(0, 2, 0, 0, [R.word("=", 1)])], 0), ([(0, 0, 0, 0, [R.word("M", 5)])], 0),
                       ([(0, 0, 0, 0, [R.word("=", 5)])], 1), ([(0, 0, 0, 0, [R.word("=", 5)])], -1), ([(0, 0, 0, 0, [R.word("S", 5), R.word("I", 1)])], 0)):
        rec2, words2, reads2 = R.records_with_reads(rng, [(0, 0, 0, 0, [R.word("=", 3), R.word("I", 2), R.word("X", 697)])] * 3 + bad)
        if extra:
            reads2[-1] = np.ones(5 + extra, dtype=np.uint8)
        with pytest.raises(F.FloxerError):
            c.add_records(rec2, words2, reads2)
    rec2["read"][-1] = len(reads2)
    with pytest.raises(F.FloxerError, match="read_index"):
        c.add_records(rec2, words2, reads2)
    # the copy calls work only behind finish
    for call in (lambda: c.letters(0), c.changes, c.alleles):
        with pytest.raises(F.FloxerError, match="flx_consensus_finish"):
            call()
    assert L.flx_consensus_num_changes(c.h) == 0 and L.flx_consensus_num_letters(c.h, 0) == 0 and L.flx_consensus_num_alleles(c.h) == 0
    c.finish()
    want = R.consensus(text, lengths, rec, words, reads, ANY)
    got = same(results(c, 2), want)
    assert len(got[2]) == 1 and len(got[1]) > 200 and len(got[0][0]) == 700 + 2 - 50
    # final: add and finish are refused behind finish
    for call in (lambda: c.add_records(rec, words, reads), lambda: c.add_records(rec[:0], words, reads), c.finish):
        with pytest.raises(F.FloxerError, match="finished"):
            call()
    same(results(c, 2), want)
    # a capacity one too small
    n = L.flx_consensus_num_changes(c.h)
    out = np.zeros(n, dtype=F.CHANGE_DTYPE)
    assert L.flx_consensus_copy_changes(c.h, out.ctypes.data_as(C.POINTER(capi.ConsensusChange)), n - 1) == -3 and str(n) in L.flx_last_error().decode()
    assert L.flx_consensus_copy_changes(c.h, out.ctypes.data_as(C.POINTER(capi.ConsensusChange)), n) == 0 and out.tobytes() == want[1].tobytes()
    al = np.zeros(1, dtype=F.ALLELE_DTYPE)
    assert L.flx_consensus_copy_alleles(c.h, al.ctypes.data_as(C.POINTER(capi.ConsensusAllele)), 0) == -3 and "1 alleles" in L.flx_last_error().decode()
    buf = np.zeros(652, dtype=np.uint8)
    assert L.flx_consensus_copy_letters(c.h, 0, buf.ctypes.data_as(C.c_char_p), 651) == -3 and "652" in L.flx_last_error().decode()
    assert L.flx_consensus_copy_letters(c.h, 0, buf.ctypes.data_as(C.c_char_p), 652) == 0 and buf.tobytes().decode() == want[0][0]
    assert L.flx_consensus_copy_letters(c.h, 2, buf.ctypes.data_as(C.c_char_p), 652) == -1
    c.close()
    # bad options, lengths and texts
    bad = capi.ConsensusOptions()
    bad.reserved[0] = 1
    for make in (lambda: F.consensus(text=text, lengths=lengths, options=bad), lambda: F.consensus(text=text, lengths=lengths, options=F.consensus_options(min_permille=1001)),
                 lambda: F.consensus(text=text, lengths=[700, 301]), lambda: F.consensus(text=text[:0], lengths=[]), lambda: F.consensus(text=np.full(1000, 6, dtype=np.uint8), lengths=lengths),
                 lambda: F.consensus(text=text, lengths=lengths, device=-1), lambda: F.consensus()):
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
    o = R.options(count_secondary=True, min_depth=2, min_count=2, min_permille=100)
    want = R.consensus(text, lengths, rec, words, reads, o)
    assert len(want[2]) > 100 and int(want[2]["count"].max()) > 1 and {R.SUB, R.DEL, R.INS} <= {int(k) for k in want[1]["kind"]}
    same(device(text, lengths, rec, words, reads, o), want)
    c = F.consensus(text=text, lengths=lengths, options=R.c_options(o))
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
    same(results(c, len(lengths)), want)
    c.close()


# ------------------------------------------------------------------------------------------------ pipeline
# Seed 29 (test_pileup_gpu.SAMPLE_SEED) was checked on the CPU oracle's records of this batch: every record of the oracle's run at 4 %
# errors, cut down to one alignment per read by the host form of the output options (duplicates dropped, the smallest NM first) and
# left-aligned by the host form of the gap options, then consensus_ref under the default thresholds. That run showed: all six planted
# SNVs as SUB rows with the planted letter; the 3-base deletion as three DEL rows on 11 000 .. 11 002 of sequence 0; the 2-base insertion
# as one INS row of A G behind position 12 499 of sequence 1; and no other change at all. The cap below allows none. That is a property
# of the alignments, not of the kernels.
OTHER_CHANGES_ALLOWED = 0


def planted_changes_found(changes, snvs):
    rows = {(int(c["ref"]), int(c["pos"]), int(c["kind"])): c for c in changes}
    for ref, pos, rank in snvs:
        c = rows.pop((ref, pos, R.SUB), None)
        assert c is not None and int(c["alt_rank"]) == rank, (ref, pos)
    for pos in (11_000, 11_001, 11_002):
        assert rows.pop((0, pos, R.DEL), None) is not None, pos
    c = rows.pop((1, 12_499, R.INS), None)
    assert c is not None and F.consensus_letters_of(c["letters"], c["length"]) == "AG"
    assert len(rows) <= OTHER_CHANGES_ALLOWED, sorted(rows)


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
    """consensus.add of every (run, reads) against the reference on the runs' own records, words and reads, joined"""
    chroms = sample["chroms"]
    lengths = [len(c) for c in chroms]
    c = F.consensus(sample["ctx"], R.c_options(o))
    parts, all_reads = [], []
    for run, reads in runs:
        c.add(run, reads)
        raw = run.raw.copy()
        raw["read"] += len(all_reads)
        parts.append((raw, run.cigars))
        all_reads += list(reads)
    c.finish()
    got = results(c, len(lengths))
    c.close()
    rec, words = coverage_ref.joined(parts)
    return same(got, R.consensus(np.concatenate(chroms), lengths, rec, words, all_reads, o))


@gpu
@pytest.mark.parametrize("realign", [False, True])
def test_pipeline(sample, realign):
    reads = sample["reads"]
    al = aligner_of(sample, **(dict(realign=F.realign_options()) if realign else {}))
    whole = al.align_reads(reads)
    half = len(reads) // 2
    o = R.options()
    one = run_against_reference(sample, [(whole, reads)], o)
    two = run_against_reference(sample, [(al.align_reads(reads[:half]), reads[:half]), (al.align_reads(reads[half:]), reads[half:])], o)
    assert one[0] == two[0] and one[1].tobytes() == two[1].tobytes() and one[2].tobytes() == two[2].tobytes()
    assert {0, 16} <= {int(f) & 16 for f in whole.raw["flag"]} and len(one[2]) > 10
    if not realign:
        planted_changes_found(one[1], sample["snvs"])


@gpu
def test_pipeline_refusals(sample):
    reads = sample["reads"][:40]
    ctx = sample["ctx"]
    plain = aligner_of(sample).align_reads(reads)
    c = F.consensus(ctx, F.consensus_options(min_mapq=2))
    with pytest.raises(F.FloxerError, match="mapq"):                     # a run made without mapq holds no mapping quality
        c.add(plain, reads)
    L = capi.lib()
    pool, offs, n = F._pool_and_offsets(reads)
    raw = C.c_void_p()
    capi.check(L.flx_align_reads(ctx.h, C.byref(F.params(error_probability=sample["rate"])), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n, C.byref(raw)))
    with pytest.raises(F.FloxerError, match="mapq"):
        c.add(raw, reads)
    L.flx_run_free(raw)
    with pytest.raises(F.FloxerError, match="consensus"):                # the context waits for its consensus objects
        capi.check(L.flx_ctx_destroy(ctx.h))
    c.close()
    bare = F.aligner(ctx, F.params(error_probability=sample["rate"], without_cigar=True)).align_reads(reads)
    pw = F.params(error_probability=sample["rate"], without_cigar=True)
    capi.check(L.flx_align_reads(ctx.h, C.byref(pw), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n, C.byref(raw)))
    c = F.consensus(ctx)
    with pytest.raises(F.FloxerError, match="without_cigar"):
        c.add(bare, reads)
    with pytest.raises(F.FloxerError, match="without_cigar"):
        c.add(raw, reads)
    L.flx_run_free(raw)
    c.add(plain, reads)                                                   # refused adds left the object as it was
    c.finish()
    lengths = [len(x) for x in sample["chroms"]]
    same(results(c, 2), R.consensus(np.concatenate(sample["chroms"]), lengths, plain.raw, plain.cigars, reads, R.options()))
    c.close()


# ------------------------------------------------------------------------------------------------ the tool
@gpu
def test_tool_files(sample, tmp_path):
    from test_md_gpu import letters
    chroms, reads = sample["chroms"], sample["reads"]
    work = tmp_path / "work"
    work.mkdir()
    fasta, fastq, out, tsv = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq"), str(work / "consensus.fasta"), str(work / "changes.tsv")
    with open(fasta, "w") as f:
        for i, c in enumerate(chroms):
            f.write(f">chr{i} sample\n" + "\n".join(letters(c[o: o + 80]) for o in range(0, len(c), 80)) + "\n")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
    exe = os.path.join(ROOT, "floxer_amd", "floxer_consensus")
    base = [exe, "--reference", fasta, "--queries", fastq, "--error-probability", str(sample["rate"])]
    env = dict(os.environ, FLX_BATCH_READS="64")                          # several batches
    r = subprocess.run(base + ["--output", out, "--changes", tsv, "--min-fraction", "0.4"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    assert sorted(os.listdir(work)) == ["changes.tsv", "consensus.fasta"] and sorted(os.listdir(tmp_path)) == ["reads.fastq", "ref.fasta", "work"]
    c = F.consensus(sample["ctx"], F.consensus_options(min_permille=400))
    c.add(aligner_of(sample).align_reads(reads), reads)
    c.finish()
    seqs, changes, _ = results(c, 2)
    c.close()
    want_fasta = "".join(f">chr{i}\n" + "".join(s[o: o + 80] + "\n" for o in range(0, len(s), 80)) for i, s in enumerate(seqs))
    alt = lambda x: "NACGT"[int(x["alt_rank"])] if int(x["kind"]) == R.SUB else "-" if int(x["kind"]) == R.DEL else F.consensus_letters_of(x["letters"], x["length"])  # noqa: E731
    want_tsv = "".join(f"chr{int(x['ref'])}\t{int(x['pos']) + 1}\t{F.CONSENSUS_KINDS[int(x['kind'])]}\t{'NACGTN'[int(x['ref_rank'])]}\t{alt(x)}\t{int(x['count'])}\t{int(x['cov'])}\n"
                       for x in changes)
    assert open(out).read() == want_fasta and open(tsv).read() == want_tsv and len(changes) >= 10
    r = subprocess.run(base + ["--output", str(work / "other.bam")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 255 and r.stderr.startswith(b"[CLI PARSER ERROR]\n") and b"[fa,fasta]" in r.stderr and sorted(os.listdir(work)) == ["changes.tsv", "consensus.fasta"]
