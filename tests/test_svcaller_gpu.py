"""Structural-variant calls on the GPU (flx_svcaller): the device object's rows() and spans() against the plain-Python rule of
tests/svcall_ref.py, which asks every span by brute force, byte for byte: the words and lanes of svcall_spans, both launches past their
grid caps, the sort's tile boundaries, the windows of svcall_count at their edges, growth, adding threads, absorb, the device against the
host form and flx_svcall_host, the calls behind finish, and end to end through the library and through the tool floxer_sv."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import sv_ref as S
import svcall_ref as R
from test_svcaller_host import cuts, dele, max_span_of, random_case, span_array, spans_as_records
from test_sv_gpu import DEL_AT, E2E_LEN, E2E_RATE, _revcomp, e2e_aligner, e2e_data

gpu = pytest.mark.gpu
W = S.word
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1000, 3000, 800, 30_000]
GEO = F.svcaller_geometry


def ins(ref, pos, q, support=1):
    return (R.INS, 0, 0, support, ref, ref, pos, pos, q, q, q)


def device_tables(rec, words, clusters, o=None, lengths=LENGTHS, ranges=None, device=0, **kw):
    """(rows, spans, max_span) of an object fed rec[a:b] for every (a, b) of ranges (all records in one add without them)"""
    s = F.svcaller(options=R.c_options(o or R.options()), lengths=lengths, device=device, **kw)
    try:
        for a, b in ranges or [(0, len(rec))]:
            s.add_records(rec[a:b], words)
        s.finish(S.cluster_array(R.cluster_tuples(clusters)))
        return s.rows(), s.spans(), s.max_span()
    finally:
        s.close()


def wanted(rec, words, clusters, o=None, lengths=LENGTHS):
    o = o or R.options()
    spans = R.spans(rec, words, o)
    return R.expected(rec, words, clusters, lengths, o), span_array(spans), max_span_of(spans)


def same(got, want, what=""):
    rows, spans, max_span = got
    assert len(rows) == len(want[0]) and rows.tobytes() == want[0].tobytes(), (what, R.row_tuples(rows)[:3], R.row_tuples(want[0])[:3])
    assert spans.tobytes() == want[1].tobytes() and max_span == want[2], (what, len(spans), len(want[1]), max_span, want[2])


def check(rec, words, clusters, o=None, lengths=LENGTHS, **kw):
    want = wanted(rec, words, clusters, o, lengths)
    same(device_tables(rec, words, clusters, o, lengths, **kw), want)
    return R.row_tuples(want[0])


# ------------------------------------------------------------------------------------------------ 1: words and lanes
def words_of(n_words, shift):
    """exactly n_words words with every op among them (from three words on: S at both ends); the lengths differ from word to word, so
    that a lane that takes another lane's word, or an S or I word that counts, changes the span"""
    if n_words < 3:
        return [W("=X"[(t + shift) % 2], 5 + t + shift) for t in range(n_words)]
    return [W("S", 7 + shift)] + [W("=XID"[(t + shift) % 4], 1 + (t * 7 + shift) % 11) for t in range(n_words - 2)] + [W("S", 9)]


@gpu
def test_words_and_lanes():
    rows = []
    for k, n_words in enumerate((1, 63, 64, 65, 129, 2, 3, 128, 200)):
        for j, flag in enumerate((0, 16, 256, 272)):
            rows.append((flag, 3, 100 + 37 * k + j, len(rows), 10 * j + k, words_of(n_words, j)))
    rows.insert(5, (4, -1, 0, 99, 0, []))
    rows.append((4, -1, 0, 100, 0, []))
    rec, words = S.records_of(rows)
    clusters = [dele(3, 120 + 40 * k, 10 + k, support=k % 3) for k in range(12)] + [ins(3, 150, 60), dele(3, 0, 5), (R.BND, 0, 1, 2, 0, 3, 5, 5, 7, 7, 7)]
    lens = {(r[2], r[2] + sum(w >> 4 for w in r[5] if w & 15 in (7, 8, 2))) for r in rows if r[0] != 4}
    assert len({b - a for a, b in lens}) >= 9                            # the spans differ
    for o in (R.options(flank=3), R.options(flank=3, count_secondary=True), R.options(flank=3, min_mapq=12), R.options(flank=3, count_secondary=True, min_mapq=31)):
        got = check(rec, words, clusters, o)
        assert any(r[10] > 0 for r in got)
    assert len(wanted(rec, words, clusters, R.options(count_secondary=True))[1]) == 36 and len(wanted(rec, words, clusters, R.options(min_mapq=12))[1]) < 18


# ------------------------------------------------------------------------------------------------ 2, 5: past the grid caps
def many_single_word_records(n, tail):
    """n records of one = word of 100 columns on sequence 3 at positions i % 500, the last `tail` ones longer and elsewhere"""
    rec = np.zeros(n, dtype=S.REC_DTYPE)
    rec["read"], rec["ref"], rec["pos"], rec["coff"], rec["clen"] = np.arange(n), 3, np.arange(n) % 500, np.arange(n), 1
    words = np.full(n, W("=", 100), dtype=np.uint32)
    for k in range(tail):
        rec["pos"][n - 1 - k] = 450
        words[n - 1 - k] = W("=", 150 + 10 * k)
    return rec, words


@gpu
def test_past_the_spans_grid_cap():
    g = GEO()
    n = g["spans_grid_cap"] * g["waves_per_block"] + 3
    rec, words = many_single_word_records(n, 3)
    o = R.options(flank=10)
    clusters = [dele(3, 570, 20, support=1), dele(3, 300, 20, support=2), dele(3, 470, 30)]         # the first (lo' 560, hi' 600) is spanned by the last three records alone
    got = check(rec, words, clusters, o)
    assert got[0][10] == 3 and got[1][10] > 500 and wanted(rec, words, clusters, o)[2] == 170


@gpu
def test_past_the_count_grid_cap():
    g = GEO()
    n = g["count_grid_cap"] * g["waves_per_block"] + 5
    rec, words = many_single_word_records(300, 3)
    clusters = []
    for i in range(n):
        if i % 11 == 0:
            clusters.append((R.BND, 0, 1, 2, 0, 3, 5, 5, 7, 7, 7))
        clusters.append(dele(3, (i * 7) % 640, 1 + i % 30, support=i % 5))
    clusters[-1] = dele(3, 455, 160, support=1)                          # the last row (lo' 450, hi' 620): spanned by the longest record only
    got = check(rec, words, clusters, R.options(flank=5))
    assert len(got) == n and got[-1][10] == 1 and got[-1][0] == len(clusters) - 1 and len({r[10] for r in got}) > 5


# ------------------------------------------------------------------------------------------------ 3: sort boundaries
@gpu
def test_sort_boundaries():
    tile = GEO()["sort_tile"]
    rng = np.random.default_rng(3)
    clusters = [dele(1, 400 + 100 * k, 20, support=k) for k in range(8)] + [ins(0, 500, 70), dele(3, 100, 10)]
    for n in (0, 1, tile - 1, tile, tile + 1):
        rec = np.zeros(n, dtype=S.REC_DTYPE)
        rec["read"], rec["coff"], rec["clen"] = np.arange(n), np.arange(n), 1
        rec["ref"] = rng.integers(0, 2, n)
        rec["pos"] = np.sort(rng.integers(0, 700, n))[::-1]              # in descending order: every key moves
        words = (rng.integers(1, 300, n).astype(np.uint32) << 4 | 7).astype(np.uint32)
        got = check(rec, words, clusters, R.options(flank=20))
        assert n < 2 or any(r[10] > 0 for r in got)
    # many equal keys, and a few others among them
    rec, words = spans_as_records([(1, 300, 900)] * 1500 + [(1, 301, 900), (0, 300, 900)] + [(1, 300, 900)] * 1500 + [(1, 300, 899), (1, 299, 2000)])
    got = check(rec, words, [dele(1, 350, 500, support=3), dele(1, 349, 501)], R.options(flank=50))
    assert [r[10] for r in got] == [3001, 1]


# ------------------------------------------------------------------------------------------------ 4: the window
@gpu
def test_the_window():
    o = R.options(flank=10)
    lengths = [5000, 1000, 1000, 700]
    cl = [dele(1, 100, 20)]                                              # lo' = 90, hi' = 130
    # windows of 0, 1, 63, 64, 65 and 200 candidates: with max_span 100 the candidates start in [30, 90]; every third one stops one
    # column short of hi'
    for k in (0, 1, 63, 64, 65, 200):
        spans = [(1, 29, 129), (1, 0, 29), (1, 91, 191), (1, 91, 130), (2, 50, 150), (0, 50, 150)]      # none of these is in the window or counts
        spans += [(1, 30 + (i * 7) % 61, 129 if i % 3 == 2 else 130) for i in range(k)]
        rec, words = spans_as_records(spans)
        got = check(rec, words, cl, o, lengths)
        assert got[0][10] == k - k // 3 and wanted(rec, words, cl, o, lengths)[2] == 100
    # the bounds at their edges (tests/test_svcall_host.py's cases, on the device)
    for spans, want in (([(1, 90, 130)], 1), ([(1, 91, 130)], 0), ([(1, 90, 129)], 0), ([(1, 89, 131), (1, 90, 130), (1, 91, 131), (1, 0, 129)], 2),
                        ([(0, 0, 5000), (1, 90, 130), (1, 0, 1000)], 2),              # the record that sets max_span lies on another sequence
                        ([(0, 90, 130), (2, 90, 130)], 0), ([(0, 90, 130), (1, 90, 130), (2, 90, 130), (1, 90, 130)], 2),
                        ([(1, 0, 40), (1, 90, 130)], 1), ([(1, 0, 39), (1, 95, 134)], 0), ([], 0)):
        rec, words = spans_as_records(spans)
        assert [r[10] for r in check(rec, words, cl, o, lengths)] == [want], spans
    # hi' < max_span: the window starts at the sequence's first position
    rec, words = spans_as_records([(0, 0, 4000), (1, 0, 200), (1, 0, 129), (1, 50, 900), (1, 91, 1000)])
    assert [r[10] for r in check(rec, words, cl, o, lengths)] == [2]
    # a cluster at position 0 and clusters that end on their sequence's end: lo' clamps at 0 and hi' at the end
    rec, words = spans_as_records([(1, 0, 25), (1, 1, 25), (1, 0, 24), (1, 989, 1000), (1, 990, 1000), (1, 970, 1000), (1, 970, 999)])
    assert [r[10] for r in check(rec, words, [dele(1, 0, 15, support=0), ins(1, 999, 60, support=0), dele(1, 980, 20, support=0)], o, lengths)] == [1, 2, 1]
    # a sequence without spans, among sequences with spans; BND clusters interleaved, so that a row's index is not its cluster's
    bnd = (R.BND, 1, 0, 4, 0, 3, 7, 9, 1, 2, 3)
    rec, words = spans_as_records([(0, 0, 5000), (1, 0, 1000), (2, 0, 1000)])
    mixed = [bnd, dele(3, 100, 20), bnd, bnd, dele(1, 100, 20, support=0), ins(2, 5, 60), bnd, dele(0, 4000, 1000), bnd]
    got = check(rec, words, mixed, o, lengths)
    assert [(r[0], r[10]) for r in got] == [(1, 0), (4, 1), (5, 1), (7, 1)]
    # an object without spans at all; no clusters; only BND clusters
    none = np.zeros(0, dtype=S.REC_DTYPE), np.zeros(0, dtype=np.uint32)
    assert [r[10] for r in check(*none, mixed, o, lengths)] == [0, 0, 0, 0]
    assert check(rec, words, [], o, lengths) == [] and check(rec, words, [bnd, bnd], o, lengths) == [] and check(*none, [], o, lengths) == []


# ------------------------------------------------------------------------------------------------ 6, 7: growth, threads, absorb
@gpu
def test_growth_and_adding_threads():
    rng = np.random.default_rng(6)
    rec, words, clusters, o = random_case(rng, 1)
    want = wanted(rec, words, clusters, o)
    assert len(want[1]) > 200
    same(device_tables(rec, words, clusters, o), want, "one add")
    same(device_tables(rec, words, clusters, o, ranges=cuts(rng, len(rec), 7), initial_capacity=8), want, "seven adds from a capacity of 8")
    s = F.svcaller(options=R.c_options(o), lengths=LENGTHS, initial_capacity=8)
    errors = []

    def add(a, b):
        try:
            s.add_records(rec[a:b], words)
        except Exception as e:                                           # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=add, args=ab) for ab in cuts(rng, len(rec), 4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    s.finish(S.cluster_array(R.cluster_tuples(clusters)))
    same((s.rows(), s.spans(), s.max_span()), want, "four threads")
    s.close()


@gpu
def test_absorb_with_the_longest_record_in_from():
    rng = np.random.default_rng(7)
    rec, words, clusters, o = random_case(rng, 2)
    long_rec, long_words = S.records_of([(0, 3, 100, 0, 60, [W("=", 20_000)])])
    long_rec["coff"] = len(words)
    rec_all, words_all = np.concatenate([rec, long_rec]), np.concatenate([words, long_words])
    clusters = clusters + [dele(3, 5000, 100, support=0)]
    want = wanted(rec_all, words_all, clusters, o)
    assert want[2] == 20_000 and R.row_tuples(want[0])[-1][10] >= 1
    a, b = F.svcaller(options=R.c_options(o), lengths=LENGTHS, initial_capacity=8), F.svcaller(options=R.c_options(o), lengths=LENGTHS)
    half = len(rec) // 2
    a.add_records(rec[:half], words)
    b.add_records(rec[half:], words)
    b.add_records(long_rec, words_all)
    a.absorb(b)
    a.finish(S.cluster_array(R.cluster_tuples(clusters)))
    same((a.rows(), a.spans(), a.max_span()), want, "absorbed")
    b.finish(S.cluster_array(R.cluster_tuples(clusters)))               # `from` is left empty, with max_span 0
    assert len(b.spans()) == 0 and b.max_span() == 0 and b.rows().tobytes() == R.expected(rec[:0], words, clusters, LENGTHS, o).tobytes()
    a.close()
    b.close()
    # `from` is usable after an absorb: what it is fed afterwards is its own
    a, b = F.svcaller(lengths=LENGTHS), F.svcaller(lengths=LENGTHS)
    b.add_records(long_rec, words_all)
    a.absorb(b)
    b.add_records(rec[:50], words)
    b.finish(S.cluster_array(R.cluster_tuples(clusters)))
    same((b.rows(), b.spans(), b.max_span()), wanted(rec[:50], words, clusters), "from, fed again")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 8: device == host form == svcall_host == reference
@gpu
def test_device_equals_host_form_equals_svcall_host_equals_the_reference():
    rng = np.random.default_rng(20261021)
    seen = set()
    for case in range(6):
        rec, words, clusters, o = random_case(rng, case)
        want = wanted(rec, words, clusters, o)
        ranges = cuts(rng, len(rec), 1 + case % 3)
        same(device_tables(rec, words, clusters, o, ranges=ranges), want, ("device", case))
        same(device_tables(rec, words, clusters, o, ranges=ranges, device=-1), want, ("host form", case))
        assert F.svcall_host(LENGTHS, rec, words, S.cluster_array(R.cluster_tuples(clusters)), R.c_options(o)).tobytes() == want[0].tobytes()
        seen |= {(int(r["gt"]), int(r["pass"]), int(r["span_n"]) > 0) for r in want[0]}
    assert {g for g, _, _ in seen} == {0, 1, 2} and {p for _, p, _ in seen} == {0, 1} and {s for _, _, s in seen} == {False, True}


# ------------------------------------------------------------------------------------------------ 9: the lifetime and the refusals
@gpu
def test_lifetime_and_refusals_on_a_device_object():
    L = capi.lib()
    lengths = [100, 50]
    rec, words = spans_as_records([(0, 0, 100), (1, 0, 50), (0, 10, 60)])
    good = [dele(0, 10, 5), dele(1, 40, 10), ins(1, 49, 10, support=3), (R.BND, 1, 0, 1, 0, 1, 1, 1, 9, 2, 1)]
    s, t = F.svcaller(lengths=lengths), F.svcaller(lengths=lengths)
    s.add_records(rec, words)
    assert L.flx_svcaller_num_spans(s.h) == 0 and L.flx_svcaller_num_rows(s.h) == 0 and s.max_span() == 0
    for call, name in ((s.rows, "copy_rows"), (s.spans, "copy_spans")):
        with pytest.raises(F.FloxerError, match=f"flx_svcaller_{name}: call flx_svcaller_finish first"):
            call()
    # a refused add and a refused finish leave the object as it was
    bad, bad_words = S.records_of([(0, 0, 0, 0, 0, [W("=", 100)]), (0, 0, 60, 0, 0, [W("=", 41)])])
    with pytest.raises(F.FloxerError, match="flx_svcaller_add_records: record 1 ends behind its sequence"):
        s.add_records(bad, bad_words)
    for wrong, message in ((dele(1, 41, 10), "ends behind its sequence"), (ins(1, 50, 10), "at or behind its sequence's end"), ((3, 0, 0, 1, 0, 0, 1, 1, 1, 1, 1), "type above 2"),
                           (dele(2, 1, 1), "outside the lengths")):
        with pytest.raises(F.FloxerError, match="flx_svcaller_finish: cluster 1 .*" + message):
            s.finish(S.cluster_array([good[0], wrong]))
    # absorb: itself, other lengths, other options, a host form
    u, v, h = F.svcaller(lengths=[100, 51]), F.svcaller(lengths=lengths, options=F.svcall_options(flank=51)), F.svcaller(lengths=lengths, device=-1)
    for other, message in ((s, "itself"), (u, "different reference lengths"), (v, "different options"), (h, "a host form and a device object")):
        with pytest.raises(F.FloxerError, match="flx_svcaller_absorb: .*" + message):
            s.absorb(other)
    with pytest.raises(F.FloxerError, match="a host form and a device object"):
        h.absorb(s)
    s.finish(S.cluster_array(good))
    want = wanted(rec, words, good, lengths=lengths)
    same((s.rows(), s.spans(), s.max_span()), want, "behind the refusals")
    # the copy contract on the device: capacity n - 1 writes nothing, capacity n into n + 1 rows leaves the last one alone
    n = len(want[0])
    rowp, spanp = C.POINTER(capi.SvcallRow), C.POINTER(capi.SvcallSpan)
    out = np.full((n + 1) * 72, 0xAB, dtype=np.uint8).view(F.SVCALL_ROW_DTYPE)
    assert L.flx_svcaller_copy_rows(s.h, out.ctypes.data_as(rowp), n - 1) == -3 and f"too small, {n} rows" in L.flx_last_error().decode() and out.tobytes() == b"\xab" * (72 * (n + 1))
    assert L.flx_svcaller_copy_rows(s.h, out.ctypes.data_as(rowp), n) == 0 and out[:n].tobytes() == want[0].tobytes() and out[n:].tobytes() == b"\xab" * 72
    assert L.flx_svcaller_copy_rows(s.h, None, n) == -1 and "null argument" in L.flx_last_error().decode()
    sp = np.full(4, 7, dtype=F.SVCALL_SPAN_DTYPE)
    for a, b in ((0, 4), (2, 1), (4, 4)):
        assert L.flx_svcaller_copy_spans(s.h, a, b, sp.ctypes.data_as(spanp)) == -1 and "a stretch outside the spans" in L.flx_last_error().decode()
    assert (sp["rs"] == 7).all()
    assert L.flx_svcaller_copy_spans(s.h, 1, 3, sp.ctypes.data_as(spanp)) == 0 and sp[:2].tobytes() == want[1][1:3].tobytes() and (sp["rs"][2:] == 7).all()
    assert L.flx_svcaller_copy_spans(s.h, 3, 3, None) == 0 and L.flx_svcaller_copy_spans(s.h, 0, 3, None) == -1
    # behind the finish
    for call in (lambda: s.add_records(rec, words), lambda: s.absorb(t), lambda: t.absorb(s), lambda: s.finish(S.cluster_array(good))):
        with pytest.raises(F.FloxerError, match="finished"):
            call()
    for x in (s, t, u, v, h):
        x.close()


# ------------------------------------------------------------------------------------------------ 10, 11: end to end
OTHERS_AT = (DEL_AT - 1050, DEL_AT - 700, DEL_AT - 350)                  # 1500 columns from each cover [DEL_AT - 300, DEL_AT + 400)
PLANTED = dict(pos_a_min=DEL_AT + 2, pos_a_max=DEL_AT + 2, q_median=80)  # the realigned gap: two columns right of where it was planted (test_sv_gpu's docstring)


@pytest.fixture(scope="module")
def e2e():
    chroms, reads, _, _ = e2e_data()
    more = reads + [(_revcomp(r) if k % 2 else r) for k, r in enumerate(chroms[0][p: p + E2E_LEN].copy() for p in OTHERS_AT)]
    assert all(p <= DEL_AT - 300 and p + E2E_LEN >= DEL_AT + 400 for p in OTHERS_AT)
    ctx = F.context(F.fmindex(chroms))
    yield chroms, reads, more, ctx
    ctx.close()


def library_rows(ctx, run, n_reads, lengths, o=None):
    """the run fed to an sv object and to an svcaller object of the context: (clusters, rows)"""
    s = F.sv(ctx)
    s.add_run(run, [E2E_LEN] * n_reads)
    s.finish()
    cl = s.clusters()
    s.close()
    c = F.svcaller(ctx, R.c_options(o) if o else None)
    c.add(run)
    c.finish(cl)
    rows, spans = c.rows(), c.spans()
    c.close()
    o = o or R.options()
    assert rows.tobytes() == R.expected(run.raw, run.cigars, cl, lengths, o).tobytes() and spans.tobytes() == span_array(R.spans(run.raw, run.cigars, o)).tobytes()
    return cl, rows


def planted_row(rows):
    hit = [r for r in rows if r["type"] == R.DEL and r["ref"] == 0 and all(int(r[k]) == v for k, v in PLANTED.items())]
    assert len(hit) == 1, R.row_tuples(rows)
    return {k: int(hit[0][k]) for k in ("ref_n", "alt_n", "span_n", "gt", "qual", "pass")}


@gpu
def test_end_to_end_through_the_library(e2e):
    chroms, reads, more, ctx = e2e
    lengths = [len(c) for c in chroms]
    run = e2e_aligner(ctx).align_reads(reads)
    _, rows = library_rows(ctx, run, len(reads), lengths)
    assert planted_row(rows) == dict(ref_n=0, alt_n=5, span_n=5, gt=2, qual=4389, **{"pass": 1})
    run2 = e2e_aligner(ctx).align_reads(more)
    cigars = [F.cigar_string(run2.cigars[int(r["coff"]): int(r["coff"]) + int(r["clen"])]) for r in run2.raw if int(r["read"]) >= len(reads)]
    assert cigars == [f"{E2E_LEN}="] * 3                                  # an error-free read maps as one = word and makes no signature
    _, rows2 = library_rows(ctx, run2, len(more), lengths)
    assert planted_row(rows2) == dict(ref_n=3, alt_n=5, span_n=8, gt=1, qual=2378, **{"pass": 1})
    assert 3 * 36 + 5 * 1574 - (8 * 325 + 3000) == 2378
    # with min_mapq the rows follow the reference as well, and a run made without mapq is refused
    _, rows3 = library_rows(ctx, run2, len(more), lengths, R.options(min_mapq=1))
    assert len(rows3) == len(rows2)
    plain = e2e_aligner(ctx, mapq=False).align_reads(reads[:2])
    c = F.svcaller(ctx, F.svcall_options(min_mapq=1))
    with pytest.raises(F.FloxerError, match="min_mapq needs"):
        c.add(plain)
    # the object is counted by its context
    L = capi.lib()
    assert L.flx_ctx_destroy(ctx.h) == -1 and "svcaller object(s) of this context are still alive" in L.flx_last_error().decode()
    c.close()


@gpu
def test_add_run_takes_a_raw_handle_and_refuses_runs_without_mapq_or_cigars(e2e):
    from test_sv_gpu import copied_records, e2e_raw_run
    chroms, reads, more, ctx = e2e
    L = capi.lib()
    lengths = [len(c) for c in chroms]
    raw = {mapq: e2e_raw_run(ctx, more, mapq) for mapq in (False, True)}
    bare = C.c_void_p()
    pool, offs, n = F._pool_and_offsets(reads)
    pw = F.params(error_probability=E2E_RATE, without_cigar=True)
    capi.check(L.flx_align_reads(ctx.h, C.byref(pw), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n, C.byref(bare)))
    try:
        rec, words = copied_records(raw[True])
        cl = [dele(0, DEL_AT + 2, 80, support=5)]
        for o in (R.options(), R.options(min_mapq=1)):
            c = F.svcaller(ctx, R.c_options(o), initial_capacity=8)
            if o["min_mapq"]:
                with pytest.raises(F.FloxerError, match="flx_svcaller_add_run: min_mapq needs a run made with flx_output_options.mapq"):
                    c.add(raw[False])
            with pytest.raises(F.FloxerError, match="min_mapq needs" if o["min_mapq"] else "flx_svcaller_add_run: record .*without_cigar"):
                c.add(bare)
            c.add(raw[True])
            c.finish(S.cluster_array(cl))
            same((c.rows(), c.spans(), c.max_span()), wanted(rec, words, cl, o, lengths), "a raw run")      # the refused runs left nothing behind
            assert o["min_mapq"] or int(c.rows()[0]["span_n"]) == 8
            c.close()
    finally:
        for r in (raw[False], raw[True], bare):
            L.flx_run_free(r)


def vcf_lines(rows, names, chroms, all_rows=False):
    """the tool's lines for the library's rows, from the rule INTEGRATION.md states"""
    out = []
    pos_of = lambda r: max(int(r["pos_a_min"]), 1) if r["type"] == R.DEL else int(r["pos_a_min"]) + 1      # noqa: E731
    for r in sorted(rows, key=lambda r: (int(r["ref"]), pos_of(r), int(r["type"]), int(r["q_median"]))):
        if int(r["gt"]) == 0 and not all_rows:
            continue
        d = r["type"] == R.DEL
        pos, q = pos_of(r), int(r["q_median"])
        info = f"SVTYPE={'DEL' if d else 'INS'};END={int(r['pos_a_max']) + q if d else pos};SVLEN={-q if d else q};CIPOS=0,{int(r['pos_a_max']) - int(r['pos_a_min'])};SUPPORT={int(r['alt_n'])}"
        if r["pos_a_min"] != r["pos_a_max"] or r["q_min"] != r["q_max"]:
            info += ";IMPRECISE"
        sample = f"{('0/0', '0/1', '1/1')[int(r['gt'])]}:{int(r['gq'])}:{int(r['ref_n']) + int(r['alt_n'])}:{int(r['ref_n'])},{int(r['alt_n'])}:{','.join(str(int(x)) for x in r['pl'])}"
        out.append("\t".join([names[int(r["ref"])], str(pos), ".", "$ACGTN"[chroms[int(r["ref"])][pos - 1]], "<DEL>" if d else "<INS>", f"{int(r['qual']) // 100}.{int(r['qual']) % 100:02d}",
                              "PASS" if r["pass"] else "LowQual", info, "GT:GQ:DP:AD:PL", sample]))
    return out


@gpu
def test_end_to_end_through_the_tool(e2e, tmp_path):
    import re
    chroms, reads, more, ctx = e2e
    lengths = [len(c) for c in chroms]
    names = ["chr0", "chr1"]
    letters = lambda r: "".join("$ACGTN"[x] for x in r)                   # noqa: E731
    fasta = str(tmp_path / "ref.fasta")
    with open(fasta, "w") as f:
        for i, c in enumerate(chroms):
            f.write(f">chr{i}\n" + "\n".join(letters(c[o: o + 100]) for o in range(0, len(c), 100)) + "\n")
    tool = os.path.join(ROOT, "floxer_amd", "floxer_sv")

    def run_tool(name, which, *extra):
        fastq, vcf = str(tmp_path / (name + ".fastq")), str(tmp_path / (name + ".vcf"))
        with open(fastq, "w") as f:
            for i, r in enumerate(which):
                f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
        # (--read-error 0.08 derives the library's default costs 36 / 1574 / 325; without it the costs would follow --error-probability)
        r = subprocess.run([tool, "--reference", fasta, "--queries", fastq, "--error-probability", str(E2E_RATE), "--read-error", "0.08", "--output", vcf] + list(extra),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()[-2000:]
        text = open(vcf).read().splitlines()
        head, body = [l for l in text if l.startswith("#")], [l for l in text if not l.startswith("#")]
        # well-formed: the header first, every id that is used is declared, the lines in (sequence, POS) order
        assert text == head + body and head[0] == "##fileformat=VCFv4.2" and head[-1].split("\t") == ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT", "SAMPLE"]
        declared = {kind: set(re.findall(rf"##{kind}=<ID=([^,>]+)", "\n".join(head))) for kind in ("INFO", "FILTER", "ALT", "FORMAT", "contig")}
        for l in body:
            chrom, pos, _, ref_letter, alt, qual, flt, info, fmt, sample = l.split("\t")
            assert chrom in declared["contig"] and alt[1:-1] in declared["ALT"] and flt in declared["FILTER"] and re.fullmatch(r"\d+\.\d\d", qual) and ref_letter in "ACGTN"
            assert {kv.split("=")[0] for kv in info.split(";")} <= declared["INFO"] and set(fmt.split(":")) <= declared["FORMAT"] and len(sample.split(":")) == 5
        keys = [(names.index(l.split("\t")[0]), int(l.split("\t")[1])) for l in body]
        assert keys == sorted(keys)
        return body

    # what the library gives for the tool's alignment options: no partial alignments, the CIGARs realigned
    tool_aligner = F.aligner(ctx, F.params(error_probability=E2E_RATE), F.output_options(drop_duplicates=True, max_alignments=1), realign=F.realign_options())
    for name, which, gt, ad, qual in (("first", reads, "1/1", "0,5", "43.89"), ("second", more, "0/1", "3,5", "23.78")):
        _, rows = library_rows(ctx, tool_aligner.align_reads(which), len(which), lengths)
        body = run_tool(name, which)
        assert body == vcf_lines(rows, names, chroms)
        dels = [l.split("\t") for l in body if "SVTYPE=DEL" in l]
        assert len(dels) == 1
        d = dels[0]
        assert (d[0], d[1], d[4], d[5], d[6]) == ("chr0", str(DEL_AT + 2), "<DEL>", qual, "PASS") and d[3] == "$ACGTN"[chroms[0][DEL_AT + 1]]
        assert d[7] == f"SVTYPE=DEL;END={DEL_AT + 82};SVLEN=-80;CIPOS=0,0;SUPPORT=5"
        assert d[9].split(":")[0] == gt and d[9].split(":")[3] == ad and d[9].split(":")[2] == str(sum(int(x) for x in ad.split(",")))
        every = run_tool(name + "_all", which, "--all-rows")
        assert every == vcf_lines(rows, names, chroms, all_rows=True)
        assert [l for l in every if l.split("\t")[9].split(":")[0] != "0/0"] == body
    # the docstring's precondition: without the realignment the deletion scatters over short words and no DEL line is written
    assert [l for l in run_tool("plain", reads, "--no-realign-affine") if "SVTYPE=DEL" in l] == []
    # a wrong output extension is refused before a device is touched
    r = subprocess.run([tool, "--reference", fasta, "--queries", str(tmp_path / "first.fastq"), "--error-probability", str(E2E_RATE), "--output", str(tmp_path / "sv.bcf")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 255 and r.stderr.startswith(b"[CLI PARSER ERROR]\n") and b"[vcf]" in r.stderr and not os.path.exists(tmp_path / "sv.bcf")
