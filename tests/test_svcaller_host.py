"""The svcaller object without a GPU (flx_svcaller with device -1, the host form): rows, spans and max_span against the plain-Python rule
of tests/svcall_ref.py on random records, fed in one add, in five adds cut anywhere and through an absorb; the copy contract of
flx_svcaller_copy_rows at capacities n - 1, n and n + 1; every refusal with its message; the ABI's names and sizes; the parser of the
tool floxer_sv and its derived costs against floxer_variants'; and tests/svcaller_check.cpp, the HIP-free half of the object under
ASan + UBSan in a program of its own."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import sv_ref as S
import svcall_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "floxer_amd", "floxer_sv")
VARIANTS_TOOL = os.path.join(ROOT, "floxer_amd", "floxer_variants")
GOLDEN = os.path.join(ROOT, "tests", "golden")
W = S.word
LENGTHS = [1000, 3000, 800, 30_000]


def span_array(spans):
    out = np.zeros(len(spans), dtype=F.SVCALL_SPAN_DTYPE)
    for i, (ref, rs, re_) in enumerate(sorted(spans)):
        out[i] = (ref, rs, re_, 0)
    return out


def max_span_of(spans):
    return max((re_ - rs for _, rs, re_ in spans), default=0)


def random_case(rng, case):
    """test_svcall_host's generator: random records, random clusters, clusters inside the records, an option mix"""
    rec, words, _ = S.random_records(rng, LENGTHS, 150 + 30 * case)
    clusters = R.random_clusters(rng, LENGTHS, 200)
    for r in rec[:: 3]:
        if int(r["ref"]) >= 0 and not int(r["flag"]) & 4:
            clusters.append(dele(int(r["ref"]), int(r["pos"]) + int(rng.integers(0, 60)), int(rng.integers(1, 40)), support=int(rng.integers(0, 4))))
    clusters = [c for c in clusters if c[0] == R.BND or c[7] + c[10] <= LENGTHS[c[4]]]
    o = R.options(count_secondary=bool(case % 2), min_mapq=0 if case % 3 else 20, flank=int(rng.integers(0, 3)) * int(rng.integers(1, 40)), min_depth=int(rng.integers(0, 4)),
                  min_qual=int(rng.integers(0, 2)) * int(rng.integers(1, 3000)))
    return rec, words, clusters, o


def cuts(rng, n, pieces):
    at = sorted(int(x) for x in rng.integers(0, n + 1, pieces - 1))
    return list(zip([0] + at, at + [n]))


def finished(rec, words, clusters, o, ranges, lengths=LENGTHS, device=-1, absorb_from=None, **kw):
    """an object fed rec[a:b] for every (a, b) of ranges and finished; with absorb_from the ranges from that index on go to a second
    object, which is absorbed; returns (rows, spans, max_span)"""
    s = F.svcaller(options=R.c_options(o), lengths=lengths, device=device, **kw)
    other = F.svcaller(options=R.c_options(o), lengths=lengths, device=device, **kw) if absorb_from is not None else None
    for i, (a, b) in enumerate(ranges):
        (other if other is not None and i >= absorb_from else s).add_records(rec[a:b], words)
    if other is not None:
        s.absorb(other)
        other.finish([])
        assert len(other.spans()) == 0 and other.max_span() == 0 and len(other.rows()) == 0      # `from` is left empty
        other.close()
    s.finish(S.cluster_array(R.cluster_tuples(clusters)))
    out = s.rows(), s.spans(), s.max_span()
    s.close()
    return out


def test_host_form_equals_the_reference_in_one_add_in_five_adds_and_through_an_absorb():
    rng = np.random.default_rng(20261021)
    seen = set()
    for case in range(6):
        rec, words, clusters, o = random_case(rng, case)
        want_rows = R.expected(rec, words, clusters, LENGTHS, o)
        spans = R.spans(rec, words, o)
        want_spans, want_max = span_array(spans), max_span_of(spans)
        n = len(rec)
        for ranges, absorb_from in (([(0, n)], None), (cuts(rng, n, 5), None), (cuts(rng, n, 2), 1), (cuts(rng, n, 4), 2)):
            rows, got_spans, got_max = finished(rec, words, clusters, o, ranges, absorb_from=absorb_from)
            assert len(rows) == len(want_rows) and rows.tobytes() == want_rows.tobytes(), (case, ranges, R.row_tuples(rows)[:3], R.row_tuples(want_rows)[:3])
            assert got_spans.tobytes() == want_spans.tobytes() and got_max == want_max, (case, ranges)
        seen |= {(int(r["gt"]), int(r["pass"]), int(r["span_n"]) > 0) for r in want_rows}
        # the one-call form gives the same rows
        assert F.svcall_host(LENGTHS, rec, words, S.cluster_array(R.cluster_tuples(clusters)), R.c_options(o)).tobytes() == want_rows.tobytes()
    assert {g for g, _, _ in seen} == {0, 1, 2} and {p for _, p, _ in seen} == {0, 1} and {s for _, _, s in seen} == {False, True}


def spans_as_records(spans):
    return S.records_of([(0, ref, rs, i, 0, [W("=", re_ - rs)]) for i, (ref, rs, re_) in enumerate(spans)])


def dele(ref, pos, q, support=1):
    return (R.DEL, 0, 0, support, ref, ref, pos, pos, q, q, q)


def test_rows_with_0_1_and_300_rows_and_the_copy_contract():
    L = capi.lib()
    rec, words = spans_as_records([(0, 0, 1000), (0, 100, 900), (1, 0, 3000)])
    o = R.options()
    for n in (0, 1, 300):
        clusters = [dele(0, 200 + (i % 400), 20, support=i % 3) for i in range(n)]
        clusters = clusters[: n // 2] + [(R.BND, 0, 1, 2, 0, 1, 5, 5, 7, 7, 7)] + clusters[n // 2:]      # a BND among them: a row's index is not its cluster's
        want = R.expected(rec, words, clusters, LENGTHS, o)
        assert len(want) == n
        s = F.svcaller(options=R.c_options(o), lengths=LENGTHS, device=-1)
        s.add_records(rec, words)
        s.finish(S.cluster_array(clusters))
        assert L.flx_svcaller_num_rows(s.h) == n and L.flx_svcaller_num_spans(s.h) == 3
        got = s.rows()
        assert len(got) == n and got.tobytes() == want.tobytes()
        rowp = C.POINTER(capi.SvcallRow)
        # capacity n into a buffer of n + 1 rows: the last row keeps its sentinel; a larger capacity writes num_rows rows as well
        for capacity in (n, n + 1):
            out = np.full(n + 1, 0xAB, dtype=np.uint8).repeat(72).view(F.SVCALL_ROW_DTYPE)
            assert len(out) == n + 1
            assert L.flx_svcaller_copy_rows(s.h, out.ctypes.data_as(rowp), capacity) == 0
            assert out[:n].tobytes() == want.tobytes() and out[n:].tobytes() == b"\xab" * 72
        if n:
            # capacity n - 1: FLX_ERR_CAPACITY, the message says how many rows there are, and nothing is written
            out = np.full(n * 72, 0xAB, dtype=np.uint8).view(F.SVCALL_ROW_DTYPE)
            assert L.flx_svcaller_copy_rows(s.h, out.ctypes.data_as(rowp), n - 1) == -3
            assert f"the row buffer is too small, {n} rows" in L.flx_last_error().decode() and out.tobytes() == b"\xab" * (72 * n)
            assert L.flx_svcaller_copy_rows(s.h, None, n) == -1 and "null argument" in L.flx_last_error().decode()
        else:
            assert L.flx_svcaller_copy_rows(s.h, None, 0) == 0            # no rows: no buffer is needed
        s.close()


def test_every_refusal_with_its_message():
    L = capi.lib()
    lengths = [100, 50]
    rec, words = spans_as_records([(0, 0, 100), (1, 0, 50), (0, 10, 60)])
    good = S.cluster_array([dele(0, 10, 5)])
    new = lambda lens=lengths, **kw: F.svcaller(options=F.svcall_options(**kw), lengths=lens, device=-1)      # noqa: E731

    # before a finish: the counts are 0 and the copy calls are refused
    s = new()
    s.add_records(rec, words)
    assert L.flx_svcaller_num_spans(s.h) == 0 and L.flx_svcaller_num_rows(s.h) == 0 and s.max_span() == 0
    with pytest.raises(F.FloxerError, match="flx_svcaller_copy_rows: call flx_svcaller_finish first"):
        s.rows()
    with pytest.raises(F.FloxerError, match="flx_svcaller_copy_spans: call flx_svcaller_finish first"):
        s.spans()
    # a refused add leaves the object as it was: coverage's refusals with coverage's messages
    for row, message in (((0, 0, 60, 0, 0, [W("=", 41)]), "ends behind its sequence"), ((0, 2, 0, 0, 0, [W("=", 1)]), "reference_id outside the list"),
                         ((0, 0, 0, 0, 0, [W("M", 5)]), "other than = X I D S"), ((0, 0, 0, 0, 0, []), "no CIGAR words \\(a run made with without_cigar"),
                         ((0, 0, -1, 0, 0, [W("=", 1)]), "negative position"), ((0, 0, 0, 0, 0, [W("=", 0)]), "length 0")):
        rec2, words2 = S.records_of([(0, 0, 0, 0, 0, [W("=", 100)]), row])
        with pytest.raises(F.FloxerError, match="flx_svcaller_add_records: record 1 .*" + message):
            s.add_records(rec2, words2)
    rec2, words2 = S.records_of([(0, 0, 0, 0, 0, [W("=", 100)])])
    rec2["clen"] = 2
    with pytest.raises(F.FloxerError, match="outside the pool"):
        s.add_records(rec2, words2)
    # every cluster refusal at finish leaves the object unfinished and unchanged
    for bad, message in (((3, 0, 0, 1, 0, 0, 1, 1, 1, 1, 1), "type above 2"), (dele(2, 1, 1), "outside the lengths"), ((R.BND, 0, 0, 1, 0, 2, 1, 1, 1, 1, 1), "outside the lengths"),
                         ((R.BND, 0, 0, 1, -1, 0, 1, 1, 1, 1, 1), "outside the lengths"), ((R.INS, 0, 0, 1, 0, 1, 1, 1, 1, 1, 1), "outside the lengths"),
                         ((R.DEL, 0, 0, 1, 0, 0, 2, 1, 1, 1, 1), "pos_a_min above pos_a_max"), ((R.DEL, 0, 0, 1, 0, 0, 1, 1, 2, 1, 3), "q_min <= q_median <= q_max"),
                         ((R.INS, 0, 0, 1, 0, 0, 1, 1, 1, 3, 2), "q_min <= q_median <= q_max"), (dele(1, 41, 10), "ends behind its sequence"),
                         ((R.INS, 0, 0, 1, 1, 1, 50, 50, 10, 10, 10), "at or behind its sequence's end")):
        with pytest.raises(F.FloxerError, match=f"flx_svcaller_finish: cluster 1 .*{re.escape(message)}"):
            s.finish(S.cluster_array([dele(0, 10, 5), bad]))
        assert L.flx_svcaller_num_spans(s.h) == 0                        # still unfinished
    arr = S.cluster_array([dele(0, 10, 5)] * 2)
    arr["res"][1] = 1
    with pytest.raises(F.FloxerError, match="flx_svcaller_finish: cluster 1 has a non-zero reserved field"):
        s.finish(arr)
    # ... and usable: one more add, then a finish with good clusters gives the reference's rows
    s.add_records(rec[:1], words)
    both = np.concatenate([rec, rec[:1]])
    cl = [dele(0, 10, 5), dele(1, 40, 10), (R.INS, 0, 0, 3, 1, 1, 49, 49, 10, 10, 10), (R.BND, 1, 0, 1, 0, 1, 1, 1, 9, 2, 1)]
    s.finish(S.cluster_array(cl))
    assert s.rows().tobytes() == R.expected(both, words, cl, lengths, R.options()).tobytes() and len(s.rows()) == 3
    assert s.spans().tobytes() == span_array(R.spans(both, words, R.options())).tobytes() and s.max_span() == 100
    # behind the finish: add, absorb (either way) and finish
    with pytest.raises(F.FloxerError, match="flx_svcaller_add_records: the svcaller object is finished"):
        s.add_records(rec, words)
    with pytest.raises(F.FloxerError, match="flx_svcaller_finish: the svcaller object is finished"):
        s.finish(good)
    t = new()
    for a, b in ((s, t), (t, s)):
        with pytest.raises(F.FloxerError, match="flx_svcaller_absorb: an svcaller object is finished"):
            a.absorb(b)
    # a stretch outside the spans
    n = L.flx_svcaller_num_spans(s.h)
    out = np.full(n + 1, 7, dtype=F.SVCALL_SPAN_DTYPE)
    spanp = C.POINTER(capi.SvcallSpan)
    for a, b in ((0, n + 1), (2, 1), (n + 1, n + 1)):
        assert L.flx_svcaller_copy_spans(s.h, a, b, out.ctypes.data_as(spanp)) == -1 and "a stretch outside the spans" in L.flx_last_error().decode()
    assert (out["rs"] == 7).all()
    assert L.flx_svcaller_copy_spans(s.h, 1, 3, out.ctypes.data_as(spanp)) == 0 and out[:2].tobytes() == s.spans()[1:3].tobytes() and (out["rs"][2:] == 7).all()
    assert L.flx_svcaller_copy_spans(s.h, 0, n, None) == -1 and "null argument" in L.flx_last_error().decode()
    assert L.flx_svcaller_copy_spans(s.h, n, n, None) == 0
    # absorb: into itself, other lengths, other options, a host form and a null
    with pytest.raises(F.FloxerError, match="flx_svcaller_absorb: null argument, or an object absorbed into itself"):
        t.absorb(t)
    u = new([100, 51])
    with pytest.raises(F.FloxerError, match="flx_svcaller_absorb: the objects belong to different reference lengths"):
        t.absorb(u)
    for kw in (dict(flank=51), dict(min_mapq=1), dict(count_secondary=True), dict(min_qual=1999), dict(cost_het=300)):
        v = new(**kw)
        with pytest.raises(F.FloxerError, match="flx_svcaller_absorb: the objects have different options"):
            t.absorb(v)
        v.close()
    v = new(flank=50, min_depth=4, min_qual=2000, cost_match=36, prior_hom=3301)        # the defaults spelled out are the defaults
    v.add_records(rec, words)
    t.absorb(v)
    t.finish(good)
    assert len(t.spans()) == 3
    for o in (s, t, u, v):
        o.close()
    # null arguments and the create's refusals
    h = C.c_void_p()
    lens = np.asarray(lengths, dtype=np.uint64)
    lp = capi.ptr(lens, capi.u64p)
    assert L.flx_svcaller_create_for_lengths(-1, lp, 2, None, 0, None) == -1 and "flx_svcaller_create_for_lengths: null argument" in L.flx_last_error().decode()
    assert L.flx_svcaller_create_for_lengths(-2, lp, 2, None, 0, C.byref(h)) == -1 and "a device below -1" in L.flx_last_error().decode()
    assert L.flx_svcaller_create_for_lengths(-1, lp, 2, None, 1 << 32, C.byref(h)) == -1 and "initial_capacity above 2^32 - 1" in L.flx_last_error().decode()
    assert L.flx_svcaller_create_for_lengths(-1, None, 0, None, 0, C.byref(h)) == -1 and "no reference lengths" in L.flx_last_error().decode()
    assert L.flx_svcaller_create(None, None, C.byref(h)) == -1 and "flx_svcaller_create: null argument" in L.flx_last_error().decode()
    bad = capi.SvcallOptions()
    bad.reserved[1] = 1
    for o, message in ((bad, "reserved"), (F.svcall_options(flank=(1 << 20) + 1), "flank is above 2^20"), (F.svcall_options(cost_het=1574), "cost_match < cost_het < cost_mismatch")):
        assert L.flx_svcaller_create_for_lengths(-1, lp, 2, C.byref(o), 0, C.byref(h)) == -1 and "flx_svcall_options: " in L.flx_last_error().decode() and message in L.flx_last_error().decode()
    assert not h
    for call, args in (("add_records", (None, None, 0, None, 0)), ("add_run", (None, None)), ("absorb", (None, None)), ("finish", (None, None, 0)), ("copy_spans", (None, 0, 0, None)),
                       ("copy_rows", (None, None, 0)), ("geometry", (None,))):
        assert getattr(L, "flx_svcaller_" + call)(*args) == -1 and f"flx_svcaller_{call}: null argument" in L.flx_last_error().decode(), call
    assert L.flx_svcaller_num_spans(None) == 0 and L.flx_svcaller_num_rows(None) == 0 and L.flx_svcaller_max_span(None) == 0
    L.flx_svcaller_free(None)
    s = new()
    assert L.flx_svcaller_add_records(s.h, None, 1, None, 0) == -1 and "null argument" in L.flx_last_error().decode()
    assert L.flx_svcaller_add_run(s.h, None) == -1 and L.flx_svcaller_finish(s.h, None, 1) == -1 and "flx_svcaller_finish: null argument" in L.flx_last_error().decode()
    s.finish([])                                                           # no spans, no clusters
    assert len(s.rows()) == 0 and len(s.spans()) == 0 and s.max_span() == 0
    s.close()
    with pytest.raises(F.FloxerError, match="needs a context or a list of reference lengths"):
        F.svcaller()


def test_symbols_sizes_and_python_names():
    L = capi.lib()
    names = [n for n in capi.EXPORTED if n.startswith("flx_svcaller_")]
    header = open(os.path.join(ROOT, "include", "floxer_amd.h")).read()
    assert set(names) == {n for n in re.findall(r"\b(flx_[a-z0-9_]+)\s*\(", header) if n.startswith("flx_svcaller_")}
    assert set(names) == {"flx_svcaller_" + n for n in ("create", "create_for_lengths", "free", "add_records", "add_run", "absorb", "finish", "num_spans", "num_rows", "max_span",
                                                        "copy_spans", "copy_rows", "geometry")}
    for name in names:
        getattr(L, name)
    assert header.index("flx_svcall_host(") < header.index("typedef struct flx_svcaller flx_svcaller") < header.index("PAF output")
    assert C.sizeof(capi.SvcallSpan) == 16 and F.SVCALL_SPAN_DTYPE.itemsize == 16 and C.sizeof(capi.SvcallOptions) == 48 and C.sizeof(capi.SvcallRow) == 72
    assert F.SVCALL_SPAN_DTYPE.names == ("ref", "rs", "re", "res")
    assert [F.SVCALL_SPAN_DTYPE.fields[n][1] for n in F.SVCALL_SPAN_DTYPE.names] == [getattr(capi.SvcallSpan, f[0]).offset for f in capi.SvcallSpan._fields_] == [0, 4, 8, 12]
    g = F.svcaller_geometry()
    assert set(g) == {"spans_grid_cap", "count_grid_cap", "waves_per_block", "sort_tile"} and all(v > 0 for v in g.values())
    assert all(g[k] & (g[k] - 1) == 0 for k in ("spans_grid_cap", "count_grid_cap"))
    assert g["sort_tile"] == F.sort_geometry()[0]
    for name in ("svcaller", "svcaller_geometry", "SVCALL_SPAN_DTYPE"):
        assert hasattr(F, name)
    assert "svcaller(ctx, svcall_options())" in F.__doc__
    for method in ("add", "add_records", "absorb", "finish", "spans", "rows", "max_span", "close"):
        assert callable(getattr(F.svcaller, method))


def test_the_end_to_end_literals_from_the_documented_cigars():
    """What tests/test_svcaller_gpu.py pins for the planted deletion, derived here without a device: the five realigned CIGARs that
    tests/test_sv_gpu.py's end-to-end docstring records (402= 80D 1098= and so on, reads of 1500 cut 400 .. 1100 columns in front of a
    deletion of 80 at 20 000 and realigned two columns right), their cluster, and then three error-free reads of one = word."""
    lengths = [40_000, 40_000]
    carriers = [(16 if k % 2 else 0, 0, 20_000 - off, k, 60, [W("=", off + 2), W("D", 80), W("=", 1500 - off - 2)]) for k, off in enumerate((400, 600, 750, 900, 1100))]
    cl = [(R.DEL, 0, 0, 5, 0, 0, 20_002, 20_002, 80, 80, 80)]
    row = lambda r: tuple(int(r[k]) for k in ("ref_n", "alt_n", "span_n", "gt", "qual", "pass"))       # noqa: E731
    for others, want in (((), (0, 5, 5, 2, 4389, 1)), ((18_950, 19_300, 19_650), (3, 5, 8, 1, 2378, 1))):
        rec, words = S.records_of(carriers + [(0, 0, p, 5 + i, 60, [W("=", 1500)]) for i, p in enumerate(others)])
        assert S.clusters(S.signatures(rec, words, [1500] * len(rec), S.options()), S.options()) == cl
        ref_rows = R.expected(rec, words, cl, lengths, R.options())
        assert row(ref_rows[0]) == want
        s = F.svcaller(lengths=lengths, device=-1)
        s.add_records(rec, words)
        s.finish(S.cluster_array(cl))
        assert s.rows().tobytes() == ref_rows.tobytes()
        s.close()
    assert 3 * 36 + 5 * 1574 == 7978 and 8 * 325 + 3000 == 5600 and 5 * 36 + 3 * 1574 + 3301 == 8203 and 7978 - 5600 == 2378


# ------------------------------------------------------------------------------------------------ the tool's parser
def tool(*args, exe=TOOL, env_name="FLX_SV_PARSE_ONLY"):
    env = dict(os.environ, **{env_name: "1"})                              # the parser alone: no device is touched, no file is opened
    return subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def parsed(*args, **kw):
    r = tool(*args, **kw)
    assert r.returncode == 0 and r.stdout == b"" and b"CLI PARSER ERROR" not in r.stderr, (args, r.stderr)
    return dict(l.split("=", 1) for l in r.stderr.decode().splitlines())


def test_tool_parser_and_cost_derivation(tmp_path):
    ref, reads = os.path.join(GOLDEN, "reference.fasta"), os.path.join(GOLDEN, "queries.fastq")
    vcf = str(tmp_path / "sv.vcf")
    base = ["--reference", ref, "--queries", reads, "--output", vcf]
    h = subprocess.run([TOOL, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0 and h.stdout == b""
    lines = h.stderr.decode().splitlines()
    options = ("reference", "queries", "output", "query-errors", "error-probability", "device", "min-length", "max-distance", "min-support", "flank", "min-depth", "min-qual",
               "heterozygosity", "read-error", "secondary", "min-mapq", "no-realign-affine", "all-rows", "batch-reads", "sample")
    for name in options:
        assert len([l for l in lines if re.search(rf"^\s+(-\w, )?--{name}(\s|$)", l)]) == 1, name
    assert len(lines) == 1 + len(options) and lines[0].startswith("floxer_sv")
    cost_keys = ("cost-match", "cost-mismatch", "cost-het", "prior-het", "prior-hom")
    costs = lambda d: tuple(int(d[k]) for k in cost_keys)                 # noqa: E731
    # the defaults
    d = parsed(*base, "--error-probability", "0.08")
    assert costs(d) == R.DEFAULT_COSTS[:1] + (1574, 325, 3000, 3301) == (36, 1574, 325, 3000, 3301)
    assert [d[k] for k in ("device", "min-length", "max-distance", "min-support", "flank", "min-depth", "min-qual", "secondary", "min-mapq", "realign-affine", "all-rows", "batch-reads",
                           "sample", "output", "heterozygosity")] == ["0", "50", "100", "2", "50", "4", "2000", "0", "0", "1", "0", "16384", "SAMPLE", vcf, "0.001"]
    # the derived costs are floxer_variants' for the same --read-error and --heterozygosity
    vbase = ["--reference", ref, "--queries", reads, "--output", str(tmp_path / "calls.vcf")]
    for extra in (["-p", "0.08"], ["-p", "0.08", "--read-error", "0.01"], ["-p", "0.01"], ["-p", "0.05", "--read-error", "0.15"], ["-e", "3"], ["-p", "0.05", "--read-error", "0.00001"],
                  ["-p", "0.08", "--heterozygosity=0.01"], ["-p", "0.3", "--read-error", "0.5", "--heterozygosity", "0.5"], ["-e", "9", "--heterozygosity", "0.000000001"]):
        assert costs(parsed(*base, *extra)) == costs(parsed(*vbase, *extra, exe=VARIANTS_TOOL, env_name="FLX_VARIANTS_PARSE_ONLY")), extra
    assert costs(parsed(*base, "-p", "0.08", "--read-error", "0.01"))[:3] == (4, 2477, 304)
    d = parsed(*base, "-p", "0.05", "--min-length", "30", "--max-distance", "7", "--min-support", "3", "--flank", "9", "--min-depth", "7", "--min-qual", "8.3", "--secondary",
               "--min-mapq", "5", "--no-realign-affine", "--all-rows", "--batch-reads", "9", "--sample", "NA12878", "--device", "1")
    assert [d[k] for k in ("min-length", "max-distance", "min-support", "flank", "min-depth", "min-qual", "secondary", "min-mapq", "realign-affine", "all-rows", "batch-reads", "sample",
                           "device")] == ["30", "7", "3", "9", "7", "830", "1", "5", "0", "1", "9", "NA12878", "1"]
    # every range at its ends
    good = (["-e", "2"], ["-p", "0.00001", "--min-mapq", "254", "--batch-reads", "16777216"], ["-p", "0.99999", "--read-error", "0.5"], ["-e", "4096"],
            ["-p", "0.05", "--min-length", "1", "--max-distance", "1", "--min-support", "1", "--flank", "1", "--min-depth", "1", "--min-qual", "0.01", "--min-mapq", "1", "--batch-reads", "1"],
            ["-p", "0.05", "--min-length", "268435455", "--max-distance", "268435455", "--min-support", "1000000", "--flank", "1048576", "--min-depth", "1000000", "--device", "1023",
             "--heterozygosity", "0.5", "--min-qual", "10000"], ["-p", "0.05", "--heterozygosity", "0.000000001", "--read-error", "0.00001"])
    for extra in good:
        parsed(*base, *extra)
    bad = ([], ["-e", "1"], ["-e", "4097"], ["-p", "0.000001"], ["-p", "1"], ["-p", "x"], ["-e", "-1"], ["-p", "0.05", "--device", "1024"])
    for name, below, above in (("min-length", "0", "268435456"), ("max-distance", "0", "268435456"), ("min-support", "0", "1000001"), ("flank", "0", "1048577"),
                               ("min-depth", "0", "1000001"), ("min-qual", "0", "10001"), ("heterozygosity", "0", "0.51"), ("read-error", "0", "0.51"), ("min-mapq", "0", "255"),
                               ("batch-reads", "0", "16777217")):
        bad += (["-p", "0.05", "--" + name, below], ["-p", "0.05", "--" + name, above], ["-p", "0.05", "--" + name], ["-p", "0.05", "--" + name, "x"])
    bad += (["-p", "0.05", "--sample", "two words"], ["-p", "0.05", "--sample", ""], ["-p", "0.05", "--sam"], ["-p", "0.05", "--signatures", str(tmp_path / "sv.tsv")],
            ["-p", "0.05", "--realign-affine"], ["-p", "0.05", "stray"])
    for extra in bad:
        r = tool(*base, *extra)
        assert r.returncode == 255 and r.stderr.startswith(b"[CLI PARSER ERROR]\n") and r.stdout == b"", (extra, r.stderr)
    for args, what in ((["--queries", reads, "--output", vcf, "-p", "0.05"], b"-r/--reference is required"), (["--reference", ref, "--output", vcf, "-p", "0.05"], b"-q/--queries is required"),
                       (["--reference", ref, "--queries", reads, "-p", "0.05"], b"-o/--output is required"),
                       (["--reference", ref, "--queries", reads, "--output", str(tmp_path / "sv.bcf"), "-p", "0.05"], b"[vcf]"),
                       (["--reference", ref, "--queries", reads, "--output", str(tmp_path / "sv.vcf.gz"), "-p", "0.05"], b"[vcf]"),
                       (["--reference", reads, "--queries", reads, "--output", vcf, "-p", "0.05"], b"-r/--reference"),
                       (["--reference", ref, "--queries", ref, "--output", vcf, "-p", "0.05"], b"-q/--queries"),
                       (["--reference", str(tmp_path / "none.fa"), "--queries", reads, "--output", vcf, "-p", "0.05"], b"does not exist"),
                       (base, b"Either a fixed number of errors"), (base + ["-e", "1"], b"PEX tree leaves")):
        r = tool(*args)
        assert r.returncode == 255 and r.stderr.startswith(b"[CLI PARSER ERROR]\n") and what in r.stderr, (args, r.stderr)
    assert not os.path.exists(vcf)                                        # the parser alone writes nothing


def test_host_half_of_the_object_under_sanitizers(tmp_path):
    """tests/svcaller_check.cpp: flx_svcaller.hpp's host table, its absorb, its finish and both copy judgements on random records, built
    with ASan + UBSan into a program of its own; nothing is preloaded"""
    exe = str(tmp_path / "svcaller_check")
    src = os.path.join(ROOT, "tests", "svcaller_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
