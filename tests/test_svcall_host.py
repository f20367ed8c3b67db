"""Structural-variant calls without a GPU (flx_svcall): flx_svcall_host against the plain-Python rule of tests/svcall_ref.py on random
records and clusters, the window bound at its edges, the genotype boundary at the defaults, the clamps, every refusal with its message,
the ABI's sizes and names, the option defaults, and tests/svcall_check.cpp: the rule header against a walk over every span under ASan + UBSan."""
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
W = S.word
LENGTHS = [1000, 3000, 800, 30_000]


def host(lengths, rec, words, clusters, o=None):
    o = o or R.options()
    return F.svcall_host(lengths, rec, words, S.cluster_array(R.cluster_tuples(clusters)), R.c_options(o))


def check(lengths, rec, words, clusters, o=None):
    o = o or R.options()
    got, want = host(lengths, rec, words, clusters, o), R.expected(rec, words, clusters, lengths, o)
    assert len(got) == len(want) and got.tobytes() == want.tobytes(), (R.row_tuples(got)[:4], R.row_tuples(want)[:4])
    return R.row_tuples(got)


def spans_as_records(spans, flag=0, mapq=0):
    """one record of a single = word per (ref, rs, re)"""
    return S.records_of([(flag, ref, rs, i, mapq, [W("=", re - rs)]) for i, (ref, rs, re) in enumerate(spans)])


def dele(ref, pos, q, support=1, pos_max=None, q_min=None, q_max=None):
    return (R.DEL, 0, 0, support, ref, ref, pos, pos if pos_max is None else pos_max, q if q_min is None else q_min, q, q if q_max is None else q_max)


def ins(ref, pos, q, support=1):
    return (R.INS, 0, 0, support, ref, ref, pos, pos, q, q, q)


def test_host_rule_equals_the_reference_on_random_records():
    rng = np.random.default_rng(20261021)
    seen = set()
    for case in range(10):
        rec, words, _ = S.random_records(rng, LENGTHS, 150 + 30 * case)
        clusters = R.random_clusters(rng, LENGTHS, 200)
        # clusters that sit inside the records, so that many are spanned
        for r in rec[:: 3]:
            if int(r["ref"]) >= 0 and not int(r["flag"]) & 4:
                clusters.append(dele(int(r["ref"]), int(r["pos"]) + int(rng.integers(0, 60)), int(rng.integers(1, 40)), support=int(rng.integers(0, 4))))
        clusters = [c for c in clusters if c[0] == R.BND or c[7] + c[10] <= LENGTHS[c[4]]]
        o = R.options(count_secondary=bool(case % 2), min_mapq=0 if case % 3 else 20, flank=int(rng.integers(0, 3)) * int(rng.integers(1, 40)), min_depth=int(rng.integers(0, 4)),
                      min_qual=int(rng.integers(0, 2)) * int(rng.integers(1, 3000)))
        rows = check(LENGTHS, rec, words, clusters, o)
        assert len(rows) == sum(c[0] != R.BND for c in clusters) and [r[0] for r in rows] == [i for i, c in enumerate(clusters) if c[0] != R.BND]
        seen |= {(r[11], r[17], r[10] > 0) for r in rows}
    assert {g for g, _, _ in seen} == {0, 1, 2} and {p for _, p, _ in seen} == {0, 1} and {s for _, _, s in seen} == {False, True}


def test_the_window_bound_at_its_edges():
    o = R.options(flank=10)
    lengths = [5000, 1000, 1000]
    cl = [dele(1, 100, 20)]                                               # lo' = 90, hi' = 130
    for spans, want in (([(1, 90, 130)], 1), ([(1, 91, 130)], 0), ([(1, 90, 129)], 0), ([(1, 89, 131), (1, 90, 130), (1, 91, 131), (1, 0, 129)], 2),
                        ([(0, 0, 5000), (1, 90, 130), (1, 0, 1000)], 2),              # the record that sets max_span lies on another sequence
                        ([(0, 90, 130), (2, 90, 130)], 0), ([(0, 90, 130), (1, 90, 130), (2, 90, 130), (1, 90, 130)], 2),
                        ([(1, 0, 40), (1, 90, 130)], 1), ([(1, 0, 39), (1, 95, 134)], 0), ([], 0)):
        rec, words = spans_as_records(spans)
        assert [r[10] for r in check(lengths, rec, words, cl, o)] == [want], spans
    # hi' < max_span: the window starts at the sequence's first position
    rec, words = spans_as_records([(0, 0, 4000), (1, 0, 200), (1, 0, 129), (1, 50, 900), (1, 91, 1000)])
    assert [r[10] for r in check(lengths, rec, words, cl, o)] == [2]
    # lo' clamps at 0 and hi' at the sequence's end
    rec, words = spans_as_records([(1, 0, 25), (1, 1, 25), (1, 0, 24), (1, 989, 1000), (1, 990, 1000), (1, 970, 1000), (1, 970, 999)])
    assert [r[10] for r in check(lengths, rec, words, [dele(1, 5, 10, support=0), ins(1, 999, 60, support=0), dele(1, 980, 20, support=0)], o)] == [1, 2, 1]
    # a cluster's own ranges: lo from pos_a_min, hi from pos_a_max + q_max
    rec, words = spans_as_records([(1, 90, 175), (1, 90, 174), (1, 91, 175)])
    assert [r[10] for r in check(lengths, rec, words, [dele(1, 100, 20, pos_max=140, q_min=10, q_max=25), (R.INS, 0, 0, 1, 1, 1, 100, 164, 60, 70, 80)], o)] == [1, 1]


def test_the_genotype_boundary_at_the_defaults():
    lengths = [1000]

    def one(carriers, others, **kw):
        rec, words = spans_as_records([(0, 0, 1000)] * (carriers + others))
        (r,) = check(lengths, rec, words, [dele(0, 500, 80, support=carriers)], R.options(**kw))
        return dict(zip(F.SVCALL_ROW_DTYPE.names[:14] + ("pl0", "pl1", "pl2", "pass"), r))

    r = one(6, 6)
    assert 6 * 36 + 6 * 1574 - 12 * 325 - 3000 == 2760
    assert (r["gt"], r["qual"], r["pass"], r["alt_n"], r["ref_n"], r["span_n"]) == (1, 2760, 1, 6, 6, 12)
    r = one(5, 5)
    assert (r["gt"], r["qual"], r["pass"]) == (1, 1800, 0)                # below the default min_qual of 2000
    assert one(5, 5, min_qual=1800)["pass"] == 1 and one(5, 5, min_qual=1801)["pass"] == 0
    r = one(5, 0)
    assert 5 * 1574 - 5 * 36 - 3301 == 4389
    assert (r["gt"], r["qual"], r["pass"], r["ref_n"]) == (2, 4389, 1, 0)
    # the default min_depth of 4 (three carriers alone have a qual of 3 * 1574 - 3 * 36 - 3301 = 1313: min_qual is taken out of the way)
    assert one(3, 0, min_qual=1)["pass"] == 0 and one(3, 0, min_depth=3, min_qual=1)["pass"] == 1 and one(4, 0, min_qual=1)["pass"] == 1 and one(4, 0)["pass"] == 1
    r = one(0, 8)
    assert (r["gt"], r["qual"], r["pass"]) == (0, 0, 0)
    # ref_n clamps at 0 when alt_n > span_n
    rec, words = spans_as_records([(0, 0, 1000)] * 2)
    (r,) = check(lengths, rec, words, [ins(0, 500, 60, support=7)])
    assert (r[8], r[9], r[10]) == (7, 0, 2)
    # other costs move the boundary as the reference says
    for kw in (dict(cost_match=10, cost_het=300, cost_mismatch=2000), dict(prior_het=1, prior_hom=1), dict(prior_het=1 << 20, prior_hom=1 << 20)):
        for carriers, others in ((1, 9), (3, 3), (9, 1), (0, 4), (4, 0)):
            one(carriers, others, **kw)


def test_which_records_count():
    rows = [(0, 0, 0, 0, 30, [W("S", 5), W("=", 400), W("I", 70), W("X", 100), W("D", 100), W("=", 300), W("S", 9)]),     # span 900: I and S do not count
            (256, 0, 0, 1, 30, [W("=", 900)]), (4, -1, 0, 2, 0, []), (2048, 0, 0, 3, 5, [W("=", 900)]), (16, 0, 100, 4, 30, [W("=", 900)])]
    rec, words = S.records_of(rows)
    cl = [dele(0, 300, 100, support=1)]
    assert R.spans(rec, words, R.options()) == [(0, 0, 900), (0, 0, 900), (0, 100, 1000)]
    assert [r[10] for r in check([1000], rec, words, cl)] == [3]
    assert [r[10] for r in check([1000], rec, words, cl, R.options(count_secondary=True))] == [4]
    assert [r[10] for r in check([1000], rec, words, cl, R.options(min_mapq=6))] == [2]
    assert [r[10] for r in check([1000], rec, words, [dele(0, 850, 50)], R.options(flank=1))] == [1]      # only the record that ends on its sequence's last position reaches


def test_every_refusal_with_its_message():
    rec, words = spans_as_records([(0, 0, 100), (1, 0, 50)])
    lengths = [100, 50]
    good = [dele(0, 10, 5)]
    for bad, message in (((3, 0, 0, 1, 0, 0, 1, 1, 1, 1, 1), "type above 2"), (dele(2, 1, 1), "outside the lengths"), ((R.BND, 0, 0, 1, 0, 2, 1, 1, 1, 1, 1), "outside the lengths"),
                         ((R.BND, 0, 0, 1, -1, 0, 1, 1, 1, 1, 1), "outside the lengths"), ((R.INS, 0, 0, 1, 0, 1, 1, 1, 1, 1, 1), "outside the lengths"),
                         (dele(0, 2, 1, pos_max=1), "pos_a_min above pos_a_max"), (dele(0, 1, 1, q_min=2, q_max=3), "q_min <= q_median <= q_max"),
                         ((R.INS, 0, 0, 1, 0, 0, 1, 1, 1, 3, 2), "q_min <= q_median <= q_max"), (dele(1, 41, 10), "ends behind its sequence"),
                         (ins(1, 50, 10), "at or behind its sequence's end")):
        with pytest.raises(F.FloxerError, match=f"flx_svcall_host: cluster 1 .*{re.escape(message)}"):
            host(lengths, rec, words, good + [bad])
    arr = S.cluster_array(good * 2)
    arr["res"][1] = 1
    with pytest.raises(F.FloxerError, match="cluster 1 has a non-zero reserved field"):
        F.svcall_host(lengths, rec, words, arr)
    # the last valid ones; a BND's q fields are not judged
    assert len(host(lengths, rec, words, [dele(1, 40, 10), ins(1, 49, 10), (R.BND, 1, 0, 1, 0, 1, 1, 1, 9, 2, 1)])) == 2
    # options
    bad = capi.SvcallOptions()
    bad.reserved[0] = 1
    for o, message in ((bad, "reserved"), (F.svcall_options(flank=(1 << 20) + 1), "flank is above 2\\^20"), (F.svcall_options(cost_het=1574), "cost_match < cost_het < cost_mismatch"),
                       (F.svcall_options(cost_match=325), "cost_match < cost_het < cost_mismatch"), (F.svcall_options(prior_hom=(1 << 20) + 1), "a cost is above 2\\^20"),
                       (F.svcall_options(cost_mismatch=(1 << 20) + 1), "a cost is above 2\\^20")):
        with pytest.raises(F.FloxerError, match="flx_svcall_options: .*" + message):
            F.svcall_host(lengths, rec, words, S.cluster_array(good), o)
    for o in (F.svcall_options(flank=1 << 20), F.svcall_options(cost_het=1573), F.svcall_options(cost_match=324), F.svcall_options(prior_het=1 << 20)):
        F.svcall_host(lengths, rec, words, S.cluster_array(good), o)
    # records: all that coverage_plan refuses, with coverage's messages
    for row, message in (((0, 0, 60, 0, 0, [W("=", 41)]), "ends behind its sequence"), ((0, 2, 0, 0, 0, [W("=", 1)]), "reference_id outside the list"), ((0, 0, 0, 0, 0, [W("M", 5)]), "other than = X I D S"),
                         ((0, 0, 0, 0, 0, []), "no CIGAR words"), ((0, 0, -1, 0, 0, [W("=", 1)]), "negative position"), ((0, 0, 0, 0, 0, [W("=", 0)]), "length 0")):
        rec2, words2 = S.records_of([(0, 0, 0, 0, 0, [W("=", 100)]), row])
        with pytest.raises(F.FloxerError, match="flx_svcall_host: record 1 .*" + message):
            F.svcall_host(lengths, rec2, words2, S.cluster_array(good))
    rec2, words2 = S.records_of([(0, 0, 0, 0, 0, [W("=", 100)])])
    rec2["clen"] = 2
    with pytest.raises(F.FloxerError, match="outside the pool"):
        F.svcall_host(lengths, rec2, words2, S.cluster_array(good))
    with pytest.raises(F.FloxerError, match="no reference lengths"):
        F.svcall_host([], rec, words, S.cluster_array(good))
    # a row buffer that is too small says how many rows there are and writes nothing
    L = capi.lib()
    lens = np.asarray(lengths, dtype=np.uint64)
    cl = S.cluster_array(good * 3)
    out = np.full(3, 7, dtype=F.SVCALL_ROW_DTYPE)
    n = C.c_uint64(2)
    args = (capi.ptr(lens, capi.u64p), 2, None, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), capi.ptr(words, capi.u32p), len(words), cl.ctypes.data_as(C.POINTER(capi.SvCluster)), 3)
    assert L.flx_svcall_host(*args, out.ctypes.data_as(C.POINTER(capi.SvcallRow)), C.byref(n)) == -3 and n.value == 3 and (out["cluster"] == 7).all()
    assert L.flx_svcall_host(*args, out.ctypes.data_as(C.POINTER(capi.SvcallRow)), C.byref(n)) == 0 and list(out["cluster"]) == [0, 1, 2]
    # no clusters: no rows
    assert len(F.svcall_host(lengths, rec, words, np.zeros(0, dtype=F.SV_CLUSTER_DTYPE))) == 0


def test_symbols_sizes_and_python_names():
    L = capi.lib()
    names = [n for n in capi.EXPORTED if n.startswith("flx_svcall_")]
    header = open(os.path.join(ROOT, "include", "floxer_amd.h")).read()
    assert set(names) == {n for n in re.findall(r"\b(flx_[a-z0-9_]+)\s*\(", header) if n.startswith("flx_svcall_")}
    for name in names:
        getattr(L, name)
    assert set(names) == {"flx_svcall_host"}
    assert header.index("flx_phase_host(") < header.index("typedef struct flx_svcall_options")          # the section lies behind the phase section
    assert C.sizeof(capi.SvcallOptions) == 48 and C.sizeof(capi.SvcallRow) == 72 and F.SVCALL_ROW_DTYPE.itemsize == 72
    assert [F.SVCALL_ROW_DTYPE.fields[n][1] for n in F.SVCALL_ROW_DTYPE.names] == [getattr(capi.SvcallRow, f[0]).offset for f in capi.SvcallRow._fields_]
    assert F.SVCALL_ROW_DTYPE.names == ("cluster", "type", "ref", "pos_a_min", "pos_a_max", "q_min", "q_median", "q_max", "alt_n", "ref_n", "span_n", "gt", "gq", "qual", "pl", "pass")
    o = F.svcall_options(count_secondary=True, min_mapq=7, flank=9, min_depth=5, min_qual=1500, cost_match=1, cost_mismatch=3, cost_het=2, prior_het=4, prior_hom=5)
    assert (o.count_secondary, o.min_mapq, o.flank, o.min_depth, o.min_qual, o.cost_match, o.cost_mismatch, o.cost_het, o.prior_het, o.prior_hom, list(o.reserved)) == \
        (1, 7, 9, 5, 1500, 1, 3, 2, 4, 5, [0, 0])
    d = F.svcall_options()
    assert all(getattr(d, f[0]) == 0 for f in capi.SvcallOptions._fields_ if f[0] != "reserved") and list(d.reserved) == [0, 0]
    assert R.model(R.options()) == (50, 4, 2000, 36, 1574, 325, 3000, 3301)
    for name in ("svcall_options", "svcall_host", "SVCALL_ROW_DTYPE"):
        assert hasattr(F, name)


def test_rule_header_against_a_walk_over_every_span_under_sanitizers(tmp_path):
    """tests/svcall_check.cpp: flx_svcall.hpp on random records and clusters, built with ASan + UBSan; nothing is preloaded"""
    exe = str(tmp_path / "svcall_check")
    src = os.path.join(ROOT, "tests", "svcall_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
