"""Structural-variant signatures without a GPU (flx_sv_host, flx_sv_clusters_host, the CLI's option checks): the library's host rule
against the plain-Python rule of tests/sv_ref.py, every refusal, the length, anchor and position boundaries, the junction orientations
and orderings, the cluster boundaries, the CLI's parser errors, and tests/sv_check.cpp: the rule header under ASan + UBSan against a
word-by-word definition."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import sv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1000, 3000, 1977, 1500]
W = R.word


def _host(lengths, rec, words, read_lengths, opt, out, capacity, n_refs=None):
    lens = np.asarray(lengths, dtype=np.uint64)
    offs = F._read_offsets(read_lengths)
    n = C.c_uint64(capacity)
    rc = capi.lib().flx_sv_host(capi.ptr(lens, capi.u64p), len(lens) if n_refs is None else n_refs, C.byref(opt) if opt is not None else None, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec),
                                capi.ptr(words, capi.u32p) if len(words) else None, len(words), capi.ptr(offs, capi.u64p), len(offs) - 1,
                                out.ctypes.data_as(C.POINTER(capi.SvSignature)) if out is not None else None, C.byref(n))
    return rc, n.value


def _sigs(rows, read_lengths, o=None, lengths=LENGTHS):
    """the library's signatures of rows as tuples, checked against the reference"""
    o = o or R.options()
    rec, words = R.records_of(rows)
    got = F.sv_host(lengths, rec, words, read_lengths, R.c_options(o))
    want = R.signatures(rec, words, read_lengths, o)
    assert got.tobytes() == R.signature_array(want).tobytes(), (R.signature_tuples(got), want)
    return want


def _clusters(sigs, o=None):
    o = o or R.options()
    got = F.sv_clusters_host(R.signature_array(sigs), R.c_options(o))
    want = R.clusters(sigs, o)
    assert got.tobytes() == R.cluster_array(want).tobytes(), (got, want)
    return want


def test_symbols_and_struct_layout():
    L = capi.lib()
    names = [n for n in capi.EXPORTED if n.startswith("flx_sv_")]
    for name in names:
        getattr(L, name)
    assert len(names) == 13 and len(set(names)) == 13
    assert C.sizeof(capi.SvOptions) == 40 and C.sizeof(capi.SvSignature) == 32 and C.sizeof(capi.SvCluster) == 48
    assert F.SV_SIGNATURE_DTYPE.itemsize == 32 and F.SV_CLUSTER_DTYPE.itemsize == 48
    assert [F.SV_SIGNATURE_DTYPE.fields[k][1] for k in ("type", "side_a", "side_b", "res", "ref_a", "ref_b", "pos_a", "q")] == list(range(0, 32, 4))
    assert [F.SV_CLUSTER_DTYPE.fields[k][1] for k in ("type", "side_a", "side_b", "support", "ref_a", "ref_b", "pos_a_min", "pos_a_max", "q_min", "q_median", "q_max", "res")] == list(range(0, 48, 4))
    assert capi.SvOptions.initial_capacity.offset == 32
    o = F.sv_options(min_length=7, max_distance=9, min_support=3, count_secondary=True, min_mapq=5, initial_capacity=8)
    assert (o.min_length, o.max_distance, o.min_support, o.count_secondary, o.min_mapq, o.initial_capacity) == (7, 9, 3, 1, 5, 8)
    assert F.SV_TYPES == ("DEL", "INS", "BND")


def test_host_rule_equals_the_reference_on_random_records():
    rng = np.random.default_rng(47)
    rec, words, read_lengths = R.random_records(rng, LENGTHS, 300)
    assert {int(f) for f in rec["flag"]} == {0, 16, 256, 272, 2048, 2064, 4}
    seen = set()
    for sec, q, ml in itertools.product([False, True], [0, 30], [0, 4, 51]):
        o = R.options(count_secondary=sec, min_mapq=q, min_length=ml)
        want = R.signatures(rec, words, read_lengths, o)
        got = F.sv_host(LENGTHS, rec, words, read_lengths, R.c_options(o))
        assert got.tobytes() == R.signature_array(want).tobytes(), o
        assert {s[0] for s in want} == {R.DEL, R.INS, R.BND}
        seen.add(got.tobytes())
        for md, ms in ((0, 0), (1, 1), (400, 3), (3000, 1)):
            oo = dict(o, max_distance=md, min_support=ms)
            cl = F.sv_clusters_host(got, R.c_options(oo))
            assert cl.tobytes() == R.cluster_array(R.clusters(want, oo)).tobytes(), oo
            assert ms != 1 or int(cl["support"].sum()) == len(want)      # every signature lies in exactly one cluster
    assert len(seen) == 12                                               # every switch matters on this batch
    # NULL options are all zero; the order of the signatures given to the cluster call does not matter
    want = R.signatures(rec, words, read_lengths, R.options())
    out = np.zeros(len(want), dtype=F.SV_SIGNATURE_DTYPE)
    assert _host(LENGTHS, rec, words, read_lengths, None, out, len(want)) == (0, len(want)) and out.tobytes() == R.signature_array(want).tobytes()
    shuffled = out[rng.permutation(len(out))]
    assert F.sv_clusters_host(shuffled).tobytes() == F.sv_clusters_host(out).tobytes() == R.cluster_array(R.clusters(want, R.options())).tobytes()
    # the capacity: one slot too few carries the need and leaves the buffer alone
    out[:] = 0
    rc, need = _host(LENGTHS, rec, words, read_lengths, None, out[:-1], len(want) - 1)
    assert rc == -3 and need == len(want) and not out.tobytes().strip(b"\0") and "too small" in capi.lib().flx_last_error().decode()
    n = C.c_uint64(0)
    sig = R.signature_array(want)
    rc = capi.lib().flx_sv_clusters_host(None, sig.ctypes.data_as(C.POINTER(capi.SvSignature)), len(sig), None, C.byref(n))
    assert rc == -3 and n.value == len(R.clusters(want, R.options())) > 0


def test_every_refusal_leaves_the_output_untouched():
    good = [(0, 1, 10, 0, 60, [W("=", 20), W("D", 60), W("=", 40)]), (16, 0, 0, 1, 60, [W("S", 3), W("I", 55), W("=", 2)])]
    good_lengths = [60, 60]

    def refused(rows, match, lengths=LENGTHS, opt=None, words_cut=0, read_lengths=None, fix=None, n_refs=None):
        rec, words = R.records_of(good + rows)
        if fix:
            fix(rec)
        rl = good_lengths + (read_lengths if read_lengths is not None else [R.query_rows(r[5]) for r in rows])
        out = np.full(8, 7, dtype=F.SV_SIGNATURE_DTYPE)
        rc, n = _host(lengths, rec, words[: len(words) - words_cut], rl, opt, out, 8, n_refs)
        assert rc == -1 and n == 8 and (out == np.full(8, 7, dtype=F.SV_SIGNATURE_DTYPE)).all(), rows
        assert match in capi.lib().flx_last_error().decode(), capi.lib().flx_last_error()

    # everything coverage refuses
    refused([(0, 1, 0, 2, 60, [])], "no CIGAR words", read_lengths=[5])                      # a run made with without_cigar
    for op in "MNHP":
        refused([(0, 1, 0, 2, 60, [W(op, 3)])], "other than")
    refused([(0, 1, 0, 2, 60, [W("=", 3), W("I", 0)])], "length 0")
    refused([(0, 4, 0, 2, 60, [W("=", 3)])], "reference_id")
    refused([(0, -1, 0, 2, 60, [W("=", 3)])], "reference_id")
    refused([(0, 0, 1000, 2, 60, [W("=", 5)])], "behind its sequence")
    refused([(0, 0, 900, 2, 60, [W("=", 60), W("I", 9), W("D", 41)])], "behind its sequence")
    refused([(0, 3, -1, 2, 60, [W("=", 5)])], "negative")
    refused([(0, 1, 0, 2, 60, [W("=", 3)])], "outside the pool", words_cut=1)
    refused([], "2^31", lengths=[50, 1 << 31])
    refused([], "empty", lengths=[50, 0])
    # its own; 2^30 sequences are refused by their count alone, ahead of the lengths: nothing is read of an array that short
    refused([], "2^30 sequences", n_refs=1 << 30)
    refused([], "2^30 sequences", n_refs=(1 << 32) - 1)
    row = [(0, 1, 0, 2, 60, [W("S", 2), W("=", 3), W("I", 1), W("X", 2)])]

    def read_index(rec):
        rec[-1]["read"] = 3

    refused(row, "read_index", fix=read_index)
    refused(row, "sum to 8, its read has 9", read_lengths=[9])
    refused(row, "sum to 8, its read has 7", read_lengths=[7])
    refused([(0, 1, 0, 2, 60, [W("S", 4), W("I", 3), W("S", 1)])], "no reference-consuming column")
    refused([(0, 1, 0, 2, 60, [W("I", 3)])], "no reference-consuming column")
    refused([(0, 1, 0, 2, 60, [W("=", 4), W("S", 3), W("=", 1)])], "S word with other words on both sides")
    refused([(0, 1, 0, 2, 60, [W("S", 1), W("=", 4), W("S", 3), W("I", 1), W("=", 1), W("S", 2)])], "S word with other words on both sides")
    refused([(2048 if k else 0, 1, 10 * k, 2, 60, [W("=", 5)]) for k in range(65)], "more than 64", read_lengths=[5])
    bad = capi.SvOptions()
    bad.reserved[1] = 1
    refused([], "reserved", opt=bad)
    n = C.c_uint64(0)
    assert capi.lib().flx_sv_clusters_host(C.byref(bad), None, 0, None, C.byref(n)) == -1 and "reserved" in capi.lib().flx_last_error().decode()
    sig = R.signature_array([(3, 0, 0, 0, 0, 1, 1)])
    assert capi.lib().flx_sv_clusters_host(None, sig.ctypes.data_as(C.POINTER(capi.SvSignature)), 1, None, C.byref(n)) == -1
    # the same words are fine where the record does not count; a span that ends exactly at its sequence's end is fine
    rows = good + [(4, -1, 0, 2, 0, []), (256, 9, 0, 2, 0, [W("M", 3)]), (0, 3, 0, 10 ** 6, 2, [W("I", 1)]), (2048, 0, 940, 2, 60, [W("S", 9), W("=", 60)])]
    rec, words = R.records_of(rows)
    o = R.options(min_mapq=3)
    got = F.sv_host(LENGTHS, rec, words, good_lengths + [69], R.c_options(o))
    assert R.signature_tuples(got) == R.signatures(rec, words, good_lengths + [69], o) == [(R.DEL, 0, 0, 1, 1, 30, 60), (R.INS, 0, 0, 0, 0, 0, 55)]


def test_lengths_anchors_and_positions():
    # len = min_length - 1 and len = min_length, at the default and at a set threshold
    assert _sigs([(0, 1, 100, 0, 0, [W("=", 10), W("D", 49), W("=", 10), W("D", 50), W("=", 10), W("I", 49), W("=", 5), W("I", 50), W("=", 5)])], [139]) == \
        [(R.DEL, 0, 0, 1, 1, 169, 50), (R.INS, 0, 0, 1, 1, 233, 50)]
    assert _sigs([(0, 1, 100, 0, 0, [W("=", 10), W("D", 6), W("=", 10), W("D", 7), W("=", 10), W("I", 6), W("=", 5), W("I", 7), W("=", 5)])], [53], R.options(min_length=7)) == \
        [(R.DEL, 0, 0, 1, 1, 126, 7), (R.INS, 0, 0, 1, 1, 147, 7)]
    # the anchor of an I: as the first word, directly behind a leading S, behind a D, and as the last word in front of a trailing S
    assert _sigs([(0, 2, 500, 0, 0, [W("I", 60), W("=", 10)])], [70]) == [(R.INS, 0, 0, 2, 2, 500, 60)]
    assert _sigs([(16, 2, 500, 0, 0, [W("S", 5), W("I", 60), W("=", 10)])], [75]) == [(R.INS, 0, 0, 2, 2, 500, 60)]
    assert _sigs([(0, 2, 500, 0, 0, [W("=", 4), W("D", 3), W("I", 60), W("=", 10)])], [74]) == [(R.INS, 0, 0, 2, 2, 506, 60)]
    assert _sigs([(0, 2, 500, 0, 0, [W("D", 3), W("I", 60), W("=", 10)])], [70]) == [(R.INS, 0, 0, 2, 2, 502, 60)]
    assert _sigs([(0, 2, 500, 0, 0, [W("=", 10), W("I", 60), W("S", 7)])], [77]) == [(R.INS, 0, 0, 2, 2, 509, 60)]
    # a D as the first and as the last reference word, ending on the sequence's last position
    assert _sigs([(0, 0, 0, 0, 0, [W("D", 50), W("=", 10)]), (0, 0, 940, 1, 0, [W("=", 5), W("I", 2), W("D", 55), W("S", 3)])], [10, 10]) == \
        [(R.DEL, 0, 0, 0, 0, 0, 50), (R.DEL, 0, 0, 0, 0, 945, 55)]
    # large coordinates: a sequence of 2^31 - 1 symbols with events at its far end
    big = (1 << 31) - 1
    lengths = [1000, big]
    far = big - 1100
    rows = [(0, 1, far, 0, 0, [W("=", 100), W("D", 900), W("=", 40), W("I", 70), W("=", 60)]),
            (2048, 1, 5, 0, 0, [W("S", 100), W("=", 170)]), (2064, 1, big - 170, 0, 0, [W("=", 170), W("S", 100)])]
    want = _sigs(rows, [270], lengths=lengths)
    assert (R.DEL, 0, 0, 1, 1, far + 100, 900) in want and (R.INS, 0, 0, 1, 1, far + 1039, 70) in want and far + 1039 >= 1 << 30 and big - 1 >= 1 << 30
    assert (R.BND, R.L, R.R, 1, 1, 5, big - 1) in want and len(want) == 4
    cl = _clusters(want * 2)
    assert (R.BND, R.L, R.R, 2, 1, 1, 5, 5, big - 1, big - 1, big - 1) in cl


def _pair(flag_a, flag_b, a=(0, 100), b=(1, 700), n=40):
    """two records of one read of 2n letters, n matching columns each: the first half of the oriented read at a, the second at b"""
    rows = []
    for flag, (ref, pos), first in ((flag_a, a, True), (flag_b, b, False)):
        lead = (flag & 16 == 0) != first                                   # a forward record of the first half carries its clip behind
        rows.append((flag, ref, pos, 0, 0, [W("S", n), W("=", n)] if lead else [W("=", n), W("S", n)]))
    return rows


def test_junction_orientations_and_ordering():
    n = 40
    # all four strand pairs; the ends as the rule has them
    assert _sigs(_pair(0, 2048), [80]) == [(R.BND, R.R, R.L, 0, 1, 139, 700)]
    assert _sigs(_pair(0, 2064), [80]) == [(R.BND, R.R, R.R, 0, 1, 139, 739)]
    assert _sigs(_pair(16, 2048), [80]) == [(R.BND, R.L, R.L, 0, 1, 100, 700)]
    assert _sigs(_pair(16, 2064), [80]) == [(R.BND, R.L, R.R, 0, 1, 100, 739)]
    # both outcomes of the canonicalisation: by ref, by pos, by side
    assert _sigs(_pair(0, 2048, a=(1, 700), b=(0, 100)), [80]) == [(R.BND, R.L, R.R, 0, 1, 100, 739)]
    assert _sigs(_pair(0, 2048, a=(1, 700), b=(1, 100)), [80]) == [(R.BND, R.L, R.R, 1, 1, 100, 739)]
    assert _sigs(_pair(0, 2048, a=(1, 100), b=(1, 700)), [80]) == [(R.BND, R.R, R.L, 1, 1, 139, 700)]
    assert _sigs(_pair(16, 2064, a=(1, 139), b=(1, 100)), [80]) == [(R.BND, R.L, R.R, 1, 1, 139, 139)]
    assert _sigs(_pair(0, 2048, a=(1, 100), b=(1, 139)), [80]) == [(R.BND, R.L, R.R, 1, 1, 139, 139)]
    # a read and its reverse complement: records reversed, strands flipped, clips mirrored
    rng = np.random.default_rng(3)
    for _ in range(50):
        m = int(rng.integers(2, 6))
        cuts = sorted(rng.choice(np.arange(1, 400), size=m - 1, replace=False).tolist())
        bounds = [0] + cuts + [400]
        fwd, rev = [], []
        for k in range(m):
            q0, q1 = bounds[k], bounds[k + 1]
            strand, ref, pos = int(rng.integers(0, 2)), int(rng.integers(0, 4)), int(rng.integers(0, 500))
            body = [W("=", q1 - q0)]

            def clipped(front, back):
                return ([W("S", front)] if front else []) + body + ([W("S", back)] if back else [])

            # on the read as given the interval is [q0, q1); a reverse record's words run over the reverse complement. The molecule's
            # other strand has the same words at the same place (the oriented sequence is the same) and the other flag
            ws = clipped(400 - q1, q0) if strand else clipped(q0, 400 - q1)
            fwd.append((16 * strand + (2048 if k else 0), ref, pos, 0, 0, ws))
            rev.append((16 * (1 - strand) + (2048 if k else 0), ref, pos, 0, 0, ws))
        assert _sigs(fwd, [400]) == _sigs(rev[::-1], [400]) == _sigs(rev, [400])
        assert len(_sigs(fwd, [400])) == m - 1
    # groups of 1, 2, 3 and 64 members
    def group(m, read=0):
        return [(2048 if k else 0, 1, 20 * k, read, 0, ([W("S", 5 * k)] if k else []) + [W("=", 5)] + ([W("S", 5 * (m - 1 - k))] if k < m - 1 else [])) for k in range(m)]

    for m in (1, 2, 3, 64):
        want = _sigs(group(m), [5 * m])
        assert want == sorted((R.BND, R.R, R.L, 1, 1, 20 * k + 4, 20 * k + 20) for k in range(m - 1))
    # neighbouring groups of the same read index apart: a run is cut where the read changes, and the same read further on is another group
    rows = group(2, 0) + group(3, 1) + group(2, 0)
    assert len(_sigs(rows, [10, 15])) == 1 + 2 + 1
    # a secondary, an unmapped record and a record below min_mapq inside a group are skipped without breaking the chain
    rows = [(0, 1, 0, 0, 9, [W("=", 5), W("S", 10)]), (256, 2, 50, 0, 9, [W("S", 2), W("=", 13)]), (4, -1, 0, 0, 0, []), (2048, 1, 100, 0, 1, [W("S", 3), W("=", 12)]),
            (2064, 3, 200, 0, 9, [W("=", 10), W("S", 5)])]
    for sec in (False, True):
        assert _sigs(rows, [15], R.options(min_mapq=5, count_secondary=sec)) == [(R.BND, R.R, R.R, 1, 3, 4, 209)]
    assert _sigs(rows, [15], R.options(count_secondary=True)) == [(R.BND, R.R, R.L, 1, 1, 4, 100), (R.BND, R.R, R.R, 1, 3, 111, 209)]
    # equal query_start values are ordered by index
    rows = [(0, 1, 300, 0, 0, [W("S", 5), W("=", 10)]), (2048, 1, 100, 0, 0, [W("S", 5), W("=", 10)]), (2048, 1, 200, 0, 0, [W("=", 15)])]
    assert _sigs(rows, [15]) == [(R.BND, R.L, R.R, 1, 1, 100, 309), (R.BND, R.R, R.L, 1, 1, 214, 300)]


def test_cluster_boundaries():
    def dels(pairs, ref=1):
        return [(R.DEL, 0, 0, ref, ref, p, q) for p, q in pairs]

    one = R.options(min_support=1)
    # gaps of exactly max_distance join, max_distance + 1 breaks: in pos_a and in q
    assert [c[3] for c in _clusters(dels([(100, 300), (200, 300)]), one)] == [2]
    assert [c[3] for c in _clusters(dels([(100, 300), (201, 300)]), one)] == [1, 1]
    assert [c[3] for c in _clusters(dels([(100, 300), (100, 400)]), one)] == [2]
    assert [c[3] for c in _clusters(dels([(100, 300), (100, 401)]), one)] == [1, 1]
    o7 = R.options(min_support=1, max_distance=7)
    assert [c[3] for c in _clusters(dels([(100, 300), (107, 293), (114, 300)]), o7)] == [3]
    assert [c[3] for c in _clusters(dels([(100, 300), (108, 300)]), o7)] == [1, 1]
    assert [c[3] for c in _clusters(dels([(100, 300), (100, 308)]), o7)] == [1, 1]
    # single linkage: a chain spans more than max_distance end to end
    chain = _clusters(dels([(100 + 7 * k, 300 + 7 * k) for k in range(10)]), o7)
    assert chain == [(R.DEL, 0, 0, 10, 1, 1, 100, 163, 300, 328, 363)]
    # the interleave case: A and C meet although B lies between them in position order
    assert _clusters(dels([(100, 300), (101, 5000), (102, 300)]), one) == [(R.DEL, 0, 0, 2, 1, 1, 100, 102, 300, 300, 300), (R.DEL, 0, 0, 1, 1, 1, 101, 101, 5000, 5000, 5000)]
    # another class breaks a group: type, reference, side
    sigs = dels([(100, 300)]) + dels([(100, 300)], ref=2) + [(R.INS, 0, 0, 1, 1, 100, 300), (R.BND, 0, 1, 1, 1, 100, 300), (R.BND, 1, 1, 1, 1, 100, 300), (R.BND, 0, 1, 1, 2, 100, 300)]
    assert [c[3] for c in _clusters(sigs, one)] == [1] * 6
    # min_support 1, 2 and 3 (2 is the default), n = 0 and n = 1, identical signatures
    sigs = dels([(100, 300)] * 3 + [(900, 60)] * 2 + [(2000, 70)])
    assert [c[3] for c in _clusters(sigs, one)] == [3, 2, 1]
    assert [c[3] for c in _clusters(sigs)] == [3, 2] == [c[3] for c in _clusters(sigs, R.options(min_support=2))]
    assert [c[3] for c in _clusters(sigs, R.options(min_support=3))] == [3]
    assert _clusters([]) == [] and _clusters([], one) == []
    assert _clusters(dels([(5, 50)])) == [] and _clusters(dels([(5, 50)]), one) == [(R.DEL, 0, 0, 1, 1, 1, 5, 5, 50, 50, 50)]
    assert _clusters(dels([(5, 50)] * 4)) == [(R.DEL, 0, 0, 4, 1, 1, 5, 5, 50, 50, 50)]
    # the median is member (support - 1) / 2 in (q, pos_a) order; the bounds of pos_a come from any member
    assert _clusters(dels([(130, 50), (100, 60), (120, 70), (110, 80)])) == [(R.DEL, 0, 0, 4, 1, 1, 100, 130, 50, 60, 80)]
    assert _clusters(dels([(130, 50), (100, 60), (120, 70)])) == [(R.DEL, 0, 0, 3, 1, 1, 100, 130, 50, 60, 70)]


def test_rule_header_against_a_word_by_word_definition_under_sanitizers(tmp_path):
    """tests/sv_check.cpp: flx_sv.hpp on random records, built with ASan + UBSan; nothing is preloaded"""
    exe = str(tmp_path / "sv_check")
    src = os.path.join(ROOT, "tests", "sv_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


def test_cli_sv_flags(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    base = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"),
            "--output", str(tmp_path / "o.sam"), "-e", "2"]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0
    lines = h.stderr.decode().splitlines()
    for flag in ("--sv-signatures", "--sv-min-length", "--sv-max-distance", "--sv-min-support", "--sv-secondary", "--sv-min-mapq"):
        line = [l for l in lines if re.search(rf"^\s+{flag}(\s|$)", l)]
        assert len(line) == 1 and line[0].startswith("      " + flag) and "not floxer's" in line[0], flag      # long spellings only
    for flag in ("--sv-min-length", "--sv-max-distance", "--sv-min-support"):
        assert "convention" in [l for l in lines if re.search(rf"^\s+{flag}\s", l)][0], flag
    assert "1-based" in [l for l in lines if re.search(r"^\s+--sv-signatures\s", l)][0]
    env = dict(os.environ, FLX_CLI_PARSE_ONLY="1")                       # the parser alone: no device is touched
    tsv, bg = str(tmp_path / "sv.tsv"), str(tmp_path / "d.bedgraph")
    for extra in (["--sv-signatures", tsv], ["--sv-signatures", tsv, "--sv-min-length", "1", "--sv-max-distance", "1", "--sv-min-support", "1"],
                  ["--sv-signatures", tsv, "--sv-secondary", "--sv-min-mapq", "254", "-Q", "-D", "-N", "1"],
                  ["--sv-signatures", tsv, "--coverage", bg, "--pileup", str(tmp_path / "p.tsv"), "--left-align-indels"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and r.stdout == b"" and b"CLI PARSER ERROR" not in r.stderr, (extra, r.stderr)
    for extra in (["--sv-signatures", tsv, "-w"], ["--without-cigar", "--sv-signatures", tsv],
                  ["--sv-signatures", tsv, "--sv-min-mapq", "1"],                                       # without -Q
                  ["--sv-min-length", "60"], ["--sv-max-distance", "3"], ["--sv-min-support", "3"], ["--sv-secondary"],
                  ["--sv-min-mapq", "1", "-Q"],                                                         # no output
                  ["--sv-signatures", str(tmp_path / "sv.txt")], ["--sv-signatures", bg], ["--sv-signatures", str(tmp_path / "sv")],
                  ["--sv-signatures", tsv, "-Q", "--sv-min-mapq", "0"], ["--sv-signatures", tsv, "-Q", "--sv-min-mapq", "255"],
                  ["--sv-signatures", tsv, "--sv-min-length", "0"], ["--sv-signatures", tsv, "--sv-max-distance", "0"],
                  ["--sv-signatures", tsv, "--sv-min-support", "0"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr and b"sv" in r.stderr, (extra, r.stderr)
    assert not any(os.path.exists(p) for p in (tsv, bg))
