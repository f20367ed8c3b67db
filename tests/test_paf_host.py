"""PAF summaries and the PAF writer without a GPU (flx_paf_summarize_host, flx_paf on device -1, flx_paf_open / write / close, the CLI's
option checks): the library's host rule against tests/paf_ref.py on crafted and random records, every refusal of the rule, the writer's
bytes for records of every kind under every option, the CLI's parser errors, and tests/paf_check.cpp: the rule header under ASan + UBSan
against a column-by-column definition. All comparisons are exact."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import paf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LENS = [50, 3000, 977, 64, 1500]
REF_IDS = ["chrA", "chrB", "c", "chrD.1", "e"]
W = R.word


def _both(rec, words, read_lengths, ref_lens=REF_LENS):
    """the host call's and the device -1 object's summaries, equal to each other"""
    a = F.paf_summarize_host(rec, words, read_lengths, ref_lens)
    p = F.paf(device=-1)
    b = p.summarize(rec, words, read_lengths, ref_lens)
    p.close()
    assert a.tobytes() == b.tobytes()
    return a


def test_crafted_records_equal_the_reference():
    rows = [
        (0, 1, 100, 0, 3, [W("S", 3), W("=", 20), W("X", 1), W("I", 2), W("=", 5), W("S", 11)]),      # unequal clips, forward
        (16, 1, 100, 0, 3, [W("S", 3), W("=", 20), W("X", 1), W("I", 2), W("=", 5), W("S", 11)]),     # the same words, reverse
        (2064, 2, 7, 1, 0, [W("S", 9), W("=", 30)]),                                                # a lead only, reverse
        (2048, 2, 7, 1, 0, [W("=", 30), W("S", 9)]),                                                # a trail only
        (0, 0, 49, 2, 0, [W("=", 1)]),                                                              # one = word, on the last base
        (256, 3, 0, 3, 6, [W("I", 4), W("=", 10), W("D", 2)]),                                       # I as first word
        (0, 4, 10, 4, 5, [W("=", 5), W("D", 2), W("D", 3), W("=", 5)]),                              # D D: one gap open
        (272, 4, 10, 5, 4, [W("=", 5), W("I", 1), W("D", 2), W("I", 1), W("=", 5)]),                 # I D I: three
        (4, -1, 0, 6, 0, []),
        (0, -1, 0, 6, 0, [W("M", 9)]),                                                              # reference_id < 0: zeros, not judged
    ]
    rec, words = R.records_of(rows)
    read_lengths = [42, 39, 1, 14, 10, 12, 77]
    got = _both(rec, words, read_lengths)
    assert got.tobytes() == R.summarize(rec, words, read_lengths, REF_LENS).tobytes()
    assert tuple(got[0]) == (3, 31, 126, 25, 1, 2, 0, 1) and tuple(got[1]) == (11, 39, 126, 25, 1, 2, 0, 1)      # a wrong flip shows
    assert tuple(got[2]) == (0, 30, 37, 30, 0, 0, 0, 0) and tuple(got[3]) == (0, 30, 37, 30, 0, 0, 0, 0)
    assert tuple(got[4]) == (0, 1, 50, 1, 0, 0, 0, 0)
    assert got["gap_opens"].tolist() == [1, 1, 0, 0, 0, 2, 1, 3, 0, 0] and not any(got[8]) and not any(got[9])
    # records that share words, and an out buffer that is filled in place
    rec2 = np.concatenate([rec, rec])
    out = np.zeros(len(rec2), dtype=F.PAF_SUMMARY_DTYPE)
    assert F.paf_summarize_host(rec2, words, read_lengths, REF_LENS, out=out) is not None
    assert out.tobytes() == got.tobytes() * 2
    assert len(_both(rec[:0], words, read_lengths)) == 0                  # no record: fine
    # neighbours that share one CIGAR array and differ in strand and position (the words are walked once for them)
    rec3 = np.repeat(rec, 3)
    rec3["flag"][1::3] ^= 16
    rec3["pos"][2::3] = np.where(rec3["ref"][2::3] >= 0, 0, rec3["pos"][2::3])
    assert _both(rec3, words, read_lengths).tobytes() == R.summarize(rec3, words, read_lengths, REF_LENS).tobytes()


def test_a_call_large_enough_for_several_judging_threads():
    rng = np.random.default_rng(8)
    ws = [W("=XID"[(i + int(i % 7 == 0)) % 4] if i % 2 else "=", 1 + i % 3) for i in range(1000)]
    rows = [((0, 16, 256, 2048)[i % 4], 1, int(rng.integers(0, 100)), 0, 0, ws) for i in range(40)]
    rec, words = R.records_of(rows)
    read_lengths = [sum(int(w) >> 4 for w in ws if int(w) & 15 in (7, 8, 1))]
    rec = np.repeat(rec, 120)                                            # 4800 records, 4.8 M words in all: the call is judged in pieces
    want = R.summarize(rec[:40 * 120:120], words, read_lengths, REF_LENS)
    got = _both(rec, words, read_lengths)
    assert got.tobytes() == np.repeat(want, 120).tobytes()
    bad = rec.copy()
    bad["pos"][[3100, 4700]] = 2999
    bad["ref"][4000] = 9
    out = np.zeros(len(bad), dtype=F.PAF_SUMMARY_DTYPE)
    with pytest.raises(capi.FloxerError, match="record 3100 ends behind its sequence"):          # the first refusal in record order
        F.paf_summarize_host(bad, words, read_lengths, REF_LENS, out=out)
    assert not out.view(np.uint32).any()


def test_random_valid_records_equal_the_reference():
    rng = np.random.default_rng(91)
    rec, words, read_lengths = R.random_valid(rng, REF_LENS, 3500)
    want = R.summarize(rec, words, read_lengths, REF_LENS)                # (raises on a record the generator got wrong)
    assert {int(f) for f in rec["flag"]} == set(R.FLAGS)
    mapped = np.array([R.mapped(r) for r in rec])
    assert int(mapped.sum()) == 3000 and (want["ref_end"][mapped] > 0).all()          # none was skipped
    assert (want["gap_opens"] > 1).any() and (want["query_start"] > 0).any()
    assert _both(rec, words, read_lengths).tobytes() == want.tobytes()


def _call_host(rec, words, read_lengths, ref_lens, out, n_words=None):
    offs = F._read_offsets(read_lengths)
    lens = np.asarray(ref_lens, dtype=np.uint64)
    return capi.lib().flx_paf_summarize_host(rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), capi.ptr(words, capi.u32p), len(words) if n_words is None else n_words,
                                             capi.ptr(offs, capi.u64p), len(offs) - 1, capi.ptr(lens, capi.u64p), len(lens), out.ctypes.data_as(C.POINTER(capi.PafSummary)))


def test_every_refusal_leaves_the_output_untouched():
    good = [(0, 1, 10, 0, 1, [W("=", 20), W("X", 1), W("=", 5)]), (16, 0, 0, 1, 2, [W("S", 3), W("I", 2), W("=", 50)])]
    good_lens = [26, 55]
    handle = F.paf(device=-1)

    def refused(row, read_len, match, reason, ref_lens=REF_LENS, words_cut=0, read_index=None):
        rec, words = R.records_of(good + [row])
        read_lengths = good_lens + [read_len]
        if read_index is not None:
            rec[-1]["read"] = read_index
        with pytest.raises(R.Refused, match=re.escape(reason)):
            for r in rec:
                R.summary(r, words, read_lengths, ref_lens, n_words=len(words) - words_cut)
        out = np.full(3, 0x5A5A5A5A, dtype=np.uint32).repeat(8).view(F.PAF_SUMMARY_DTYPE)
        before = out.tobytes()
        assert _call_host(rec, words, read_lengths, ref_lens, out, n_words=len(words) - words_cut) == -1 and out.tobytes() == before, row
        assert match in capi.lib().flx_last_error().decode(), capi.lib().flx_last_error()
        with pytest.raises(capi.FloxerError, match=re.escape(match)):
            handle.summarize(rec, words[: len(words) - words_cut] if words_cut else words, read_lengths, ref_lens, out=out)
        assert out.tobytes() == before

    refused((0, 1, 0, 2, 0, []), 5, "no CIGAR words", "no words")
    for op in "MNHP":
        refused((0, 1, 0, 2, 0, [W(op, 3)]), 3, "other than", "op")
    refused((0, 1, 0, 2, 0, [W("=", 3), W("I", 0)]), 3, "length 0", "zero length")
    refused((0, 5, 0, 2, 0, [W("=", 3)]), 3, "reference_id", "reference_id")
    refused((0, 1, -1, 2, 0, [W("=", 3)]), 3, "negative", "negative position")
    refused((0, 3, 62, 2, 0, [W("=", 3)]), 3, "behind its sequence", "behind its sequence")
    refused((0, 3, 0, 2, 0, [W("=", 60), W("I", 9), W("D", 5)]), 69, "behind its sequence", "behind its sequence")
    refused((0, 1, 0, 2, 0, [W("=", 3)]), 3, "outside the pool", "words outside the pool", words_cut=1)
    refused((0, 1, 0, 2, 0, [W("=", 3), W("S", 2), W("=", 3)]), 8, "both sides", "interior clip")
    refused((0, 1, 0, 2, 0, [W("S", 1), W("X", 3), W("S", 2), W("D", 3), W("S", 2)]), 8, "both sides", "interior clip")
    refused((0, 1, 0, 2, 0, [W("=", 3)]), 3, "read_index", "read_index", read_index=3)
    row = (0, 1, 0, 2, 0, [W("S", 2), W("=", 3), W("I", 1), W("X", 2)])
    refused(row, 9, "sum to 8, its read has 9", "read length")
    refused(row, 7, "sum to 8, its read has 7", "read length")
    refused((0, 1, 0, 2, 0, [W("S", 4), W("I", 3), W("S", 1)]), 8, "no reference-consuming column", "no reference-consuming column")
    refused((0, 1, 0, 2, 0, [W("S", 4)]), 4, "no reference-consuming column", "no reference-consuming column")
    big = [W("I", (1 << 28) - 1)] * 9 + [W("=", 1)]
    refused((0, 1, 0, 2, 0, big), 9 * ((1 << 28) - 1) + 1, "2^31", "2^31")
    # the bound itself: query-consuming lengths of exactly 2^31 are refused, 2^31 - 1 (below) are summarised
    at_limit = [W("I", (1 << 28) - 1)] * 8 + [W("=", 8)]
    assert sum(w >> 4 for w in at_limit) == 1 << 31
    refused((0, 1, 0, 2, 0, at_limit), 1 << 31, "2^31", "2^31")
    handle.close()
    # what is fine: a span that ends exactly at its sequence's end, a D-only record, the same bad words in an unmapped record
    rec, words = R.records_of(good + [(0, 3, 4, 2, 0, [W("S", 9), W("=", 60)]), (0, 3, 0, 3, 4, [W("D", 4)]), (4, 0, 0, 9, 0, [W("M", 3)])])
    read_lengths = good_lens + [69, 0]
    assert _both(rec, words, read_lengths).tobytes() == R.summarize(rec, words, read_lengths, REF_LENS).tobytes()
    # one row below the bound: 2^31 - 1 query-consuming lengths (no letters are read: the read is its length alone)
    below = [W("I", (1 << 28) - 1)] * 8 + [W("=", 7)]
    rec, words = R.records_of(good + [(0, 1, 0, 2, 0, below)])
    read_lengths = good_lens + [(1 << 31) - 1]
    got = _both(rec, words, read_lengths)
    assert got.tobytes() == R.summarize(rec, words, read_lengths, REF_LENS).tobytes() and int(got[2]["query_end"]) == (1 << 31) - 1
    # the lengths themselves, and a null output
    out = np.zeros(5, dtype=F.PAF_SUMMARY_DTYPE)
    assert _call_host(rec, words, read_lengths, [50, 1 << 31], out) == -1 and "2^31" in capi.lib().flx_last_error().decode()
    assert _call_host(rec, words, read_lengths, [50, 0], out) == -1 and "empty" in capi.lib().flx_last_error().decode()


def test_symbols_sizes_and_python_names():
    L = capi.lib()
    names = [n for n in capi.EXPORTED if n.startswith("flx_paf_")]
    assert sorted(names) == sorted(["flx_paf_create", "flx_paf_free", "flx_paf_summarize", "flx_paf_summarize_host", "flx_paf_open", "flx_paf_write", "flx_paf_close"])
    for name in names:
        getattr(L, name)
    assert C.sizeof(capi.PafSummary) == 32 and C.sizeof(capi.PafOptions) == 32 and F.PAF_SUMMARY_DTYPE.itemsize == 32
    assert list(F.PAF_SUMMARY_DTYPE.names) == ["query_start", "query_end", "ref_end", "matches", "mismatches", "ins_bases", "del_bases", "gap_opens"]
    assert [F.PAF_SUMMARY_DTYPE.fields[k][1] for k in F.PAF_SUMMARY_DTYPE.names] == list(range(0, 32, 4))
    header = open(os.path.join(ROOT, "include", "floxer_amd.h")).read()
    assert set(re.findall(r"\b(flx_[a-z0-9_]+)\s*\(", header)) == set(capi.EXPORTED)
    o = F.paf_options(write_cigar=True, skip_secondary=True)
    assert (o.write_cigar, o.write_unmapped, o.mapq_from_records, o.skip_secondary, list(o.reserved)) == (1, 0, 0, 1, [0] * 4)
    # options are judged at open: reserved fields, switches above 1
    ids = (C.c_char_p * 1)(b"r")
    lens = np.array([5], dtype=np.uint64)
    for field, value in (("reserved", None), ("write_cigar", 2), ("skip_secondary", 7)):
        bad = capi.PafOptions()
        if value is None:
            bad.reserved[3] = 1
        else:
            setattr(bad, field, value)
        h = C.c_void_p()
        assert L.flx_paf_open(b"/nonexistent-dir/x.paf", ids, capi.ptr(lens, capi.u64p), 1, C.byref(bad), C.byref(h)) == -1 and not h
    h = C.c_void_p()
    assert L.flx_paf_open(b"/nonexistent-dir/x.paf", ids, capi.ptr(lens, capi.u64p), 1, None, C.byref(h)) == -6 and not h


# ------------------------------------------------------------------------------------------------ the writer
def _writer_batch():
    """records of every kind over four reads, with scores and cs strings"""
    rows = [
        (0, 1, 100, 0, 3, [W("S", 3), W("=", 20), W("X", 1), W("I", 2), W("=", 5), W("S", 11)], 60),
        (256, 2, 5, 0, 0, [W("=", 42)], 0),
        (272, 4, 10, 0, 4, [W("=", 5), W("I", 1), W("D", 2), W("I", 1), W("=", 35)], 3),
        (16, 0, 0, 1, 9, [W("X", 9)], 254),                               # den = num: de 1.0000
        (2064, 3, 1, 1, 0, [W("S", 2), W("=", 7)], 17),
        (4, -1, 0, 2, 0, [], 0),
        (2048, 1, 2000, 3, 1, [W("=", 31), W("X", 1), W("S", 8)], 1),     # 1 / 32: the fifth decimal is exactly 5
        (0, 1, 0, 3, 3, [W("=", 20), W("D", 3), W("=", 20)], 44),
    ]
    rec, words = R.records_of(rows)
    read_ids = ["read/0", "r1", "unmapped one", "r3"]
    read_lengths = [42, 9, 13, 40]
    scores = np.array([77, 84, -5, -36, 14, 0, 58, 70], dtype=np.int32)
    cs = [b":20*ag+tt:5", b":42", b":5+a-cg+t:35", b"*ac*ac*ac*ac*ac*ac*ac*ac*ac", b":7", None, b":31*tg", b":20-acg:20"]
    return rec, words, read_ids, read_lengths, scores, cs


def _cs_pool(cs):
    refs = np.zeros((len(cs), 2), dtype=np.uint64)
    pool = bytearray(b"..")                                              # (offsets need not start at 0)
    for i, s in enumerate(cs):
        if s:
            refs[i] = (len(pool), len(s))
            pool += s + b"|"
    return refs, np.frombuffer(bytes(pool), dtype=np.uint8)


def _write(path, o, rec, words, read_ids, read_lengths, summ, scores=None, cs=None, calls=1):
    w = F.paf_writer(path, REF_IDS, REF_LENS, R.c_options(o))
    refs, pool = _cs_pool(cs) if cs is not None else (None, None)
    step = (len(rec) + calls - 1) // calls
    for a in range(0, len(rec), step):
        b = min(len(rec), a + step)
        w.write(read_ids, read_lengths, rec[a:b], words, summ[a:b], None if scores is None else scores[a:b], None if refs is None else refs[a:b], pool)
    w.close()
    return open(path, "rb").read()


def test_writer_bytes_for_every_kind_under_every_option(tmp_path):
    rec, words, read_ids, read_lengths, scores, cs = _writer_batch()
    assert {int(f) for f in rec["flag"]} == set(R.FLAGS)
    summ = F.paf_summarize_host(rec, words, read_lengths, REF_LENS)
    assert summ.tobytes() == R.summarize(rec, words, read_lengths, REF_LENS).tobytes()
    seen = set()
    for k, (cg, un, mq, sk) in enumerate(itertools.product([False, True], repeat=4)):
        o = R.options(write_cigar=cg, write_unmapped=un, mapq_from_records=mq, skip_secondary=sk)
        for with_scores, with_cs in itertools.product([False, True], repeat=2):
            want = R.lines(read_ids, read_lengths, rec, words, summ, REF_IDS, REF_LENS, o, scores if with_scores else None, cs if with_cs else None)
            got = _write(str(tmp_path / f"o{k}.paf"), o, rec, words, read_ids, read_lengths, summ, scores if with_scores else None, cs if with_cs else None,
                         calls=1 + k % 3)
            assert got == want, (o, with_scores, with_cs)
            seen.add(got)
    assert len(seen) == 64                                               # every switch changes the bytes of this batch
    # the lines themselves, spelled out once
    text = R.lines(read_ids, read_lengths, rec, words, summ, REF_IDS, REF_LENS, R.options(write_cigar=True, write_unmapped=True, mapq_from_records=True), scores, cs).decode()
    ls = text.split("\n")
    assert ls[0] == "read/0\t42\t3\t31\t+\tchrB\t3000\t100\t126\t25\t28\t60\ttp:A:P\tNM:i:3\tAS:i:77\tde:f:0.0741\tcg:Z:3S20=1X2I5=11S\tcs:Z::20*ag+tt:5"
    assert ls[1] == "read/0\t42\t0\t42\t+\tc\t977\t5\t47\t42\t42\t0\ttp:A:S\tNM:i:0\tAS:i:84\tde:f:0.0000\tcg:Z:42=\tcs:Z::42"
    assert ls[3] == "r1\t9\t0\t9\t-\tchrA\t50\t0\t9\t0\t9\t254\ttp:A:P\tNM:i:9\tAS:i:-36\tde:f:1.0000\tcg:Z:9X\tcs:Z:*ac*ac*ac*ac*ac*ac*ac*ac*ac"
    assert ls[4].startswith("r1\t9\t0\t7\t-\tchrD.1\t64\t1\t8\t7\t7\t17\ttp:A:P\t")       # supplementary: P; reverse: the lead turned round
    assert ls[5] == "unmapped one\t13\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0"
    assert "\tde:f:0.0313\t" in ls[6] and ls[6].startswith("r3\t40\t0\t32\t+\t")
    assert ls[8] == "" and len(ls) == 9
    assert R.divergence(0, 5) == "0.0000" and R.divergence(5, 5) == "1.0000" and R.divergence(1, 32) == "0.0313" and R.divergence(3, 32) == "0.0938"


def test_writer_refusals_write_nothing(tmp_path):
    rec, words, read_ids, read_lengths, scores, cs = _writer_batch()
    summ = F.paf_summarize_host(rec, words, read_lengths, REF_LENS)

    def refused(path, o, rec, summ, match, cs=cs):
        w = F.paf_writer(path, REF_IDS, REF_LENS, R.c_options(o))
        refs, pool = _cs_pool(cs)
        w.write(read_ids, read_lengths, rec[:2], words, summ[:2], None, refs[:2], pool)
        with pytest.raises(capi.FloxerError, match=re.escape(match)):
            w.write(read_ids, read_lengths, rec, words, summ, None, refs, pool)
        w.close()
        assert open(path, "rb").read() == R.lines(read_ids, read_lengths, rec[:2], words, summ[:2], REF_IDS, REF_LENS, o, None, cs[:2])

    bad = rec.copy()
    bad[6]["res"] = 255
    refused(str(tmp_path / "a.paf"), R.options(mapq_from_records=True), bad, summ, "above 254")
    w = F.paf_writer(str(tmp_path / "b.paf"), REF_IDS, REF_LENS)          # without the option the column is 255 and the records' value is not read
    w.write(read_ids, read_lengths, bad, words, summ)
    w.close()
    assert open(str(tmp_path / "b.paf"), "rb").read() == R.lines(read_ids, read_lengths, bad, words, summ, REF_IDS, REF_LENS, R.options())
    ones = summ.copy()
    ones[7] = (0xFFFFFFFF,) * 8
    refused(str(tmp_path / "c.paf"), R.options(), rec, ones, "could not make")
    ones[7] = summ[7]
    ones[7]["gap_opens"] = 0xFFFFFFFF                                    # (one field alone is not the mark)
    w = F.paf_writer(str(tmp_path / "d.paf"), REF_IDS, REF_LENS)
    w.write(read_ids, read_lengths, rec, words, ones)
    w.close()
    bad_cs = list(cs)
    bad_cs[7] = b":20\tx"
    refused(str(tmp_path / "e.paf"), R.options(), rec, summ, "cs string", cs=bad_cs)
    outside = rec.copy()
    outside[7]["ref"] = len(REF_LENS)
    refused(str(tmp_path / "f.paf"), R.options(), outside, summ, "outside the references")


def test_rule_header_against_its_columns_under_sanitizers(tmp_path):
    """tests/paf_check.cpp: flx_paf.hpp on random records, built with ASan + UBSan; nothing is preloaded"""
    exe = str(tmp_path / "paf_check")
    src = os.path.join(ROOT, "tests", "paf_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


def test_cli_paf_flags(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    inputs = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"), "-e", "2"]
    base = inputs + ["--output", str(tmp_path / "o.sam")]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0
    lines = h.stderr.decode().splitlines()
    for flag in ("--paf", "--paf-cigar", "--paf-unmapped", "--paf-skip-secondary"):
        line = [l for l in lines if re.search(rf"^\s+{flag}(\s|$)", l)]
        assert len(line) == 1 and line[0].startswith("      " + flag) and "not floxer's" in line[0], flag      # long spellings only
    env = dict(os.environ, FLX_CLI_PARSE_ONLY="1")                       # the parser alone: no device is touched
    paf = str(tmp_path / "o.paf")
    for args in (base + ["--paf", paf], base + ["--paf", paf, "--paf-cigar", "--paf-unmapped", "--paf-skip-secondary"],
                 base + ["--paf", paf, "--paf-cigar", "--cs-tag", "-Q", "-D"], inputs + ["--paf", paf], inputs + ["--paf", paf, "--paf-cigar", "--realign-affine"],
                 inputs + ["--output", str(tmp_path / "o.bam"), "--paf", paf, "--sort-by-coordinate", "--bam-index"]):
        r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and r.stdout == b"" and b"CLI PARSER ERROR" not in r.stderr, (args, r.stderr)

    def error(args):
        r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and r.stderr.startswith(b"[CLI PARSER ERROR]\n"), (args, r.stderr)
        return r.stderr.decode()[len("[CLI PARSER ERROR]\n"):]

    needs = "The options --paf-cigar, --paf-unmapped and --paf-skip-secondary need --paf.\n"
    for flag in ("--paf-cigar", "--paf-unmapped", "--paf-skip-secondary"):
        assert error(base + [flag]) == needs
    with_w = "The option --paf needs the alignments' CIGARs and cannot be combined with -w/--without-cigar.\n"
    assert error(base + ["--paf", paf, "-w"]) == with_w and error(inputs + ["--without-cigar", "--paf", paf]) == with_w
    assert with_w.replace("--paf", "--pileup") == error(base + ["--pileup", str(tmp_path / "s.tsv"), "-w"])       # the wording the other options use
    sort = "The option --sort-by-coordinate writes BAM and needs an -o/--output that ends in .bam.\n"
    assert error(inputs + ["--paf", paf, "--sort-by-coordinate"]) == sort
    assert error(inputs + ["--paf", paf, "--sort-by-coordinate", "--bam-index"]) == sort
    assert error(inputs + ["--paf", paf, "--bam-index"]) == "The options --bam-index and --sort-tmp need --sort-by-coordinate.\n"
    assert error(inputs) == "Option -o/--output is required but not set.\n"                      # today's message, byte for byte
    assert error(inputs + ["--paf-cigar"]) == "Option -o/--output is required but not set.\n"
    assert "[paf]" in error(base + ["--paf", str(tmp_path / "o.txt")]) and "[bam,sam]" in error(inputs + ["--paf", paf, "--output", str(tmp_path / "o.txt")])
    assert "Missing value" in error(base + ["--paf"])
    assert not os.path.exists(paf)
