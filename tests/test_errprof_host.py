"""Error profile without a GPU (flx_errprof_host, the CLI's option checks): the plain-numpy rule of tests/errprof_ref.py against its own
column-by-column loop, the library's host rule against errprof_ref under the four filter switches, every refusal of the rule with the
table untouched, the position bins and the homopolymer bins case by case, the CLI's parser errors, and tests/errprof_check.cpp: the
rule header under ASan + UBSan against a walk of every column."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import errprof_cases as K
import errprof_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [50, 3000, 977, 64, 1500]
SWITCHES = [R.options(count_secondary=s, min_mapq=q) for s, q in itertools.product([False, True], [0, 3])]


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(47)
    text = R.random_text(rng, LENGTHS)
    rec, words = R.random_records(rng, LENGTHS, 400)
    return text, rec, words, R.fitted_reads(rng, text, LENGTHS, rec, words)


def test_reference_against_its_naive_loop(batch):
    text, rec, words, reads = batch
    assert {int(f) for f in rec["flag"]} == {0, 16, 256, 272, 2048, 2064, 4} and set(np.unique(text)) == set(range(6))
    seen = set()
    for o in SWITCHES:
        t = R.table(text, LENGTHS, rec, words, reads, o)
        assert R.same(t, R.table_naive(text, LENGTHS, rec, words, reads, o)) == [], o
        tot = dict(zip(R.TOTALS, (int(x) for x in t["TOTALS"])))
        assert int(t["PAIR_EQ"].sum()) == tot["matches"] == int(t["POS_MATCH"].sum()) and int(t["PAIR_X"].sum()) == tot["mismatches"] == int(t["POS_MISMATCH"].sum())
        assert int(t["INS_LETTER"].sum()) == tot["ins_bases"] == int(t["POS_INS"].sum()) and int(t["DEL_LETTER"].sum()) == tot["del_bases"]
        assert int(t["INS_LEN"].sum()) == int(t["HP_INS"].sum()) == tot["ins_events"] and int(t["DEL_LEN"].sum()) == int(t["HP_DEL"].sum()) == int(t["POS_DEL"].sum()) == tot["del_events"]
        assert int(t["IDENTITY"].sum()) == tot["records"] and int(t["POS_CLIP"].sum()) == tot["clip_bases"] > 0
        assert t["HP_INS"][0] > 0 and t["HP_INS"][33] > 0 and t["HP_INS"][1:33].sum() > 0 and t["HP_DEL"][33] > 0 and t["HP_DEL"][1:32].sum() > 0
        assert all((t[k] > 0).sum() > 30 for k in ("POS_MATCH", "POS_MISMATCH", "POS_INS", "POS_CLIP", "POS_DEL"))
        seen.add(b"".join(v.tobytes() for v in t.values()))
    assert len(seen) == 4                                                # both counting switches matter on this batch
    assert len(R.tsv(t).splitlines()) == sum(n for _, n in R.SECTIONS) + 6


def _host(text, lengths, rec, words, reads, opt, table):
    lens = np.asarray(lengths, dtype=np.uint64)
    text = np.ascontiguousarray(text, dtype=np.uint8)
    pool, offs, n = F._pool_and_offsets(reads)
    return capi.lib().flx_errprof_host(capi.ptr(text, capi.u8p), capi.ptr(lens, capi.u64p), len(lens), C.byref(opt) if opt is not None else None,
                                       rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), capi.ptr(words, capi.u32p), len(words),
                                       capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n, C.byref(table))


def test_host_rule_equals_the_reference(batch):
    text, rec, words, reads = batch
    for o in SWITCHES:
        want = R.table(text, LENGTHS, rec, words, reads, o)
        assert R.same(F.errprof_host(text, LENGTHS, rec, words, reads, R.c_options(o)), want) == [], o
    # NULL options are all zero, and the call adds to what the table holds
    want = R.table(text, LENGTHS, rec, words, reads, R.options())
    assert R.same(F.errprof_host(text, LENGTHS, rec, words, reads), want) == []
    assert R.same(F.errprof_host(text, LENGTHS, rec, words, reads, table=want), R.times(want, 2)) == []
    # records that share words and reads; a list of sequences in place of the concatenation
    rec2 = np.concatenate([rec, rec])
    seqs = np.split(text, np.cumsum(LENGTHS)[:-1])
    assert R.same(F.errprof_host(seqs, None, rec2, words, reads), R.times(want, 2)) == []


def test_every_refusal_leaves_the_table_untouched():
    rng = np.random.default_rng(5)
    text = R.random_text(rng, LENGTHS)
    good = [(0, 1, 10, 60, [R.word("=", 20), R.word("X", 1), R.word("=", 5)]), (16, 0, 0, 60, [R.word("S", 3), R.word("I", 2), R.word("=", 50)])]

    def refused(rows, lengths=LENGTHS, opt=None, words_cut=0, match=None, fix=None, txt=text):
        rec, words, reads = R.records_with_reads(rng, good + rows)
        if fix:
            fix(rec, reads)
        table = capi.ErrprofTable()
        C.memset(C.byref(table), 7, C.sizeof(table))
        rc = _host(txt, lengths, rec, words[: len(words) - words_cut], reads, opt, table)
        assert rc == -1 and bytes(table) == b"\x07" * C.sizeof(table), rows
        if match:
            assert match in capi.lib().flx_last_error().decode(), capi.lib().flx_last_error()

    # coverage's refusals
    refused([(0, 1, 0, 60, [])], match="no CIGAR words")
    for op in "MNHP":
        refused([(0, 1, 0, 60, [R.word(op, 3)])], match="other than")
    refused([(0, 1, 0, 60, [R.word("=", 3), R.word("I", 0)])], match="length 0")
    refused([(0, 5, 0, 60, [R.word("=", 3)])], match="reference_id")
    refused([(0, -1, 0, 60, [R.word("=", 3)])], match="reference_id")
    refused([(0, 3, 60, 60, [R.word("=", 5)])], match="behind its sequence")
    refused([(0, 3, 0, 60, [R.word("=", 60), R.word("I", 9), R.word("D", 5)])], match="behind its sequence")
    refused([(0, 3, -1, 60, [R.word("=", 5)])], match="negative")
    refused([(0, 1, 0, 60, [R.word("=", 3)])], words_cut=1, match="outside the pool")
    refused([], lengths=[50, 1 << 31], match="2^31")
    refused([], lengths=[50, 0], match="empty")
    # pileup's
    row = [(0, 1, 0, 60, [R.word("S", 2), R.word("=", 3), R.word("I", 1), R.word("X", 2)])]

    def read_index(rec, reads):
        rec[-1]["read"] = len(reads)

    def longer(rec, reads):
        reads[-1] = np.concatenate([reads[-1], [1]]).astype(np.uint8)

    def shorter(rec, reads):
        reads[-1] = reads[-1][:-1]

    refused(row, fix=read_index, match="read_index")
    refused(row, fix=longer, match="sum to 8, its read has 9")
    refused(row, fix=shorter, match="sum to 8, its read has 7")
    refused([(0, 1, 0, 60, [R.word("S", 4), R.word("I", 3), R.word("S", 1)])], match="no reference-consuming column")
    refused([(0, 1, 0, 60, [R.word("I", 3)])], match="no reference-consuming column")
    # its own: the text's ranks, the options, a record of 2^31 columns plus rows
    bad_text = text.copy()
    bad_text[sum(LENGTHS) - 1] = 6
    refused([], txt=bad_text, match="rank above 5")
    bad = capi.ErrprofOptions()
    bad.reserved[4] = 1
    refused([], opt=bad, match="reserved")
    refused([], opt=F.errprof_options(flush_threshold=(1 << 31) + 1), match="flush_threshold")
    assert not hasattr(F.errprof_options(), "count_deletions")


def test_a_record_of_two_to_the_31_columns_and_rows_is_refused():
    """eight S words of 2^28 - 1 rows and an = word of 4: 2^31 - 4 rows plus 4 columns are exactly 2^31. The judgement asks for the read's
    length alone and refuses before a letter is read, so the offsets may name a read that long over a small pool."""
    lens = np.array([4], dtype=np.uint64)
    text = np.ones(4, dtype=np.uint8)
    pool = np.ones(16, dtype=np.uint8)
    offs = np.array([0, 8 * ((1 << 28) - 1) + 4], dtype=np.uint64)
    rec, words = R.records_of([(0, 0, 0, 0, [R.word("S", (1 << 28) - 1)] * 8 + [R.word("=", 4)])])
    table = capi.ErrprofTable()
    L = capi.lib()
    rc = L.flx_errprof_host(capi.ptr(text, capi.u8p), capi.ptr(lens, capi.u64p), 1, None, rec.ctypes.data_as(C.POINTER(capi.Record)), 1, capi.ptr(words, capi.u32p),
                            len(words), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), 1, C.byref(table))
    assert rc == -1 and "2^31 or more" in L.flx_last_error().decode() and bytes(table) == bytes(C.sizeof(table))


@pytest.mark.parametrize("length", K.POSITION_LENGTHS)
def test_position_bins(length):
    text, lengths, rec, words, reads = K.position_case(length)
    want = R.table(text, lengths, rec, words, reads, R.options())
    assert R.same(want, R.table_naive(text, lengths, rec, words, reads, R.options())) == []
    assert R.same(F.errprof_host(text, lengths, rec, words, reads), want) == []
    K.check_position_case(length, want)


def test_homopolymer_bins():
    text, lengths, rec, words, reads, expected = K.homopolymer_case()
    for i, (section, index) in enumerate(expected):                      # every record on its own: its one gap falls into the bin that was worked out by hand
        got = F.errprof_host(text, lengths, rec[i: i + 1], words, reads)
        assert int(got[section][index]) == 1 and int(got[section].sum()) == 1, (i, section, index, np.nonzero(got[section])[0])
    want = R.table(text, lengths, rec, words, reads, R.options())
    assert R.same(want, R.table_naive(text, lengths, rec, words, reads, R.options())) == []
    assert R.same(F.errprof_host(text, lengths, rec, words, reads), want) == []


def test_symbols_and_python_names():
    L = capi.lib()
    names = [n for n in capi.EXPORTED if n.startswith("flx_errprof")]
    for name in names:
        getattr(L, name)
    assert len(names) == 9
    assert C.sizeof(capi.ErrprofOptions) == 32 and C.sizeof(capi.ErrprofTable) == 1152 * 8
    assert tuple(capi.ERRPROF_SECTIONS[:-1]) == R.SECTIONS and F.ERRPROF_SECTIONS == tuple(n for n, _ in R.SECTIONS) and F.ERRPROF_TOTALS == R.TOTALS
    assert capi.ErrprofTable.TOTALS.offset == 1137 * 8 and capi.ErrprofTable.reserved.offset == 1145 * 8
    o = F.errprof_options(count_secondary=True, min_mapq=7, flush_threshold=9)
    assert (o.count_secondary, o.min_mapq, o.flush_threshold) == (1, 7, 9)
    with pytest.raises(F.FloxerError):                                   # no device: the host form is errprof_host
        F.errprof(text=[np.ones(5, dtype=np.uint8)], device=-1)


def test_rule_header_against_a_column_walk_under_sanitizers(tmp_path):
    """tests/errprof_check.cpp: flx_errprof.hpp on random records, built with ASan + UBSan; nothing is preloaded"""
    exe = str(tmp_path / "errprof_check")
    src = os.path.join(ROOT, "tests", "errprof_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


def test_cli_error_profile_flags(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    base = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"),
            "--output", str(tmp_path / "o.sam"), "-e", "2"]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0
    lines = h.stderr.decode().splitlines()
    for flag in ("--error-profile", "--error-profile-secondary", "--error-profile-min-mapq"):
        line = [l for l in lines if re.search(rf"^\s+{flag}(\s|$)", l)]
        assert len(line) == 1 and line[0].startswith("      " + flag) and "not floxer's" in line[0], flag      # long spellings only
    env = dict(os.environ, FLX_CLI_PARSE_ONLY="1")                       # the parser alone: no device is touched
    tsv, other = str(tmp_path / "profile.tsv"), str(tmp_path / "sites.tsv")
    for extra in (["--error-profile", tsv], ["--error-profile", tsv, "--error-profile-secondary", "--error-profile-min-mapq", "254", "-Q", "-D", "-N", "1"],
                  ["--error-profile", tsv, "--pileup", other, "--left-align-indels"], ["--error-profile", tsv, "--error-profile-min-mapq", "1", "-Q"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and r.stdout == b"" and b"CLI PARSER ERROR" not in r.stderr, (extra, r.stderr)
    for extra in (["--error-profile", tsv, "-w"], ["--without-cigar", "--error-profile", tsv],
                  ["--error-profile", tsv, "--error-profile-min-mapq", "1"],                             # without -Q
                  ["--error-profile-secondary"], ["--error-profile-min-mapq", "1", "-Q"],                # no output
                  ["--error-profile", str(tmp_path / "profile.txt")], ["--error-profile", str(tmp_path / "profile")],
                  ["--error-profile", tsv, "-Q", "--error-profile-min-mapq", "0"], ["--error-profile", tsv, "-Q", "--error-profile-min-mapq", "255"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr and b"error-profile" in r.stderr, (extra, r.stderr)
    assert not any(os.path.exists(p) for p in (tsv, other))
