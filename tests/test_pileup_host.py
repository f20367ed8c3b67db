"""Allele pileup without a GPU (flx_pileup_host, flx_pileup_sites_host, the CLI's option checks): the plain-numpy rule of
tests/pileup_ref.py against its own column-by-column loop, the library's host rule against pileup_ref, every refusal of the rule, the
site thresholds on their boundaries, the CLI's parser errors, and tests/pileup_check.cpp: the rule header under ASan + UBSan against a
walk of every column."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import pileup_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [50, 3000, 977, 64, 1500]
SWITCHES = [R.options(count_secondary=s, min_mapq=q) for s, q in itertools.product([False, True], [0, 3])]
SITE_SWITCHES = [R.options(), R.options(min_depth=1, min_count=1, min_permille=1), R.options(min_depth=6, min_count=3, min_permille=500),
                 R.options(min_depth=2, min_count=1, min_permille=1000)]


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(43)
    rec, words = R.random_records(rng, LENGTHS, 400)
    return rec, words, R.attach_reads(rng, rec, words)


def test_reference_against_its_naive_loop(batch):
    rec, words, reads = batch
    assert {int(f) for f in rec["flag"]} == {0, 16, 256, 272, 2048, 2064, 4}
    assert any((r == 0).any() for r in reads) and any((r == 5).any() for r in reads)
    seen = set()
    for o in SWITCHES:
        c = R.counts(LENGTHS, rec, words, reads, o)
        assert (c == R.counts_naive(LENGTHS, rec, words, reads, o)).all(), o
        assert all(c[k].max() >= 1 for k in range(7)) and c[R.DEPTH].max() > 3
        assert (c[R.A:R.T + 1].sum(axis=0) <= c[R.DEPTH]).all()          # a letter is counted on a DEPTH column only
        seen.add(c.tobytes())
        for s in SITE_SWITCHES:
            a, b = R.sites(LENGTHS, c, s), R.sites_naive(LENGTHS, c, s)
            assert len(a) == len(b) and a.tobytes() == b.tobytes()
        assert 0 < len(R.sites(LENGTHS, c, SITE_SWITCHES[1])) < sum(LENGTHS)
    assert len(seen) == 4                                                # both counting switches matter on this batch
    # the same read as flag 0 and flag 16: complementary planes at mirrored columns
    read = np.array([1, 2, 3, 4, 5, 0, 1, 1], dtype=np.uint8)
    ws = [R.word("X", 8)]
    fw = R.counts([8], *R.records_of([(0, 0, 0, 0, ws)]), [read], R.options())
    rv = R.counts([8], *R.records_of([(16, 0, 0, 0, ws)]), [read], R.options())
    assert (fw[R.A:R.T + 1] == rv[R.A:R.T + 1][::-1, ::-1]).all() and fw[R.A:R.T + 1].sum() == 6 and (fw[R.DEPTH] == 1).all()


def _host(lengths, rec, words, reads, opt, counts):
    lens = np.asarray(lengths, dtype=np.uint64)
    pool, offs, n = F._pool_and_offsets(reads)
    return capi.lib().flx_pileup_host(capi.ptr(lens, capi.u64p), len(lens), C.byref(opt) if opt is not None else None,
                                      rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), capi.ptr(words, capi.u32p), len(words),
                                      capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n, capi.ptr(counts, capi.u32p))


def test_host_rule_equals_the_reference(batch):
    rec, words, reads = batch
    for o in SWITCHES:
        want = R.counts(LENGTHS, rec, words, reads, o)
        got = F.pileup_host(LENGTHS, rec, words, reads, R.c_options(o))
        assert got.shape == want.shape and (got == want).all(), o
        for s in SITE_SWITCHES:
            full = dict(o, **{k: s[k] for k in ("min_depth", "min_count", "min_permille")})
            assert F.pileup_sites_host(LENGTHS, got, R.c_options(full)).tobytes() == R.sites(LENGTHS, want, full).tobytes(), full
    # NULL options are all zero, and the call adds to what the array holds
    want = R.counts(LENGTHS, rec, words, reads, R.options())
    counts = np.full((7, sum(LENGTHS)), 5, dtype=np.uint32)
    assert _host(LENGTHS, rec, words, reads, None, counts) == 0 and (counts == want + 5).all()
    assert F.pileup_sites_host(LENGTHS, want).tobytes() == R.sites(LENGTHS, want, R.options()).tobytes()
    # records that share words and reads
    rec2 = np.concatenate([rec, rec])
    assert (F.pileup_host(LENGTHS, rec2, words, reads) == 2 * want).all()
    # the capacity of the site call: one slot too few carries the need
    sites = R.sites(LENGTHS, want, R.options(min_depth=1, min_count=1, min_permille=1))
    lens = np.asarray(LENGTHS, dtype=np.uint64)
    opt = R.c_options(R.options(min_depth=1, min_count=1, min_permille=1))
    out = np.zeros(len(sites), dtype=F.SITE_DTYPE)
    n = C.c_uint64(len(sites) - 1)
    rc = capi.lib().flx_pileup_sites_host(capi.ptr(lens, capi.u64p), len(lens), C.byref(opt), capi.ptr(want, capi.u32p), out.ctypes.data_as(C.POINTER(capi.PileupSite)), C.byref(n))
    assert rc == -3 and n.value == len(sites) and "too small" in capi.lib().flx_last_error().decode()
    rc = capi.lib().flx_pileup_sites_host(capi.ptr(lens, capi.u64p), len(lens), C.byref(opt), capi.ptr(want, capi.u32p), out.ctypes.data_as(C.POINTER(capi.PileupSite)), C.byref(n))
    assert rc == 0 and n.value == len(sites) and out.tobytes() == sites.tobytes()


def test_every_refusal_leaves_the_counts_untouched():
    rng = np.random.default_rng(5)
    good = [(0, 1, 10, 60, [R.word("=", 20), R.word("X", 1), R.word("=", 5)]), (16, 0, 0, 60, [R.word("S", 3), R.word("I", 2), R.word("=", 50)])]

    def refused(rows, lengths=LENGTHS, opt=None, words_cut=0, match=None, fix=None):
        rec, words, reads = R.records_with_reads(rng, good + rows)
        if fix:
            fix(rec, reads)
        counts = np.full((7, sum(LENGTHS)), 7, dtype=np.uint32)
        rc = _host(lengths, rec, words[: len(words) - words_cut], reads, opt, counts)
        assert rc == -1 and (counts == 7).all(), rows
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
    # its own
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
    bad = R.c_options(R.options(min_permille=1001))
    refused([], opt=bad, match="min_permille")
    bad = capi.PileupOptions()
    bad.reserved[2] = 1
    refused([], opt=bad, match="reserved")
    counts = np.zeros((7, sum(LENGTHS)), dtype=np.uint32)
    lens = np.asarray(LENGTHS, dtype=np.uint64)
    n = C.c_uint64(0)
    for opt, match in ((bad, "reserved"), (R.c_options(R.options(min_permille=1001)), "min_permille")):
        assert capi.lib().flx_pileup_sites_host(capi.ptr(lens, capi.u64p), len(lens), C.byref(opt), capi.ptr(counts, capi.u32p), None, C.byref(n)) == -1
        assert match in capi.lib().flx_last_error().decode()
    # the same words are fine where the record does not count; a span that ends exactly at its sequence's end and a D-only record are fine
    rows = good + [(4, -1, 0, 0, []), (256, 9, 0, 0, [R.word("M", 3)]), (0, 3, 0, 2, [R.word("I", 1)]), (2048, 3, 4, 60, [R.word("S", 9), R.word("=", 60)]),
                   (0, 3, 0, 60, [R.word("D", 4)])]
    rec, words, reads = R.records_with_reads(rng, rows)
    rec[2]["read"] = 10 ** 6                                             # (not judged: it does not count)
    opt = R.options(min_mapq=3)
    counts = np.zeros((7, sum(LENGTHS)), dtype=np.uint32)
    assert _host(LENGTHS, rec, words, reads, R.c_options(opt), counts) == 0
    assert (counts == R.counts_naive(LENGTHS, rec, words, reads, opt)).all()
    at = sum(LENGTHS[:3])
    assert counts[R.DEL][at: at + 4].tolist() == [1] * 4 and counts[R.DEPTH][at + 3] == 0 and counts[R.DEPTH][at + 4] == 1
    assert counts[R.INS][0] == 1 and counts[R.INS].sum() == 1            # the leading insertion of the flag-16 record: anchored on its first column


def _one_position(v, o):
    """the sites of one position with the plane counts v"""
    cnt = np.array(v, dtype=np.uint32).reshape(7, 1)
    got = F.pileup_sites_host([1], cnt, R.c_options(o))
    want = R.sites_naive([1], cnt, o)
    assert got.tobytes() == want.tobytes(), (v, o)
    return len(got)


def test_site_thresholds_on_their_boundaries():
    #                 DEPTH DEL A  C  G  T  INS
    o = R.options(min_depth=10, min_count=3, min_permille=300)
    assert _one_position([10, 0, 0, 3, 0, 0, 0], o) == 1                  # best * 1000 == min_permille * cov
    assert _one_position([11, 0, 0, 3, 0, 0, 0], o) == 0                  # one below the fraction (3000 < 3300)
    assert _one_position([7, 3, 0, 0, 0, 0, 0], o) == 1                   # cov == min_depth through DEL, DEL the best plane
    assert _one_position([9, 0, 0, 3, 0, 0, 0], o) == 0                   # cov one below
    assert _one_position([8, 2, 0, 2, 2, 0, 0], o) == 0                   # best one below min_count, a tie of three planes
    assert _one_position([10, 0, 0, 0, 0, 0, 3], o) == 1                  # INS the best plane
    assert _one_position([10, 0, 0, 0, 3, 3, 0], o) == 1                  # a tie between planes
    assert _one_position([10, 0, 1, 1, 1, 0, 0], o) == 0                  # three letters, none of them often enough
    # the defaults for 0: 4, 2, 200
    d = R.options()
    assert _one_position([4, 0, 2, 0, 0, 0, 0], d) == 1 and _one_position([3, 0, 2, 0, 0, 0, 0], d) == 0
    assert _one_position([10, 0, 2, 0, 0, 0, 0], d) == 1 and _one_position([11, 0, 2, 0, 0, 0, 0], d) == 0 and _one_position([5, 0, 1, 1, 1, 1, 1], d) == 0
    # 64-bit: cov above 2^32, best * 1000 above 2^32
    big = 0xFFFFFFFF
    assert _one_position([big, big, 0, 0, 0, big, 0], R.options(min_permille=500)) == 1
    assert _one_position([big, big, 0, 0, 0, big, 0], R.options(min_permille=501)) == 0
    assert _one_position([big, 0, 0, 0, 0, 0, big], R.options(min_permille=1000)) == 1
    # reference ids on both sides of a boundary, in position order
    lengths = [2, 1, 3]
    cnt = np.zeros((7, 6), dtype=np.uint32)
    cnt[R.DEPTH], cnt[R.G] = 5, [0, 5, 5, 5, 0, 5]
    got = F.pileup_sites_host(lengths, cnt)
    assert got.tobytes() == R.sites(lengths, cnt, R.options()).tobytes()
    assert got["ref"].tolist() == [0, 1, 2, 2] and got["pos"].tolist() == [1, 0, 0, 2] and got["alt"][:, 2].tolist() == [5] * 4


def test_symbols_and_python_names():
    L = capi.lib()
    names = [n for n in capi.EXPORTED if n.startswith("flx_pileup")]
    for name in names:
        getattr(L, name)
    assert len(names) == 13
    assert C.sizeof(capi.PileupOptions) == 32 and C.sizeof(capi.PileupSite) == 40 and F.SITE_DTYPE.itemsize == 40
    assert [F.SITE_DTYPE.fields[k][1] for k in ("ref", "pos", "depth", "del", "ins", "alt", "res")] == [0, 4, 8, 12, 16, 20, 36]
    o = F.pileup_options(count_secondary=True, min_mapq=7, min_depth=9, min_count=3, min_permille=250)
    assert (o.count_secondary, o.min_mapq, o.min_depth, o.min_count, o.min_permille) == (1, 7, 9, 3, 250)
    assert F.PILEUP_PLANES == ("DEPTH", "DEL", "A", "C", "G", "T", "INS")


def test_rule_header_against_a_column_walk_under_sanitizers(tmp_path):
    """tests/pileup_check.cpp: flx_pileup.hpp on random records, built with ASan + UBSan; nothing is preloaded"""
    exe = str(tmp_path / "pileup_check")
    src = os.path.join(ROOT, "tests", "pileup_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


def test_cli_pileup_flags(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    base = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"),
            "--output", str(tmp_path / "o.sam"), "-e", "2"]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0
    lines = h.stderr.decode().splitlines()
    for flag in ("--pileup", "--pileup-min-depth", "--pileup-min-count", "--pileup-min-fraction", "--pileup-secondary", "--pileup-min-mapq"):
        line = [l for l in lines if re.search(rf"^\s+{flag}(\s|$)", l)]
        assert len(line) == 1 and line[0].startswith("      " + flag) and "not floxer's" in line[0], flag      # long spellings only
    assert "1-based" in [l for l in lines if re.search(r"^\s+--pileup\s", l)][0]
    env = dict(os.environ, FLX_CLI_PARSE_ONLY="1")                       # the parser alone: no device is touched
    tsv, bg = str(tmp_path / "sites.tsv"), str(tmp_path / "d.bedgraph")
    for extra in (["--pileup", tsv], ["--pileup", tsv, "--pileup-min-depth", "1", "--pileup-min-count", "1", "--pileup-min-fraction", "1"],
                  ["--pileup", tsv, "--pileup-min-fraction", "0.0005", "--pileup-secondary", "--pileup-min-mapq", "254", "-Q", "-D", "-N", "1"],
                  ["--pileup", tsv, "--coverage", bg, "--left-align-indels"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and r.stdout == b"" and b"CLI PARSER ERROR" not in r.stderr, (extra, r.stderr)
    for extra in (["--pileup", tsv, "-w"], ["--without-cigar", "--pileup", tsv],
                  ["--pileup", tsv, "--pileup-min-mapq", "1"],                                          # without -Q
                  ["--pileup-min-depth", "3"], ["--pileup-min-count", "3"], ["--pileup-min-fraction", "0.5"], ["--pileup-secondary"],
                  ["--pileup-min-mapq", "1", "-Q"],                                                     # no output
                  ["--pileup", str(tmp_path / "sites.txt")], ["--pileup", bg], ["--pileup", str(tmp_path / "sites")],
                  ["--pileup", tsv, "-Q", "--pileup-min-mapq", "0"], ["--pileup", tsv, "-Q", "--pileup-min-mapq", "255"],
                  ["--pileup", tsv, "--pileup-min-fraction", "0"], ["--pileup", tsv, "--pileup-min-fraction", "1.001"],
                  ["--pileup", tsv, "--pileup-min-fraction", "-0.1"], ["--pileup", tsv, "--pileup-min-depth", "0"],
                  ["--pileup", tsv, "--pileup-min-count", "0"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr and b"pileup" in r.stderr, (extra, r.stderr)
    assert not any(os.path.exists(p) for p in (tsv, bg))
