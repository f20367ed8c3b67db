"""Depth of coverage without a GPU (flx_coverage_host, the CLI's option checks): the plain-numpy rule of tests/coverage_ref.py against its
own column-by-column loop, the library's host rule against coverage_ref, every refusal of the rule, the CLI's parser errors, and tests/coverage_check.cpp: the rule header under
ASan + UBSan against a walk of every column."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import coverage_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [50, 3000, 977, 64, 1500]
SWITCHES = [dict(count_deletions=d, count_secondary=s, min_mapq=q, report_zero=z)
            for d, s, q, z in itertools.product([False, True], [False, True], [0, 3], [False, True])]


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(41)
    return R.random_records(rng, LENGTHS, 400)


def test_reference_against_its_naive_loop(batch):
    rec, words = batch
    assert {int(f) for f in rec["flag"]} == {0, 16, 256, 272, 2048, 2064, 4}
    seen = set()
    for o in SWITCHES:
        d = R.depth(LENGTHS, rec, words, o)
        assert (d == R.depth_naive(LENGTHS, rec, words, o)).all(), o
        assert d.max() > 1 and (d == 0).any()
        seen.add(d.tobytes())
        for zero in (False, True):
            a, b = R.runs(LENGTHS, d, zero), R.runs_naive(LENGTHS, d, zero)
            assert a.tolist() == b.tolist()
        ru = R.runs(LENGTHS, d, True)
        assert int((ru["end"] - ru["start"]).sum()) == sum(LENGTHS)
        for w in (0, 1, 7, 1000):
            win = R.windows(LENGTHS, d, w)
            assert win.tolist() == R.windows_naive(LENGTHS, d, w).tolist()
            assert int(win["depth_sum"].sum()) == int(d.astype(np.int64).sum()) and int(win["covered"].sum()) == int((d > 0).sum())
            assert len(win) == sum(1 if w == 0 else -(-n // w) for n in LENGTHS)
    assert len(seen) == 8                                                # the three counting switches all matter on this batch


def _host(lengths, rec, words, opt, depth):
    lens = np.asarray(lengths, dtype=np.uint64)
    return capi.lib().flx_coverage_host(capi.ptr(lens, capi.u64p), len(lens), C.byref(opt) if opt is not None else None,
                                        rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), capi.ptr(words, capi.u32p), len(words),
                                        capi.ptr(depth, capi.u32p))


def test_host_rule_equals_the_reference(batch):
    rec, words = batch
    for o in SWITCHES:
        assert (F.coverage_host(LENGTHS, rec, words, R.c_options(o)) == R.depth(LENGTHS, rec, words, o)).all(), o
    # NULL options are all zero, and the call adds to what the array holds
    want = R.depth(LENGTHS, rec, words, R.options())
    depth = np.full(sum(LENGTHS), 5, dtype=np.uint32)
    assert _host(LENGTHS, rec, words, None, depth) == 0 and (depth == want + 5).all()
    # records that share words, and words nobody refers to
    rec2 = np.concatenate([rec, rec])
    assert (F.coverage_host(LENGTHS, rec2, words, None) == 2 * want).all()


def test_every_refusal_leaves_the_depth_untouched():
    good = [(0, 1, 10, 60, [R.word("=", 20), R.word("X", 1), R.word("=", 5)]), (16, 0, 0, 60, [R.word("=", 50)])]

    def refused(rows, lengths=LENGTHS, opt=None, words_cut=0, match=None):
        rec, words = R.records_of(good + rows)
        depth = np.full(sum(LENGTHS), 7, dtype=np.uint32)
        rc = _host(lengths, rec, words[: len(words) - words_cut], opt, depth)
        assert rc == -1 and (depth == 7).all(), rows
        if match:
            assert match in capi.lib().flx_last_error().decode(), capi.lib().flx_last_error()

    refused([(0, 1, 0, 60, [])], match="no CIGAR words")                                   # a counted record of a without_cigar run
    for op in "MNHP":
        refused([(0, 1, 0, 60, [R.word(op, 3)])], match="other than")
    refused([(0, 1, 0, 60, [R.word("=", 3), 9 << 4 | 9])], match="other than")
    refused([(0, 1, 0, 60, [R.word("=", 3), R.word("I", 0)])], match="length 0")
    refused([(0, 5, 0, 60, [R.word("=", 3)])], match="reference_id")
    refused([(0, -1, 0, 60, [R.word("=", 3)])], match="reference_id")
    refused([(0, 3, 60, 60, [R.word("=", 5)])], match="behind its sequence")
    refused([(0, 3, 0, 60, [R.word("=", 60), R.word("I", 9), R.word("D", 5)])], match="behind its sequence")     # the D column counts for the span
    refused([(0, 3, -1, 60, [R.word("=", 5)])], match="negative")
    refused([(0, 1, 0, 60, [R.word("=", 3)])], words_cut=1, match="outside the pool")
    bad = capi.CoverageOptions()
    bad.reserved[2] = 1
    refused([], opt=bad, match="reserved")
    refused([], lengths=[50, 1 << 31], match="2^31")
    refused([], lengths=[50, 0], match="empty")
    # the same words are fine where the record does not count, and a span that ends exactly at its sequence's end is fine
    rec, words = R.records_of(good + [(4, -1, 0, 0, []), (256, 9, 0, 0, [R.word("M", 3)]), (0, 3, 0, 2, [R.word("P", 1)]), (2048, 3, 4, 60, [R.word("S", 9), R.word("=", 60)])])
    depth = np.zeros(sum(LENGTHS), dtype=np.uint32)
    assert _host(LENGTHS, rec, words, R.c_options(R.options(min_mapq=3)), depth) == 0
    assert int(depth.sum()) == 26 + 50 + 60 and depth[sum(LENGTHS[:3]) + 4] == 1 and depth[sum(LENGTHS[:3]) + 3] == 0


def test_symbols_geometry_and_python_names():
    L = capi.lib()
    for name in capi.EXPORTED:
        if name.startswith("flx_coverage"):
            getattr(L, name)
    assert sum(n.startswith("flx_coverage") for n in capi.EXPORTED) == 14
    t, b = F.coverage_geometry()
    assert t >= 64 and b >= 2 and t * b + 1 <= 1 << 28
    assert C.sizeof(capi.CoverageOptions) == 32 and C.sizeof(capi.DepthRun) == 24 and C.sizeof(capi.DepthWindow) == 40
    assert F.RUN_DTYPE.itemsize == 24 and F.WINDOW_DTYPE.itemsize == 40
    o = F.coverage_options(count_deletions=True, min_mapq=7)
    assert (o.count_deletions, o.count_secondary, o.min_mapq, o.report_zero) == (1, 0, 7, 0)


def test_rule_header_against_a_column_walk_under_sanitizers(tmp_path):
    """tests/coverage_check.cpp: flx_coverage.hpp on random records, built with ASan + UBSan"""
    exe = str(tmp_path / "coverage_check")
    src = os.path.join(ROOT, "tests", "coverage_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


def test_cli_coverage_flags(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    base = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"),
            "--output", str(tmp_path / "o.sam"), "-e", "2"]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0
    lines = h.stderr.decode().splitlines()
    for flag in ("--coverage", "--coverage-summary", "--coverage-windows", "--coverage-window", "--coverage-deletions", "--coverage-secondary",
                 "--coverage-zero", "--coverage-min-mapq"):
        line = [l for l in lines if re.search(rf"^\s+{flag}(\s|$)", l)]
        assert len(line) == 1 and line[0].startswith("      " + flag) and "not floxer's" in line[0], flag      # long spellings only
    env = dict(os.environ, FLX_CLI_PARSE_ONLY="1")                       # the parser alone: no device is touched
    bg, tsv, tsv2 = str(tmp_path / "d.bedgraph"), str(tmp_path / "s.tsv"), str(tmp_path / "w.tsv")
    for extra in (["--coverage", bg], ["--coverage-summary", tsv], ["--coverage-windows", tsv2, "--coverage-window", "100"],
                  ["--coverage", bg, "--coverage-summary", tsv, "--coverage-windows", tsv2, "--coverage-window", "1", "--coverage-deletions",
                   "--coverage-secondary", "--coverage-zero", "--coverage-min-mapq", "254", "-Q", "-D", "-N", "1"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and r.stdout == b"" and b"CLI PARSER ERROR" not in r.stderr, (extra, r.stderr)
    for extra in (["--coverage", bg, "-w"], ["-w", "--coverage-summary", tsv], ["--coverage-windows", tsv2, "--coverage-window", "10", "--without-cigar"],
                  ["--coverage", bg, "--coverage-min-mapq", "1"],                                       # without -Q
                  ["--coverage-deletions"], ["--coverage-secondary"], ["--coverage-zero"], ["--coverage-min-mapq", "1", "-Q"],       # no output
                  ["--coverage-window", "10"], ["--coverage", bg, "--coverage-window", "10"], ["--coverage-windows", tsv2],
                  ["--coverage-windows", tsv2, "--coverage-window", "0"],
                  ["--coverage", str(tmp_path / "d.bed")], ["--coverage", tsv], ["--coverage-summary", bg], ["--coverage-summary", str(tmp_path / "s.txt")],
                  ["--coverage-windows", bg, "--coverage-window", "10"],
                  ["--coverage", bg, "-Q", "--coverage-min-mapq", "0"], ["--coverage", bg, "-Q", "--coverage-min-mapq", "255"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr and b"overage" in r.stderr, (extra, r.stderr)
    assert not any(os.path.exists(p) for p in (bg, tsv, tsv2))
