"""Left-aligned indels, without a GPU: the rule (floxer_amd/csrc/flx_leftalign.hpp through flx_left_align) against the plain Python rule of
tests/leftalign_ref.py on hand-made paths and on 20 000 random, non-optimal paths over low-complexity sequences, with everything the
rule promises checked per path; the struct layouts, symbols and defaults; the option checks (judged before the context is looked at);
the CLI's flag combinations; and tests/leftalign_check.cpp: the header under ASan + UBSan against a one-column-at-a-time definition."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import leftalign_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(cases):
    ref, qry, words, jobs = R.pack_jobs(cases)
    return [R.path_of(w) for w in F.left_align(ref, qry, words, jobs)]


def case(cigar, ref, qry, begin=0):
    return R.parse(cigar), np.array(list(ref), dtype=np.uint8), np.array(list(qry), dtype=np.uint8), begin


# hand-made paths: (path, ref, qry, begin) -> the words the rule gives
HAND = [
    # a 1-column D and a 1-row I at the right end of a 7-letter homopolymer: they land on the run's second column (the first stays)
    (case("7=1D2=", b"AAAAAAAACG", b"AAAAAAACG"), "1=1D8="),
    (case("1=6=1D2=", b"CAAAAAAAGT", b"CAAAAAAGT"), "1=1D8="),
    (case("7=1I2=", b"AAAAAAACG", b"AAAAAAAACG"), "1=1I8="),
    # the issue's example: the word count grows
    (case("5=2D1X", b"ACACACAG", b"ACACAT"), "1=2D4=1X"),
    (case("5=2D1X", b"GTACACAG", b"GTACAT"), "2=2D3=1X"),
    # a period-3 repeat: a D of 3, of 6, and a shift that is no multiple of the period
    (case("1X9=3D1X", b"TACGACGACGACGT", b"GACGACGACGA"), "1X3D9=1X"),
    (case("1X8=6D1X", b"TCGACGACGACGACGT", b"GCGACGACGA"), "1X6D8=1X"),
    (case("1X1=8=3D2=", b"TTCGACGACGACGAC", b"GTCGACGACGAC"), "1X1=3D10="),
    # the = run consumed exactly, then X: stop; the other gap kind: stop
    (case("2=1X3=1D1=", b"GGTAAAAC", b"GGCAAAC"), "2=1X1D4="),
    (case("2=1I3=1D1=", b"GGAAAAC", b"GGTAAAC"), "2=1I1D4="),
    # the same kind: merge and stop, merge and go on
    (case("1=1X1D2=1D1=", b"GTAAAAC", b"GCAAC"), "1=1X2D3="),
    (case("3=1D2=1D1=", b"GAAAAAAC", b"GAAAAC"), "1=2D5="),
    # the first-word rule
    (case("3=2D", b"AAAAA", b"AAA"), "1=2D2="),
    (case("2D3=1D", b"AAAAAA", b"AAA"), "3D3="),
    (case("1=1D", b"AA", b"A"), "1=1D"),
    # nothing to do
    (case("4=", b"ACGT", b"ACGT"), "4="),
    (case("2I", b"", b"AC"), "2I"),
    (case("2=1D2=", b"ACGTA", b"ACTA", ), "2=1D2="),
    # begin is not 0; letters of rank 0 and 5
    (case("3=1D1=", [9, 9, 0, 0, 0, 0, 5], [0, 0, 0, 5], 2), "1=1D3="),
    (case("1X3=1I1=", [1, 5, 5, 5, 0], [0, 5, 5, 5, 5, 0]), "1X1I4="),
]


def test_hand_made_paths():
    cases = [c for c, _ in HAND]
    want = [R.parse(w) for _, w in HAND]
    assert [R.left_align(*c) for c in cases] == want
    assert host(cases) == want
    for c, w in zip(cases, want):
        R.check_properties(*c, w)
    # adjacent words of one op in the input merge too
    assert host([case("2=2=1X1X1D1D2=", b"ACGTAAAAAA", b"ACGTCCAA")]) == [R.parse("4=2X2D2=")]


def test_host_rule_on_20000_random_paths():
    cases = R.random_corpus(11, 20000)
    got = host(cases)
    moved = grown = merged = 0
    for c, g in zip(cases, got):
        want = R.left_align(*c)
        assert g == want, (R.show(c[0]), R.show(g), R.show(want))
        R.check_properties(*c, g)
        moved += g != c[0]
        grown += len(g) > len(c[0])
        merged += sum(op in (R.I, R.D) for op, _ in g) < sum(op in (R.I, R.D) for op, _ in c[0])
    assert moved > 4000 and grown > 500 and merged > 500, (moved, grown, merged)
    # input that is not in normal form: neighbouring words of one op
    cases2 = R.random_corpus(13, 4000, repeats=True)
    assert sum(not R.normal_form(c[0]) for c in cases2) > 1500
    for c, g in zip(cases2, host(cases2)):
        assert g == R.left_align(*c), (R.show(c[0]), R.show(g))
        R.check_properties(*c, g)
    assert [R.show(p) for p in host([case("1X1X", b"AA", b"CC"), case("5=1X1X", b"AAAAAAA", b"AAAAACC"), case("1D1D", b"AA", b"")])] == ["2X", "5=2X", "2D"]
    # idempotent through the library as well
    again = host([(g, c[1], c[2], c[3]) for c, g in zip(cases[:2000], got[:2000])])
    assert again == got[:2000]


def test_bad_jobs_are_refused():
    ref = np.array(list(b"AAAAAAAACG"), dtype=np.uint8)
    qry = np.array(list(b"AAAAAAACG"), dtype=np.uint8)
    words = R.words_of(R.parse("7=1D2=") + [(4, 3), (7, 0)])             # a soft clip and a zero-length word behind the path
    good = (0, 3, 0, 10, 0, 0, 9)
    assert [R.show(R.path_of(w)) for w in F.left_align(ref, qry, words, [good])] == ["1=1D8="]
    bad = {"outside its pools": [(0, 6, 0, 10, 0, 0, 9), (5, 1, 0, 10, 0, 0, 9)][:1] + [(0, 3, 1, 10, 0, 0, 9), (0, 3, 0, 10, 0, 1, 9), (1 << 40, 1, 0, 10, 0, 0, 9)],
           "other than = X I D": [(3, 1, 0, 10, 0, 0, 9)],
           "length 0": [(4, 1, 0, 10, 0, 0, 9)],
           "do not fit": [(0, 3, 0, 9, 0, 0, 9), (0, 3, 0, 10, 1, 0, 9), (0, 3, 0, 10, 0, 0, 8)]}
    for msg, jobs in bad.items():
        for j in jobs:
            with pytest.raises(F.FloxerError, match=msg):
                F.left_align(ref, qry, words, [good, j])
    assert F.left_align(ref, qry, words, []) == [] and [len(w) for w in F.left_align(ref, qry, words, [(0, 0, 0, 0, 0, 0, 0)])] == [0]
    # the raw calls: reserved fields, the output pool's capacity, null arguments; the kernel's seam judges its jobs on the host as well
    L = capi.lib()
    job = (capi.LeftAlignJob * 1)(capi.LeftAlignJob(0, 3, 0, 0, 10, 0, 0, 9, 0))
    out = np.zeros(8, dtype=np.uint32)
    refs = (capi.CigarRef * 1)()
    args = lambda n: (capi.ptr(ref, capi.u8p), 10, capi.ptr(qry, capi.u8p), 9, capi.ptr(words, capi.u32p), len(words), job, 1, capi.ptr(out, capi.u32p), C.byref(n), refs)
    n = C.c_uint64(2)
    assert L.flx_left_align(*args(n)) == -3 and n.value == 3 and b"too small" in L.flx_last_error()
    n = C.c_uint64(8)
    assert L.flx_left_align(*args(n)) == 0 and n.value == 3 and (refs[0].offset, refs[0].length) == (0, 3)
    job[0].reserved2 = 1
    assert L.flx_left_align(*args(n)) == -1 and b"reserved" in L.flx_last_error() and n.value == 0
    job[0].reserved2 = 0
    assert L.flx_left_align_batch(None, *args(n)) == -1 and b"null" in L.flx_last_error()
    assert L.flx_left_align(None, 10, *args(n)[2:]) == -1 and b"null" in L.flx_last_error()


def test_struct_layouts_exported_symbols_and_defaults():
    assert C.sizeof(capi.GapOptions) == 32 and C.sizeof(capi.LeftAlignJob) == 48 and C.sizeof(capi.CigarRef) == 16
    assert [getattr(capi.GapOptions, f).offset for f in ("left_align", "reserved")] == [0, 4]
    assert [getattr(capi.LeftAlignJob, f).offset for f in ("cigar_offset", "cigar_length", "reserved", "ref_offset", "ref_length", "begin", "query_offset",
                                                           "query_length", "reserved2")] == [0, 8, 12, 16, 24, 28, 32, 40, 44]
    assert [getattr(capi.CigarRef, f).offset for f in ("offset", "length", "reserved")] == [0, 8, 12]
    assert C.sizeof(capi.RunOptions) == 64 and C.sizeof(capi.SplitOptions) == 32        # the frozen structs keep their sizes
    new = {"flx_align_reads_gaps", "flx_align_reads_resident_gaps", "flx_align_batch_gaps", "flx_left_align", "flx_left_align_batch"}
    assert set(capi.EXPORTED) >= new
    for name in capi.EXPORTED:
        assert hasattr(capi.lib(), name), name
    o = F.gap_options()
    assert (o.left_align, list(o.reserved)) == (1, [0] * 7)
    assert F.gap_options(left_align=False).left_align == 0
    assert F.aligner(None, None).gaps is None


def test_options_are_judged_before_the_context_is_looked_at():
    L = capi.lib()
    p = F.params(error_probability=0.05)
    run = C.c_void_p()
    pool = np.ones(8, dtype=np.uint8)
    offs = np.array([0, 8], dtype=np.uint64)

    def call(gaps, split=None, partial=None):
        b = capi.RunOptions()
        if partial is not None:
            b.partial = C.pointer(partial)
        gp = C.byref(gaps) if gaps is not None else None
        sp = C.byref(split) if split is not None else None
        # (no context at all: the options are judged first)
        a = L.flx_align_reads_gaps(None, C.byref(p), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), 1, C.byref(b), sp, gp, C.byref(run))
        ea = L.flx_last_error()
        r = L.flx_align_reads_resident_gaps(None, C.byref(p), None, C.byref(b), sp, gp, C.byref(run))
        assert a == r == -1
        return ea + b"|" + L.flx_last_error()

    for k in range(7):
        g = F.gap_options()
        g.reserved[k] = 1
        assert call(g).count(b"flx_gap_options: the reserved fields") == 2, k
    g = F.gap_options()
    g.left_align = 2
    assert call(g).count(b"flx_gap_options: left_align must be 0 or 1") == 2
    p.without_cigar = 1
    assert call(F.gap_options()).count(b"flx_gap_options.left_align needs the CIGAR's trace") == 2
    for off in (None, capi.GapOptions(), F.gap_options(left_align=False)):      # off: it needs nothing
        msg = call(off)
        assert b"flx_gap_options" not in msg and b"null" in msg, msg
    p.without_cigar = 0
    # the other options' refusals still come, and a valid struct leaves the refusal to the null context
    assert call(F.gap_options(), split=F.split_options()).count(b"needs flx_partial_options.enable") == 2
    msg = call(F.gap_options())
    assert b"flx_gap_options" not in msg and b"null" in msg, msg
    # the batch seam judges the struct first as well
    g = F.gap_options()
    g.reserved[3] = 1
    assert L.flx_align_batch_gaps(None, None, 0, None, 0, None, 0, None, None, None, None, None, None, C.byref(g)) == -1
    assert b"flx_gap_options: the reserved fields" in L.flx_last_error()


def test_rule_header_against_single_steps_under_sanitizers(tmp_path):
    """tests/leftalign_check.cpp: flx_leftalign.hpp on 20 000 random paths, built with ASan + UBSan"""
    exe = str(tmp_path / "leftalign_check")
    src = os.path.join(ROOT, "tests", "leftalign_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


def test_cli_flags(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    base = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"),
            "--output", str(tmp_path / "o.sam"), "-e", "2"]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0
    line = [l for l in h.stderr.decode().splitlines() if l.strip().startswith("--left-align-indels ")]
    assert len(line) == 1 and line[0].startswith("      --") and "opt-in, not floxer's" in line[0]        # long spelling only
    env = dict(os.environ, FLX_CLI_PARSE_ONLY="1")               # the options are parsed, then only the reader runs (no GPU)
    for extra in (["--left-align-indels"], ["--left-align-indels", "--md-tag", "-Q", "-D", "-N", "2"],
                  ["--left-align-indels", "--partial-alignments", "-N", "1", "--split-tails", "--partial-extend", "--sa-tag"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and b"CLI PARSER ERROR" not in r.stderr, (extra, r.stderr)
    for extra in (["--left-align-indels", "-w"], ["--without-cigar", "--left-align-indels"], ["--left-align"], ["--left-align-indels", "x"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr, extra
