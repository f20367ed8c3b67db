"""Affine-gap realignment, without a GPU: the rule (floxer_amd/csrc/flx_realign.hpp through flx_realign) against the plain Python rule
of tests/realign_ref.py, word for word and in score, NM and band, on hand-made paths and on 2400 random paths (alphabets of 4 and 2
letters, bands 1, 2 and 16, four score sets), with everything the rule promises checked per path; the struct layouts, symbols and
defaults; every refusal; and tests/realign_check.cpp: the header under ASan + UBSan against a full-matrix definition."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import realign_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def opts(scores=R.DEFAULT, band=16):
    return F.realign_options(True, *scores, band)


def host(cases, scores=R.DEFAULT, band=16):
    ref, qry, words, jobs = R.pack_jobs(cases)
    return F.realign(ref, qry, words, jobs, opts(scores, band))


def same(got, want):
    path, score, nm, lo, hi = want
    return (R.path_of(got["words"]), got["score"], got["num_errors"], got["diag_lo"], got["diag_hi"], got["kept"]) == (path, score, nm, lo, hi, 0)


def case(cigar, ref, qry, begin=0):
    return R.parse(cigar), np.array(list(ref), dtype=np.uint8), np.array(list(qry), dtype=np.uint8), begin


# hand-made paths under the default scores: (path, ref, qry, begin) -> the words the rule gives
HAND = [
    # the issue's scattered deletion: three gap words become one gap and an X (28 -> 30 under the default scores)
    (case("10=1D2=1D1=1D10=", b"TTGACCATCT" + b"ACGCGT" + b"AATCGGCTAC", b"TTGACCATCT" + b"CGG" + b"AATCGGCTAC"), "10=3D2=1X10="),
    # already optimal: all =, one X, one gap
    (case("12=", b"ACGTTGCAAGCT", b"ACGTTGCAAGCT"), "12="),
    (case("5=1X6=", b"ACGTTGCAAGCT", b"ACGTTCCAAGCT"), "5=1X6="),
    (case("6=3D6=", b"ACGTTGCAAGCTAGG", b"ACGTTGGCTAGG"), "6=3D6="),
    # the ends: all-D (no rows), all-I (no columns), the empty path
    (case("4D", b"ACGT", b""), "4D"),
    (case("3I", b"", b"ACG"), "3I"),
    (case("", b"", b""), ""),
    # begin is not 0; ranks 0 and 5 are letters like any other
    (case("3=1D3=", [9, 9, 0, 5, 0, 1, 5, 0, 5], [0, 5, 0, 5, 0, 5], 2), "3=1D3="),
    # ties: the walk starts at the end and takes a gap move as soon as one is as good, so in a homopolymer the gap lands on the right
    (case("4=2D2=", b"AAAAAAAA", b"AAAAAA"), "6=2D"),
    (case("4=2I2=", b"AAAAAA", b"AAAAAAAA"), "6=2I"),
    # I against D at equal cost: up wins over left at the last cell
    (case("2=1X2=", b"ACGTA", b"ACTTA"), "2=1X2="),
    (case("1I1D", b"A", b"C"), "1X"),
]


def test_hand_made_paths():
    cases = [c for c, _ in HAND]
    got = host(cases)
    for (c, want), g in zip(HAND, got):
        ref_rule = R.realign(*c)
        assert same(g, ref_rule), (R.show(c[0]), R.show(R.path_of(g["words"])), R.show(ref_rule[0]), g, ref_rule[1:])
        R.check_properties(*c, R.path_of(g["words"]), g["score"])
        if want is not None:
            assert R.show(ref_rule[0]) == want, (R.show(c[0]), R.show(ref_rule[0]))
    merged = R.path_of(got[0]["words"])
    assert R.gap_words(merged) == 1 and R.gap_words(HAND[0][0][0]) == 3 and got[0]["score"] == 30 == R.path_score(HAND[0][0][0], R.DEFAULT) + 2, R.show(merged)


def test_host_rule_on_2400_random_paths():
    cases = R.random_corpus(7, 2400)
    changed = fewer = pressed = 0
    for band_i, band in enumerate((1, 2, 16)):
        for set_i, scores in enumerate(R.SCORE_SETS):
            part = cases[band_i * 4 + set_i:: 12]
            assert len(part) == 200
            for c, g in zip(part, host(part, scores, band)):
                want = R.realign(*c, scores, band)
                out = R.path_of(g["words"])
                assert same(g, want), (band, scores, R.show(c[0]), R.show(out), R.show(want[0]), g["score"], want[1])
                R.check_properties(*c, out, g["score"], scores, band)
                changed += out != c[0]
                fewer += R.gap_words(out) < R.gap_words(c[0])
                ds = [j - i for i, j in R.cells(out)]
                pressed += min(ds) == want[3] or max(ds) == want[4]
    # the data does what it is about: most paths change, many lose gap words, and the narrow bands are reached
    assert changed > 1200 and fewer > 200 and pressed > 20, (changed, fewer, pressed)


def test_rule_is_not_idempotent_and_says_so():
    """the band follows the input path, so a second pass can reach a path the first could not: the documented limit, on one example"""
    c = (R.parse("2I1X3=1D2X"), np.array([0, 1, 0, 0, 1, 0, 0, 0, 0], np.uint8), np.array([0, 0, 0, 0, 0, 1, 1, 1], np.uint8), 1)
    first = host([c], R.DEFAULT, 1)[0]
    again = host([(R.path_of(first["words"]), c[1], c[2], c[3])], R.DEFAULT, 1)[0]
    assert (R.show(R.path_of(first["words"])), first["score"], first["diag_lo"], first["diag_hi"]) == ("1X2=1D2=1X2I", -14, -3, 1)
    assert (R.show(R.path_of(again["words"])), again["score"], again["diag_lo"], again["diag_hi"]) == ("1D2=1D3=3I", -12, -2, 2)
    assert same(first, R.realign(*c, R.DEFAULT, 1))


def test_bad_jobs_and_options_are_refused():
    ref = np.array(list(b"AAAAAAAACG"), dtype=np.uint8)
    qry = np.array(list(b"AAAAAAACG"), dtype=np.uint8)
    words = R.words_of(R.parse("7=1D2=") + [(4, 3), (7, 0)])             # a soft clip and a zero-length word behind the path
    good = (0, 3, 0, 10, 0, 0, 9)
    assert [R.show(R.path_of(g["words"])) for g in F.realign(ref, qry, words, [good])] == ["7=1D2="]
    bad = {"outside its pools": [(0, 6, 0, 10, 0, 0, 9), (0, 3, 1, 10, 0, 0, 9), (0, 3, 0, 10, 0, 1, 9), (1 << 40, 1, 0, 10, 0, 0, 9)],
           "other than = X I D": [(3, 1, 0, 10, 0, 0, 9)],
           "length 0": [(4, 1, 0, 10, 0, 0, 9)],
           "do not fit": [(0, 3, 0, 9, 0, 0, 9), (0, 3, 0, 10, 1, 0, 9), (0, 3, 0, 10, 0, 0, 8)]}
    for msg, jobs in bad.items():
        for j in jobs:
            with pytest.raises(F.FloxerError, match=msg):
                F.realign(ref, qry, words, [good, j])
    assert F.realign(ref, qry, words, []) == [] and [len(g["words"]) for g in F.realign(ref, qry, words, [(0, 0, 0, 0, 0, 0, 0)])] == [0]
    # the options: every bound, judged before anything else (the batch seam: before the context is looked at)
    L = capi.lib()
    job = (capi.RealignJob * 1)(capi.RealignJob(0, 3, 0, 0, 10, 0, 0, 9, 0))
    out = np.zeros(8, dtype=np.uint32)
    res = (capi.RealignResult * 1)()

    def call(o, n, batch=False):
        args = (capi.ptr(ref, capi.u8p), 10, capi.ptr(qry, capi.u8p), 9, capi.ptr(words, capi.u32p), len(words), job, 1,
                C.byref(o) if o is not None else None, capi.ptr(out, capi.u32p), C.byref(n), res)
        return L.flx_realign_batch(None, *args) if batch else L.flx_realign(*args)

    refusals = [(dict(enable=2), b"enable must be 0 or 1"), (dict(match=256), b"a score above 255"), (dict(mismatch=256), b"a score above 255"),
                (dict(gap_open=256), b"a score above 255"), (dict(gap_extend=256), b"a score above 255"), (dict(band=1025), b"band above 1024"),
                (dict(match=1, mismatch=16, gap_open=1, gap_extend=1), b"must not exceed 8"), (dict(gap_open=200, gap_extend=200), b"must not exceed 8")]
    for fields, msg in refusals:
        o = F.realign_options()
        for k, v in fields.items():
            setattr(o, k, v)
        for batch in (False, True):
            n = C.c_uint64(8)
            assert call(o, n, batch) == -1 and msg in L.flx_last_error(), (fields, batch, L.flx_last_error())
    for k in range(2):
        o = F.realign_options()
        o.reserved[k] = 1
        assert call(o, C.c_uint64(8)) == -1 and b"reserved fields" in L.flx_last_error()
    # at the bounds it runs; enable = 0 and NULL are the defaults here: the call is the request
    for o in (F.realign_options(True, 255, 255, 255, 255, 1024), F.realign_options(True, 1, 15, 1, 1, 1), F.realign_options(False), None):
        n = C.c_uint64(8)
        assert call(o, n) == 0 and n.value == 3, L.flx_last_error()
    # capacity, reserved job fields, null arguments
    n = C.c_uint64(2)
    assert call(None, n) == -3 and n.value == 3 and b"too small" in L.flx_last_error()
    n = C.c_uint64(8)
    assert call(None, n) == 0 and (res[0].offset, res[0].length, res[0].num_errors, res[0].score, res[0].diag_lo, res[0].diag_hi, res[0].kept) == (0, 3, 1, 12, -16, 17, 0)
    job[0].reserved2 = 1
    assert call(None, n) == -1 and b"reserved" in L.flx_last_error() and n.value == 0
    job[0].reserved2 = 0
    assert call(None, n, batch=True) == -1 and b"null" in L.flx_last_error()
    assert L.flx_ctx_get_realign_counters(None, None) == -1
    # the batch seam behind K5 judges both structs before the context is looked at
    o = F.realign_options()
    o.band = 2000
    assert L.flx_align_batch_realign(None, None, 0, None, 0, None, 0, None, None, None, None, None, None, None, C.byref(o), None) == -1
    assert b"band above 1024" in L.flx_last_error()
    g = F.gap_options()
    g.reserved[0] = 1
    assert L.flx_align_batch_realign(None, None, 0, None, 0, None, 0, None, None, None, None, None, None, C.byref(g), None, None) == -1
    assert b"flx_gap_options: the reserved fields" in L.flx_last_error()
    assert L.flx_align_batch_realign(None, None, 0, None, 0, None, 0, None, None, None, None, None, None, None, C.byref(F.realign_options()), None) == -1
    assert b"flx_align_batch_realign: null argument" in L.flx_last_error()


def test_a_path_too_long_for_32_bits_is_kept():
    """(rows + columns + 2) * max(a, b, o + e) >= 2^29: the words come back as they are, flagged"""
    ln = (1 << 28) - 8
    words = np.array([(ln << 4) | R.D], dtype=np.uint32)
    ref = np.zeros(ln, dtype=np.uint8)
    g = F.realign(ref, np.zeros(0, np.uint8), words, [(0, 1, 0, ln, 0, 0, 0)], F.realign_options(True, 2, 4, 4, 2, 1))[0]
    assert (list(g["words"]), g["kept"], g["score"], g["num_errors"], g["diag_lo"], g["diag_hi"]) == ([int(words[0])], 1, 0, ln, -1, ln + 1)


def test_struct_layouts_exported_symbols_and_defaults():
    assert C.sizeof(capi.RealignOptions) == 32 and C.sizeof(capi.RealignResult) == 32 and C.sizeof(capi.RealignCounters) == 64
    assert [getattr(capi.RealignOptions, f).offset for f in ("enable", "match", "mismatch", "gap_open", "gap_extend", "band", "reserved")] == [0, 4, 8, 12, 16, 20, 24]
    assert [getattr(capi.RealignResult, f).offset for f in ("offset", "length", "num_errors", "score", "diag_lo", "diag_hi", "kept")] == [0, 8, 12, 16, 20, 24, 28]
    assert capi.RealignJob is capi.LeftAlignJob
    new = {"flx_realign", "flx_realign_batch", "flx_align_batch_realign", "flx_ctx_get_realign_counters"}
    assert set(capi.EXPORTED) >= new
    for name in capi.EXPORTED:
        assert hasattr(capi.lib(), name), name
    o = F.realign_options()
    assert (o.enable, o.match, o.mismatch, o.gap_open, o.gap_extend, o.band, list(o.reserved)) == (1, 0, 0, 0, 0, 0, [0, 0])
    assert F.REALIGN_DEFAULTS == dict(match=2, mismatch=4, gap_open=4, gap_extend=2, band=16)
    # a zeroed field is its default: the same words as the defaults spelled out
    c = R.random_corpus(3, 20)
    ref, qry, words, jobs = R.pack_jobs(c)
    a = F.realign(ref, qry, words, jobs, None)
    b = F.realign(ref, qry, words, jobs, F.realign_options(True, 2, 4, 4, 2, 16))
    assert all(list(x["words"]) == list(y["words"]) and x["score"] == y["score"] for x, y in zip(a, b))


def test_rule_header_against_full_matrices_under_sanitizers(tmp_path):
    """tests/realign_check.cpp: flx_realign.hpp on random paths, built with ASan + UBSan"""
    exe = str(tmp_path / "realign_check")
    src = os.path.join(ROOT, "tests", "realign_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------ whole runs, the writer, the CLI
def test_run_calls_refuse_bad_options_and_without_cigar_before_any_work():
    """flx_align_reads_realign / _resident_realign judge the options first: no context, no reads, no launch"""
    L = capi.lib()
    assert {"flx_align_reads_realign", "flx_align_reads_resident_realign", "flx_run_copy_scores", "flx_sam_write_scored"} <= set(capi.EXPORTED)
    p = F.params(error_probability=0.05, without_cigar=True)
    run = C.c_void_p()
    for o, msg in ((F.realign_options(), b"flx_realign_options.enable needs the CIGAR's trace"), (F.realign_options(band=1025), b"band above 1024"),
                   (F.realign_options(match=1, mismatch=16, gap_open=1, gap_extend=1), b"must not exceed 8")):
        assert L.flx_align_reads_realign(None, C.byref(p), None, None, 0, None, None, None, C.byref(o), C.byref(run)) == -1
        assert msg in L.flx_last_error(), L.flx_last_error()
        assert L.flx_align_reads_resident_realign(None, C.byref(p), None, None, None, None, C.byref(o), C.byref(run)) == -1
        assert msg in L.flx_last_error(), L.flx_last_error()
    o = F.realign_options()
    o.enable = 2
    assert L.flx_align_reads_realign(None, C.byref(F.params(error_probability=0.05)), None, None, 0, None, None, None, C.byref(o), C.byref(run)) == -1
    assert b"enable must be 0 or 1" in L.flx_last_error()
    assert L.flx_run_copy_scores(None, None) == -1


def _as_tags_of_bam(data):
    """[[(tag, type, value)]] per record of a BAM file's bytes, signed 32-bit values (type i) included"""
    import struct
    from test_md_host import bgzf_members
    data = b"".join(bgzf_members(data))
    off = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref = struct.unpack_from("<i", data, off)[0]
    off += 4
    for _ in range(n_ref):
        off += 4 + struct.unpack_from("<i", data, off)[0] + 4
    out = []
    while off < len(data):
        bs, _, _, l_name, _, _, n_cig, _, l_seq = struct.unpack_from("<iiiBBHHHi", data, off)
        at, end, tags = off + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq, off + 4 + bs, []
        while at < end:
            tag, ty = data[at: at + 2].decode(), chr(data[at + 2])
            at += 3
            if ty == "Z":
                z = data.index(b"\0", at)
                tags.append((tag, ty, data[at:z]))
                at = z + 1
            else:
                size = {"C": 1, "S": 2, "I": 4, "i": 4}[ty]
                tags.append((tag, ty, int.from_bytes(data[at: at + size], "little", signed=ty == "i")))
                at += size
        assert at == end
        out.append(tags)
        off = end
    return out


def test_writer_as_tag_sam_and_bam(tmp_path):
    from test_md_host import CIG, MD_BYTES, MD_REFS, ROWS, _md_refs, _records
    L = capi.lib()
    scores = np.array([8, -3, -3, 77, -2147483648], dtype=np.int32)      # (the unmapped record's 77 is never written)

    def write(path, md, sc, threads=1):
        ref_ids = (C.c_char_p * 2)(b"chrA", b"chrB")
        ref_lens = np.array([100000, 5000], dtype=np.uint64)
        pool = np.array([1, 2, 3, 4, 1, 2, 3, 4, 4, 3, 2, 1], dtype=np.uint8)
        offs = np.array([0, 4, 8, 12], dtype=np.uint64)
        ids = (C.c_char_p * 3)(b"r0", b"r1", b"r2")
        quals = (C.c_char_p * 3)(b"IIII", b"JJJJ", b"")
        cig = np.asarray(CIG, dtype=np.uint32)
        mdb = np.frombuffer(MD_BYTES + b"\0", dtype=np.uint8)
        w = C.c_void_p()
        capi.check(L.flx_sam_open(path.encode(), ref_ids, capi.ptr(ref_lens, capi.u64p), 2, C.byref(w)))
        capi.check(L.flx_sam_set_threads(w, threads))
        args = [w, ids, capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), quals, _records(ROWS), len(ROWS), capi.ptr(cig, capi.u32p),
                _md_refs(MD_REFS) if md else None, capi.ptr(mdb, capi.u8p)]
        if isinstance(sc, str):
            rc = L.flx_sam_write_tagged(*args)
        else:
            rc = L.flx_sam_write_scored(*args, sc.ctypes.data_as(C.POINTER(C.c_int32)) if sc is not None else None)
        L.flx_sam_close(w)
        assert rc == 0
        return open(path, "rb").read()

    for ext in ("sam", "bam"):
        p = lambda n: str(tmp_path / f"{n}.{ext}")
        for md in (False, True):
            assert write(p("null"), md, None) == write(p("tagged"), md, "tagged")          # scores NULL is flx_sam_write_tagged
        got, got_md = write(p("as"), False, scores), write(p("asmd"), True, scores)
        assert write(p("as2"), True, scores, threads=3) == got_md
        if ext == "sam":
            body = lambda b: [l.split("\t") for l in b.decode().splitlines() if not l.startswith("@")]
            assert [f[11:] for f in body(got)] == [["NM:i:0", "AS:i:8"], ["NM:i:1", "AS:i:-3"], ["NM:i:1", "AS:i:-3"], [], ["NM:i:0", "AS:i:-2147483648"]]
            assert [f[11:] for f in body(got_md)] == [["NM:i:0", "MD:Z:4", "AS:i:8"], ["NM:i:1", "MD:Z:2A1", "AS:i:-3"], ["NM:i:1", "MD:Z:2A1", "AS:i:-3"], [],
                                                      ["NM:i:0", "AS:i:-2147483648"]]
            assert [f[:11] for f in body(got)] == [f[:11] for f in body(write(p("plain"), False, None))]
        else:
            assert [[(t, v) for t, _, v in r] for r in _as_tags_of_bam(got)] == [[("NM", 0), ("AS", 8)], [("NM", 1), ("AS", -3)], [("NM", 1), ("AS", -3)], [],
                                                                                 [("NM", 0), ("AS", -2147483648)]]
            assert [[(t, v) for t, _, v in r] for r in _as_tags_of_bam(got_md)] == [[("NM", 0), ("MD", b"4"), ("AS", 8)], [("NM", 1), ("MD", b"2A1"), ("AS", -3)],
                                                                                    [("NM", 1), ("MD", b"2A1"), ("AS", -3)], [], [("NM", 0), ("AS", -2147483648)]]
            assert all(ty == "i" for r in _as_tags_of_bam(got) for t, ty, _ in r if t == "AS")


def test_cli_flags(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    base = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"),
            "--output", str(tmp_path / "o.sam"), "-e", "2"]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0
    flags = ["--realign-affine", "--realign-match", "--realign-mismatch", "--realign-gap-open", "--realign-gap-extend", "--realign-band"]
    for fl in flags:
        line = [l for l in h.stderr.decode().splitlines() if l.strip().startswith(fl + " ")]
        assert len(line) == 1 and line[0].startswith("      --") and "not floxer's" in line[0], fl             # long spelling only
    env = dict(os.environ, FLX_CLI_PARSE_ONLY="1")               # the options are parsed, then only the reader runs (no GPU)
    good = (["--realign-affine"], ["--realign-affine", "--md-tag", "-Q", "-D", "-N", "2", "--left-align-indels"],
            ["--realign-affine", "--partial-alignments", "-N", "1", "--split-tails", "--partial-extend", "--sa-tag"],
            ["--realign-affine", "--realign-match", "1", "--realign-mismatch", "15", "--realign-gap-open", "1", "--realign-gap-extend", "1", "--realign-band", "1024"],
            ["--realign-affine", "--realign-match=255", "--realign-mismatch=255", "--realign-gap-open=255", "--realign-gap-extend=255"])
    for extra in good:
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and b"CLI PARSER ERROR" not in r.stderr, (extra, r.stderr)
    bad = (["--realign-affine", "-w"], ["--without-cigar", "--realign-affine"], ["--realign"], ["--realign-affine", "x"],
           ["--realign-band", "8"], ["--realign-match", "2"], ["--realign-mismatch", "2"], ["--realign-gap-open", "2"], ["--realign-gap-extend", "2"],
           ["--realign-affine", "--realign-match", "0"], ["--realign-affine", "--realign-match", "256"], ["--realign-affine", "--realign-band", "1025"],
           ["--realign-affine", "--realign-gap-extend", "256"], ["--realign-affine", "--realign-band"],
           ["--realign-affine", "--realign-match", "1", "--realign-mismatch", "16", "--realign-gap-open", "1", "--realign-gap-extend", "1"])
    for extra in bad:
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr, extra
