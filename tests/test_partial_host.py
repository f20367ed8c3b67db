"""Partial alignments without a GPU: the selection rule (flx_choose_partials) on hand-made candidate arrays, the writer on
soft-clipped and supplementary records (SAM and BAM parsed back here), and how the option meets -D, -N, -Q and -w."""
import ctypes as C
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
from test_output_options_host import to_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQ, X, INS, DEL, S = 7, 8, 1, 2, 4


def w(n, op):
    return n << 4 | op


# candidate rows: (read, q_from, q_to, orientation, reference, start, nm, cigar offset, cigar length)
def choose(rows, cigars=None, **kw):
    return F.choose_partials(rows, cigars, F.partial_options(**kw) if kw else None).tolist()


# ------------------------------------------------------------------------------------------------ the selection rule
def test_struct_layouts_and_exported_symbols():
    assert C.sizeof(capi.PartialOptions) == 32 and C.sizeof(capi.PartialCandidate) == 48 and C.sizeof(capi.RunOptions) == 64
    assert capi.PartialCandidate.start.offset == 24 and capi.PartialCandidate.cigar_offset.offset == 40
    assert set(capi.EXPORTED) >= {"flx_align_reads_opt", "flx_align_reads_resident_opt", "flx_choose_partials", "flx_partial_mapq"}
    for name in capi.EXPORTED:
        assert hasattr(capi.lib(), name), name
    o = F.partial_options()
    assert (o.enable, o.min_query_span, o.max_records, list(o.reserved)) == (1, 0, 0, [0] * 5)


def test_order_is_rows_then_nm_then_reference_then_verification_order():
    # the longest first whatever its NM; of two of equal rows the smaller NM; then the smaller reference id; then the earlier one
    rows = [(0, 0, 999, 0, 1, 50, 9, 0, 1),        # 1000 rows, nm 9
            (0, 1000, 2999, 0, 1, 90, 30, 1, 1),   # 2000 rows: the primary although its NM is the largest
            (0, 3000, 3999, 0, 1, 10, 9, 2, 1)]    # 1000 rows
    assert choose(rows) == [2048, 0, 2048]
    rows = [(0, 0, 999, 0, 0, 50, 9, 0, 1), (0, 0, 999, 0, 0, 9000, 8, 1, 1)]
    assert choose(rows) == [-1, 0]                                       # NM decides between equal rows
    rows = [(0, 0, 999, 0, 1, 50, 8, 0, 1), (0, 0, 999, 0, 0, 9000, 8, 1, 1)]
    assert choose(rows) == [-1, 0]                                       # then the reference id
    rows = [(0, 0, 999, 0, 0, 50, 8, 0, 1), (0, 0, 999, 1, 0, 9000, 8, 1, 1)]
    assert choose(rows) == [0, -1]                                       # then the verification order, whatever the strand
    # reads are separate: each has a primary of its own
    rows = [(3, 0, 999, 0, 0, 50, 8, 0, 1), (4, 0, 999, 1, 0, 9000, 8, 1, 1), (4, 1000, 1200, 0, 0, 7, 0, 2, 1)]
    assert choose(rows) == [0, 16, 2048]


def test_overlap_is_judged_in_forward_coordinates_across_strands():
    # (the caller turns node [from, to] of the reverse complement into [len-1-to, len-1-from]: the array holds forward intervals)
    rows = [(0, 0, 1999, 0, 0, 100, 5, 0, 1), (0, 1999, 2999, 1, 0, 70000, 0, 1, 1), (0, 2000, 2999, 1, 0, 70000, 1, 2, 1)]
    assert choose(rows) == [0, -1, 2064]                                 # one shared base is an overlap; abutting intervals are not
    rows = [(0, 500, 2499, 1, 2, 100, 5, 0, 1), (0, 0, 499, 0, 0, 7, 2, 1, 1), (0, 400, 600, 0, 0, 9, 0, 2, 1), (0, 2500, 2999, 0, 1, 3, 0, 3, 1)]
    assert choose(rows) == [16, 2048, -1, 2048]


def test_max_records_and_its_default():
    rows = [(0, 1000 * i, 1000 * i + 999 - i, 0, 0, 10 * i, 0, i, 1) for i in range(6)]      # rows 1000, 999, ..: taken in this order
    assert choose(rows) == [0, 2048, 2048, 2048, -1, -1]                 # the default: 4
    assert choose(rows, max_records=0) == [0, 2048, 2048, 2048, -1, -1]
    assert choose(rows, max_records=1) == [0, -1, -1, -1, -1, -1]
    assert choose(rows, max_records=6) == [0] + [2048] * 5
    assert choose(rows, max_records=2, min_query_span=5000) == [0, 2048, -1, -1, -1, -1]     # (the span filters candidates before they are traced)


def test_duplicates_compare_cigar_words():
    cig = np.array([w(1000, EQ), w(1000, EQ), w(999, EQ), w(1, X)], dtype=np.uint32)
    # equal in strand, reference, start, NM and words (at another offset): dropped, whatever its interval
    rows = [(0, 0, 999, 0, 0, 100, 0, 0, 1), (0, 1000, 1999, 0, 0, 100, 0, 1, 1)]
    assert choose(rows, cig) == [0, -1]
    assert choose(rows) == [0, 2048]                                     # without words CIGARs compare by (offset, length)
    for change in ({3: 1}, {4: 1}, {5: 101}, {6: 1}):                    # another strand / reference / start / NM: not a duplicate
        other = list(rows[1])
        for k, v in change.items():
            other[k] = v
        assert choose([rows[0], tuple(other)], cig)[1] in (2048, 2064), change
    rows = [(0, 0, 999, 0, 0, 100, 1, 0, 1), (0, 1000, 1999, 0, 0, 100, 1, 2, 2)]            # other words
    assert choose(rows, cig) == [0, 2048]


def test_options_are_checked():
    rows = [(0, 0, 999, 0, 0, 100, 0, 0, 1)]
    o = F.partial_options()
    o.enable = 2
    with pytest.raises(F.FloxerError, match="enable"):
        F.choose_partials(rows, None, o)
    for k in range(5):
        o = F.partial_options()
        o.reserved[k] = 1
        with pytest.raises(F.FloxerError, match="reserved"):
            F.choose_partials(rows, None, o)
    with pytest.raises(F.FloxerError):
        F.partial_options(min_query_span=-1)


# ------------------------------------------------------------------------------------------------ the writer
READ_LEN = [40, 12, 30]


def _write(path, rows, cig, threads=1, md=None):
    L = capi.lib()
    ref_ids = (C.c_char_p * 2)(b"chrA", b"chrB")
    ref_lens = np.array([100000, 50000], dtype=np.uint64)
    rng = np.random.default_rng(5)
    pool = rng.integers(1, 5, size=sum(READ_LEN), dtype=np.uint8)
    offs = np.cumsum([0] + READ_LEN).astype(np.uint64)
    ids = (C.c_char_p * 3)(b"r0", b"r1", b"r2")
    quals = (C.c_char_p * 3)(b"I" * 40, b"J" * 12, b"")
    recs = (capi.Record * len(rows))()
    for i, r in enumerate(rows):
        recs[i] = capi.Record(*r)
    h = C.c_void_p()
    capi.check(L.flx_sam_open(path.encode(), ref_ids, capi.ptr(ref_lens, capi.u64p), 2, C.byref(h)))
    capi.check(L.flx_sam_set_threads(h, threads))
    if md is None:
        rc = L.flx_sam_write(h, ids, capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), quals, recs, len(rows), capi.ptr(cig, capi.u32p))
    else:
        refs = (capi.MdRef * len(rows))()
        blob = b""
        for i, m in enumerate(md):
            refs[i] = capi.MdRef(len(blob), len(m), 0)
            blob += m
        buf = np.frombuffer(blob, dtype=np.uint8).copy()
        rc = L.flx_sam_write_tagged(h, ids, capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), quals, recs, len(rows), capi.ptr(cig, capi.u32p),
                                    refs, capi.ptr(buf, capi.u8p))
    capi.check(L.flx_sam_close(h))
    assert rc == 0, capi.lib().flx_last_error()
    return "".join("$ACGTN"[x] for x in pool), offs


def _bam(path):
    data = gzip.open(path, "rb").read()
    off = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref = struct.unpack_from("<i", data, off)[0]
    off += 4
    for _ in range(n_ref):
        off += 4 + struct.unpack_from("<i", data, off)[0] + 4
    out = []
    while off < len(data):
        bs, ref_id, pos, l_name, mapq, bin_, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", data, off)
        at = off + 36 + l_name
        words = struct.unpack_from(f"<{n_cig}I", data, at)
        at += 4 * n_cig
        seq = "".join("=ACMGRSVTWYHKDBN"[(data[at + (b >> 1)] >> (4 if b % 2 == 0 else 0)) & 15] for b in range(l_seq))
        at += (l_seq + 1) // 2 + l_seq
        out.append(dict(ref=ref_id, pos=pos, bin=bin_, flag=flag, l_seq=l_seq, seq=seq, tags=data[at: off + 4 + bs],
                        cigar="".join(f"{x >> 4}{'MIDNSHP=X'[x & 15]}" for x in words)))
        off += 4 + bs
    return out


def _reg2bin(beg, end):
    end -= 1
    for shift, base in [(14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)]:
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def _writer_case():
    # r0 (40 bases): primary 5S 30= 1X 1= 3S at 16350 (its 32 aligned columns end below 16384, the 16-kb bin boundary; 40 would not)
    # and a supplementary on the other strand with a leading clip only; r1 unmapped; r2 (30 bases) a primary with a trailing clip only
    cig = np.array([w(5, S), w(30, EQ), w(1, X), w(1, EQ), w(3, S),
                    w(8, S), w(10, EQ), w(2, DEL), w(22, EQ),
                    w(20, EQ), w(2, INS), w(4, EQ), w(4, S)], dtype=np.uint32)
    #        read flag       ref pos    nm coff clen reserved
    rows = [(0, 0,          0, 16350, 1, 0, 5, 0),
            (0, 2048 | 16,  1, 700,   2, 5, 4, 0),
            (1, 4,         -1, 0,     0, 0, 0, 0),
            (2, 16,         0, 16370, 2, 9, 4, 0)]
    want = [dict(flag=0, ref=0, pos=16350, cigar="5S30=1X1=3S", span=32, read=0, nm=1),
            dict(flag=2064, ref=1, pos=700, cigar="8S10=2D22=", span=34, read=0, nm=2),
            dict(flag=4, ref=-1, pos=0, cigar="", span=0, read=1, nm=None),
            dict(flag=16, ref=0, pos=16370, cigar="20=2I4=4S", span=24, read=2, nm=2)]
    return cig, rows, want


def test_writer_soft_clips_and_supplementary_flag_in_sam_and_bam(tmp_path):
    cig, rows, want = _writer_case()
    md = [b"30A1", b"10^AC22", b"", b"24"]
    for tagged in (False, True):
        files = {}
        for ext in ("sam", "bam"):
            for threads in (1, 3):
                path = str(tmp_path / f"t{int(tagged)}_{threads}.{ext}")
                letters, offs = _write(path, rows, cig, threads, md if tagged else None)
                files[ext, threads] = open(path, "rb").read()
            assert files[ext, 1] == files[ext, 3]                        # bytes do not depend on the writer's thread count
        body = [l.split("\t") for l in files["sam", 1].decode().splitlines() if not l.startswith("@")]
        bam = _bam(str(tmp_path / f"t{int(tagged)}_1.bam"))
        assert len(body) == len(bam) == len(want)
        for f, b, e, m in zip(body, bam, want, md):
            seq = letters[int(offs[e["read"]]): int(offs[e["read"] + 1])]
            assert (int(f[1]), f[2], int(f[3]), f[5]) == (e["flag"], "*" if e["ref"] < 0 else ["chrA", "chrB"][e["ref"]], e["pos"] + 1, e["cigar"] or "*")
            assert f[9] == seq                                           # a supplementary record with soft clips carries the whole read
            assert (b["flag"], b["ref"], b["pos"], b["cigar"], b["l_seq"], b["seq"]) == (e["flag"], e["ref"], e["pos"], e["cigar"], READ_LEN[e["read"]], seq)
            assert b["bin"] == _reg2bin(e["pos"], e["pos"] + max(1, e["span"]))      # from the aligned span: clips consume no reference
            if e["nm"] is None:
                assert len(f) == 11 and b["tags"] == b""
            else:
                assert f[11] == f"NM:i:{e['nm']}" and b["tags"][:4] == b"NMC" + bytes([e["nm"]])
                assert (f[12:] == ["MD:Z:" + m.decode()] and b["tags"][4:] == b"MDZ" + m + b"\0") if tagged else (len(f) == 12 and len(b["tags"]) == 4)
        # the first record's clips decide nothing: 16350 + 32 stays in the 16-kb bin, 16350 + 40 would not
        assert bam[0]["bin"] == 4681 and _reg2bin(16350, 16390) != 4681


def test_writer_long_cigar_placeholder_with_clips(tmp_path):
    """more than 65535 operations: the record carries <l_seq>S<span>N and the real CIGAR, clips included, in CG:B,I"""
    n = 33000
    words = [w(3, S)] + [w(1, EQ), w(1, X)] * n + [w(7, S)]
    cig = np.array(words, dtype=np.uint32)
    path = str(tmp_path / "long.bam")
    L = capi.lib()
    ref_ids = (C.c_char_p * 1)(b"chrA")
    ref_lens = np.array([1000000], dtype=np.uint64)
    pool = np.ones(2 * n + 10, dtype=np.uint8)
    offs = np.array([0, 2 * n + 10], dtype=np.uint64)
    ids = (C.c_char_p * 1)(b"r0")
    recs = (capi.Record * 1)(capi.Record(0, 2048, 0, 500, n, 0, len(words), 0))
    h = C.c_void_p()
    capi.check(L.flx_sam_open(path.encode(), ref_ids, capi.ptr(ref_lens, capi.u64p), 1, C.byref(h)))
    capi.check(L.flx_sam_write(h, ids, capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), None, recs, 1, capi.ptr(cig, capi.u32p)))
    capi.check(L.flx_sam_close(h))
    (b,) = _bam(path)
    assert b["flag"] == 2048 and b["l_seq"] == 2 * n + 10 and b["cigar"] == f"{2 * n + 10}S{2 * n}N" and b["bin"] == _reg2bin(500, 500 + 2 * n)
    tag = b["tags"][b["tags"].index(b"CGBI"):]
    assert struct.unpack_from("<i", tag, 4)[0] == len(words) and struct.unpack_from(f"<{len(words)}I", tag, 8) == tuple(words)


# ------------------------------------------------------------------------------------------------ with the other options
def test_drop_duplicates_and_max_alignments_leave_partial_records_alone():
    rng = np.random.default_rng(8)
    part = (w(5, S), w(30, EQ), w(5, S))
    rows = [(0, 0, 0, 100, 0, (w(40, EQ),)), (0, 256, 0, 100, 0, (w(40, EQ),)), (0, 256, 1, 7, 3, (w(40, EQ),)),       # an ordinary read
            (1, 16, 0, 500, 2, part), (1, 2048, 1, 900, 0, part), (1, 2064, 1, 900, 0, part),                           # partial records
            (2, 4, -1, 0, 0, ())]
    run = to_run(rows, rng)
    assert F.select_records(run, F.output_options(True, 0)).tolist() == [True, False, True, True, True, True, True]
    assert F.select_records(run, F.output_options(False, 1)).tolist() == [True, False, False, True, True, True, True]
    assert F.select_records(run, F.output_options(True, 1, True)).tolist() == [True, False, False, True, True, True, True]


def _mapq(rows, cigars, flags):
    arr = (capi.PartialCandidate * len(rows))()
    for a, c in zip(arr, rows):
        a.read_index, a.q_from, a.q_to, a.orientation, a.reference_id, a.start, a.nm, a.cigar_offset, a.cigar_length = c
    fl = np.array(flags, dtype=np.int32)
    out = np.zeros(len(rows), dtype=np.uint8)
    capi.check(capi.lib().flx_partial_mapq(arr, len(rows), capi.ptr(cigars, capi.u32p) if cigars is not None else None,
                                           fl.ctypes.data_as(C.POINTER(C.c_int32)), capi.ptr(out, capi.u8p)))
    return out.tolist()


def test_mapping_quality_of_kept_candidates():
    """each kept record: read_mapq over the candidates with exactly its forward interval (flx_mapq.hpp: one locus 60; n loci of the
    best NM 3, 2, 1, 0; else min(60, 10 * (next NM - best NM)))"""
    cig = np.array([w(2000, EQ), w(1000, EQ)], dtype=np.uint32)
    rows = [(0, 0, 1999, 0, 0, 5000, 4, 0, 1),       # kept primary; its interval has three more candidates:
            (0, 0, 1999, 0, 0, 5100, 6, 0, 1),       #   the same locus (overlaps on the reference)
            (0, 0, 1999, 0, 1, 5000, 7, 0, 1),       #   another locus, 3 errors more
            (0, 0, 1999, 1, 0, 5000, 9, 0, 1),       #   another strand: another locus
            (0, 2000, 2999, 1, 0, 90000, 2, 1, 1),   # kept supplementary, alone on its interval
            (0, 1990, 2999, 0, 0, 7000, 0, 1, 1)]    # not kept, another interval: tells nothing about either
    flags = choose(rows, cig)
    assert flags == [0, -1, -1, -1, 2064, -1]
    assert _mapq(rows, cig, flags) == [30, 0, 0, 0, 60, 0]
    # two loci of the best NM on the primary's interval: 3; a unique one whatever else the read has: 60
    rows2 = [rows[0], (0, 0, 1999, 0, 1, 300, 4, 0, 1), rows[4]]
    assert _mapq(rows2, cig, choose(rows2, cig)) == [3, 0, 60]
    # a duplicate of the kept record (other offset, the same words) is no second locus
    cig3 = np.array([w(2000, EQ), w(2000, EQ)], dtype=np.uint32)
    rows3 = [(0, 0, 1999, 0, 0, 5000, 4, 0, 1), (0, 0, 1999, 0, 0, 5000, 4, 1, 1)]
    assert choose(rows3, cig3) == [0, -1] and _mapq(rows3, cig3, [0, -1]) == [60, 0]


def test_without_cigar_is_refused_before_any_work(tmp_path):
    L = capi.lib()
    p = F.params(error_probability=0.05, without_cigar=True)
    bundle = capi.RunOptions()
    part = F.partial_options()
    bundle.partial = C.pointer(part)
    run = C.c_void_p()
    pool = np.ones(8, dtype=np.uint8)
    offs = np.array([0, 8], dtype=np.uint64)
    # (no context at all: the options are judged first)
    assert L.flx_align_reads_opt(None, C.byref(p), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), 1, C.byref(bundle), C.byref(run)) == -1
    assert b"without_cigar" in L.flx_last_error() and b"flx_partial_options" in L.flx_last_error()
    assert L.flx_align_reads_resident_opt(None, C.byref(p), None, C.byref(bundle), C.byref(run)) == -1
    assert b"without_cigar" in L.flx_last_error()
    part.enable = 0                                                     # switched off: the refusal is the null context's, not the option's
    assert L.flx_align_reads_resident_opt(None, C.byref(p), None, C.byref(bundle), C.byref(run)) == -1
    assert b"without_cigar" not in L.flx_last_error()
    part.enable = 3
    p.without_cigar = 0
    assert L.flx_align_reads_resident_opt(None, C.byref(p), None, C.byref(bundle), C.byref(run)) == -1 and b"enable" in L.flx_last_error()
    part.enable = 1
    bundle.reserved[2] = 1
    assert L.flx_align_reads_resident_opt(None, C.byref(p), None, C.byref(bundle), C.byref(run)) == -1 and b"reserved pointers" in L.flx_last_error()


def test_cli_flags(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    base = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"),
            "--output", str(tmp_path / "o.sam"), "-e", "2"]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0
    for name in ("--partial-alignments", "--partial-min-span <value>", "--partial-max <value>"):
        line = [l for l in h.stderr.decode().splitlines() if l.strip().startswith(name)]
        assert len(line) == 1 and line[0].startswith("      --") and "not floxer's" in line[0], name        # long spellings only
    env = dict(os.environ, FLX_CLI_PARSE_ONLY="1")               # the options are parsed, then only the reader runs (no GPU)
    for extra in (["--partial-alignments"], ["--partial-alignments", "--partial-min-span", "500", "--partial-max=2"],
                  ["--partial-alignments", "-D", "-N", "1", "-Q", "--md-tag", "-I"], ["--partial-alignments", "-d"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and b"CLI PARSER ERROR" not in r.stderr, (extra, r.stderr)
    for extra in (["--partial-alignments", "-w"], ["--partial-min-span", "500"], ["--partial-max", "2"],
                  ["--partial-alignments", "--partial-min-span", "0"], ["--partial-alignments", "--partial-max", "x"], ["--partial"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr, extra
