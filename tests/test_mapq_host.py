"""Mapping quality without a GPU: flx_assign_mapq (the rule the record stage applies to every read's records when
flx_output_options.mapq is set) against a plain-Python restatement of it, the options' validation, the writer's MAPQ column in SAM
and BAM, and the CLI's flag."""
import ctypes as C
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
from test_output_options_host import random_read, to_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cigar_span(cig):
    """reference symbols a CIGAR covers; cig: BAM words, or a string of '=', 'X', 'I', 'D' operations"""
    if isinstance(cig, str):
        import re
        return sum(int(n) for n, op in re.findall(r"(\d+)([=XIDM])", cig) if op in "=XD")
    return sum(int(w) >> 4 for w in cig if int(w) & 15 in (7, 8, 2))


def _read_loci(rows, i, j, read_lengths):
    """the loci of the read whose records are rows[i:j]: [[record indices], NM], by the sweep of flx_mapq.hpp"""
    recs = []
    for t in range(i, j):
        read, flag, ref, pos, nm, cig = rows[t]
        if flag & 4:
            continue
        if len(cig) == 0 or cig == "*":
            span = int(read_lengths[read]) if read_lengths is not None else 0
        else:
            span = cigar_span(cig)
        recs.append((ref, flag & 16, pos, t, pos + max(span, 1), nm))
    recs.sort()
    loci = []
    end = key = None
    for ref, strand, pos, t, stop, nm in recs:
        if key == (ref, strand) and pos < end:
            loci[-1][0].append(t)
            loci[-1][1] = min(loci[-1][1], nm)
            end = max(end, stop)
        else:
            loci.append([[t], nm])
            key, end = (ref, strand), stop
    return loci


def _reads_of(rows):
    i = 0
    while i < len(rows):
        j = i
        while j < len(rows) and rows[j][0] == rows[i][0]:
            j += 1
        yield i, j
        i = j


def loci_per_read(rows, read_lengths=None):
    """{read: number of loci} of the reads that have a mapped record"""
    return {rows[i][0]: len(_read_loci(rows, i, j, read_lengths)) for i, j in _reads_of(rows) if not rows[i][1] & 4}


def restate_mapq(rows, read_lengths=None):
    """the rule of flx_mapq.hpp in plain Python. rows: [(read, flag, ref, pos, nm, cigar words or string)] of whole reads, each
    read's records contiguous and in output order. A record whose CIGAR is empty ((), '' or '*') spans read_lengths[read] (None: 0).
    Returns one mapping quality per record."""
    out = [0] * len(rows)
    for i, j in _reads_of(rows):
        loci = _read_loci(rows, i, j, read_lengths)
        primary = [t for t in range(i, j) if not rows[t][1] & (4 | 256)]
        if primary:
            l0 = next(l for l in loci if primary[0] in l[0])
            b = l0[1]
            n = sum(1 for l in loci if l[1] == b)
            above = [l[1] for l in loci if l[1] > b]
            if n >= 2:
                q = {2: 3, 3: 2, 4: 1}.get(n, 0)
            elif len(loci) == 1:
                q = 60
            else:
                q = min(60, 10 * (min(above) - b)) if above else 0
            for t in l0[0]:
                out[t] = q
    return out


def loci_read(rng, read, n_refs, ties, gap, with_cigar=True):
    """a read whose loci are known by construction: `ties` loci of the best NM, then (gap > 0) one locus gap above it and a few
    further ones; every locus has one to four overlapping records, some nested, some sharing a start; loci are 1000 apart or
    abut (a record that starts where the one before ends: two loci)"""
    b = int(rng.integers(0, 4))
    nms = [b] * ties + ([b + gap] + [b + gap + int(x) for x in rng.integers(0, 5, size=int(rng.integers(0, 3)))] if gap else [])
    als = []
    at = [int(rng.integers(0, 500)) for _ in range(n_refs * 2)]
    for nm in nms:
        ref, strand = int(rng.integers(0, n_refs)), int(rng.integers(0, 2)) * 16
        slot = 2 * ref + (strand >> 4)
        start = at[slot]
        n_rec = int(rng.integers(1, 5))
        locus_end = start
        for k in range(n_rec):
            # '=' and 'X' and 'D' count for the span, 'I' does not; a span of 0 (insertions only) counts as 1
            words = [int(rng.integers(1, 30)) << 4 | int(rng.choice([7, 8, 2, 1])) for _ in range(int(rng.integers(1, 5)))]
            if rng.random() < 0.1:
                words = [int(rng.integers(1, 9)) << 4 | 1]
            pos = start if k == 0 else int(rng.integers(start, max(start + 1, locus_end)))      # inside the locus so far
            span = max(1, cigar_span(words)) if with_cigar else 1
            als.append([ref, strand, pos, nm if k == 0 else nm + int(rng.integers(0, 3)), tuple(words) if with_cigar else ()])
            locus_end = max(locus_end, pos + span)
        at[slot] = locus_end + (0 if rng.random() < 0.4 else 1000)                              # the next one abuts or is far
    order = rng.permutation(len(als))
    als = [als[k] for k in order]
    als.sort(key=lambda a: a[0])
    best = min(a[3] for a in als)
    out, primary = [], False
    for ref, strand, pos, nm, cig in als:
        flag = strand
        if not primary and nm == best:
            primary = True
        else:
            flag |= 256
        out.append((read, flag, ref, pos, nm, cig))
    return out


@pytest.mark.parametrize("with_cigar", [True, False])
def test_assign_mapq_matches_the_restatement(with_cigar):
    rng = np.random.default_rng(41 + with_cigar)
    seen = set()
    for trial in range(8):
        rows, want = [], []
        n_refs = 1 + trial % 3
        for read in range(80):
            kind = read % 4
            if kind == 0:
                rows += random_read(rng, read, n_refs, with_cigar)        # the output options' generator (unmapped-only reads too)
                want.append(None)
            else:
                ties = int(rng.choice([1, 1, 2, 3, 4, 5, 7]))
                gap = int(rng.integers(1, 9)) if ties == 1 and rng.random() < 0.8 else int(rng.integers(0, 3))
                rows += loci_read(rng, read, n_refs, ties, gap, with_cigar)
                want.append(60 if ties == 1 and gap == 0 else min(60, 10 * gap) if ties == 1 else {2: 3, 3: 2, 4: 1}.get(ties, 0))
        run = to_run(rows, rng)
        lens = rng.integers(1, 50, size=80) if trial % 2 else None
        got = F.assign_mapq(run, lens).tolist()
        exp = restate_mapq(rows, lens)
        assert got == exp, trial
        if with_cigar or lens is None:
            # the constructed reads get the quality their construction says (spans of CIGAR-less records are 1 without lengths)
            for read, w in enumerate(want):
                if w is not None:
                    qs = {exp[t] for t, r in enumerate(rows) if r[0] == read and not r[1] & 256}
                    assert qs == {w}, (trial, read)
                    seen.add(w)
        for t, r in enumerate(rows):
            if r[1] & 4:
                assert got[t] == 0
    assert seen >= {0, 1, 2, 3, 10, 20, 30, 40, 50, 60}


def test_assign_mapq_edge_cases():
    rng = np.random.default_rng(7)
    m = lambda n: (n << 4 | 7,)
    # abutting intervals are two loci, overlapping by one symbol is one; the strand and the reference separate loci
    rows = [(0, 0, 0, 100, 1, m(50)), (0, 256, 0, 150, 1, m(50)),                      # [100,150) [150,200): a tie of two
            (1, 0, 0, 100, 1, m(51)), (1, 256, 0, 150, 1, m(50)),                      # [100,151) [150,200): one locus
            (2, 0, 0, 100, 1, m(51)), (2, 256 | 16, 0, 150, 1, m(50)),                 # other strand: two loci
            (3, 0, 0, 100, 1, m(51)), (3, 256, 1, 150, 1, m(50)),                      # other reference: two loci
            (4, 4, -1, 0, 0, ()),                                                      # unmapped
            (5, 0, 0, 10, 2, m(100)), (5, 256, 0, 20, 5, m(10)), (5, 256, 0, 105, 9, m(10)), (5, 256, 0, 400, 4, m(10)),
            # read 5: [10,110) holds [20,30) and (by the running end, not the last record's end) [105,115): one locus, NM 2; s = 4
            (6, 0, 0, 10, 0, (5 << 4 | 1,)), (6, 256, 0, 11, 7, m(5)),                 # span 0 counts as 1: [10,11) and [11,16)
            (7, 0, 0, 10, 0, m(5)), (7, 256, 0, 500, 9, m(5))]                         # 10 * 9 is capped at 60
    run = to_run(rows, rng)
    got = F.assign_mapq(run).tolist()
    assert got == restate_mapq(rows)
    assert got == [3, 0, 60, 60, 3, 0, 3, 0, 0, 20, 20, 20, 0, 60, 0, 60, 0]
    # records without CIGAR: the read's length is the span; without lengths every span is 1
    rows = [(0, 0, 0, 100, 1, ()), (0, 256, 0, 130, 1, ()), (1, 0, 0, 100, 1, ()), (1, 256, 0, 130, 2, ())]
    run = to_run(rows, rng)
    assert F.assign_mapq(run, [31, 30]).tolist() == [60, 60, 10, 0] == restate_mapq(rows, [31, 30])
    assert F.assign_mapq(run).tolist() == [3, 0, 10, 0] == restate_mapq(rows)
    with pytest.raises(F.FloxerError):
        F.assign_mapq(run, [31])
    # record arrays the pipeline never forms: no primary, and a primary that is not the best
    rows = [(0, 256, 0, 100, 1, m(5)), (1, 0, 0, 100, 3, m(5)), (1, 256, 0, 200, 1, m(5))]
    run = to_run(rows, rng)
    assert F.assign_mapq(run).tolist() == [0, 0, 0] == restate_mapq(rows)
    assert F.assign_mapq(to_run([], rng)).tolist() == []
    # the result does not depend on what the records' reserved field holds
    rows = [(0, 0, 0, 100, 1, m(50)), (0, 256, 0, 150, 1, m(50))]
    run = to_run(rows, rng)
    run.raw["res"] = 77
    assert F.assign_mapq(run).tolist() == [3, 0]
    assert run.mapq.tolist() == [77, 77]


def test_output_options_mapq_field_validation():
    rng = np.random.default_rng(6)
    run = to_run([(0, 0, 0, 1, 0, (5 << 4 | 7,)), (0, 256, 0, 1, 0, (5 << 4 | 7,))], rng)
    assert C.sizeof(capi.OutputOptions) == 32 and capi.OutputOptions.mapq.offset == 4 and capi.OutputOptions.mapq.size == 4
    o = F.output_options(True, 1, True)
    assert (o.drop_duplicates, o.mapq, o.max_alignments_per_read) == (1, 1, 1)
    assert F.select_records(run, o).tolist() == [True, False]              # mapq = 1 is accepted and selects nothing by itself
    assert F.select_records(run, F.output_options(mapq=True)).tolist() == [True, True]
    o = F.output_options()
    assert (o.drop_duplicates, o.mapq, o.max_alignments_per_read, o.reserved2[0], o.reserved2[1]) == (0, 0, 0, 0, 0)
    assert F.select_records(run, o).tolist() == [True, True]               # zeroed options still select nothing
    o.mapq = 2
    with pytest.raises(F.FloxerError):
        F.select_records(run, o)
    for k in (0, 1):
        o = F.output_options(mapq=True)
        o.reserved2[k] = 1
        with pytest.raises(F.FloxerError):
            F.select_records(run, o)


def _write(path, recs, cig, mapq=None, threads=1, calls=None):
    """the records through flx_sam_open / flx_sam_write / flx_sam_close; mapq None: the setter is not called at all.
    calls: [(records, cigar words)] for several flx_sam_write calls on one writer (default: one call)"""
    L = capi.lib()
    ref_ids = (C.c_char_p * 2)(b"chrA", b"chrB")
    ref_lens = np.array([100000, 5000], dtype=np.uint64)
    pool = np.array([1, 2, 3, 4, 1, 2, 3, 4, 4, 3, 2, 1], dtype=np.uint8)
    offs = np.array([0, 4, 8, 12], dtype=np.uint64)
    ids = (C.c_char_p * 3)(b"r0", b"r1", b"r2")
    quals = (C.c_char_p * 3)(b"IIII", b"JJJJ", b"")
    w = C.c_void_p()
    capi.check(L.flx_sam_open(path.encode(), ref_ids, capi.ptr(ref_lens, capi.u64p), 2, C.byref(w)))
    capi.check(L.flx_sam_set_threads(w, threads))
    if mapq is not None:
        capi.check(L.flx_sam_set_mapq(w, mapq))
    rc = 0
    for r, c in calls if calls is not None else [(recs, cig)]:
        rc = rc or L.flx_sam_write(w, ids, capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), quals, r, len(r), capi.ptr(c, capi.u32p))
    L.flx_sam_close(w)
    return rc


def _records(rows):
    recs = (capi.Record * len(rows))()
    for i, r in enumerate(rows):
        recs[i] = capi.Record(*r)
    return recs


def _bam_records(path):
    data = gzip.open(path, "rb").read()
    off = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref = struct.unpack_from("<i", data, off)[0]
    off += 4
    for _ in range(n_ref):
        off += 4 + struct.unpack_from("<i", data, off)[0] + 4
    out = []
    while off < len(data):
        bs, ref_id, pos, l_name, mapq, bin_, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", data, off)
        out.append(dict(ref=ref_id, pos=pos, mapq=mapq, bin=bin_, flag=flag, name=data[off + 36: off + 36 + l_name - 1].decode()))
        off += 4 + bs
    return out


def _reg2bin(beg, end):
    end -= 1
    for shift, base in [(14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)]:
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def test_writer_mapq_column_sam_and_bam(tmp_path):
    cig = np.array([4 << 4 | 7, 2 << 4 | 7, 1 << 4 | 8, 1 << 4 | 7, 4 << 4 | 7], dtype=np.uint32)
    #        read flag ref pos   nm coff clen reserved
    rows = [(0, 0, 0, 16380, 0, 0, 1, 60), (0, 256, 1, 7, 1, 1, 3, 0), (0, 256 | 16, 0, 900, 2, 1, 3, 3), (1, 4, -1, 0, 0, 0, 0, 0),
            (2, 16, 1, 40, 0, 4, 1, 254)]
    recs = _records(rows)
    for ext in ("sam", "bam"):
        files = {}
        for name, mapq in [("parent", None), ("off", 0), ("on", 1), ("off_again", None)]:
            path = str(tmp_path / f"{name}.{ext}")
            assert _write(path, recs, cig, mapq, threads=1 + (name == "on")) == 0
            files[name] = open(path, "rb").read()
        # the switch off is the writer without the switch: the same bytes, MAPQ 255 in every record
        assert files["off"] == files["parent"] == files["off_again"]
        if ext == "sam":
            body = lambda b: [l.split("\t") for l in b.decode().splitlines() if not l.startswith("@")]
            assert [f[4] for f in body(files["parent"])] == ["255"] * 5
            on = body(files["on"])
            assert [int(f[4]) for f in on] == [r[7] for r in rows]
            assert [f[:4] + f[5:] for f in on] == [f[:4] + f[5:] for f in body(files["parent"])]       # nothing but column 5
        else:
            off, on = _bam_records(str(tmp_path / "parent.bam")), _bam_records(str(tmp_path / "on.bam"))
            assert [r["mapq"] for r in off] == [255] * 5
            assert [r["mapq"] for r in on] == [r[7] for r in rows]
            assert [{k: v for k, v in r.items() if k != "mapq"} for r in on] == [{k: v for k, v in r.items() if k != "mapq"} for r in off]
        # a quality that BAM cannot hold is refused when the switch is on, and ignored when it is off
        bad = _records([(0, 0, 0, 5, 0, 0, 1, 255)])
        assert _write(str(tmp_path / f"bad.{ext}"), bad, cig, 1) == -1                              # FLX_ERR_INVALID
        assert b"mapping quality" in capi.lib().flx_last_error()
        assert _write(str(tmp_path / f"ignored.{ext}"), bad, cig, 0) == 0


def test_writer_span_does_not_outlive_a_write_call(tmp_path):
    """two flx_sam_write calls whose CIGAR buffers have one address and one length and other operations: each record's BAM bin is
    its own CIGAR's (16380 + 4 stays in the 16-kb bin 4681 + 0; 16380 + 10 crosses into the next level up)"""
    cig = np.array([4 << 4 | 7], dtype=np.uint32)
    recs = _records([(0, 0, 0, 16380, 0, 0, 1, 0)])
    path = str(tmp_path / "one.bam")
    assert _write(path, recs, cig) == 0
    assert [r["bin"] for r in _bam_records(path)] == [_reg2bin(16380, 16384)] == [4681]

    def two_calls():                                              # the second call's words are written after the first call ran
        yield recs, cig
        cig[0] = 10 << 4 | 7                                      # the same buffer, other words
        yield recs, cig

    path = str(tmp_path / "two.bam")
    assert _write(path, None, None, calls=two_calls()) == 0
    assert [r["bin"] for r in _bam_records(path)] == [_reg2bin(16380, 16384), _reg2bin(16380, 16390)] == [4681, 585]


def test_cli_accepts_the_mapping_quality_flag(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    base = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"),
            "--output", str(tmp_path / "o.sam"), "-e", "2"]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0
    line = [l for l in h.stderr.decode().splitlines() if "--mapping-quality" in l]
    assert len(line) == 1 and "-Q," in line[0] and "not floxer's" in line[0]
    shorts = [l.split(",")[0].strip() for l in h.stderr.decode().splitlines() if l.startswith("  -")]
    assert len(shorts) == len(set(shorts)) == 29                  # floxer's 25, --devices, -D, -N, -Q: no spelling taken twice
    env = dict(os.environ, FLX_CLI_PARSE_ONLY="1")               # the options are parsed, then only the reader runs (no GPU)
    for extra in (["-Q"], ["--mapping-quality"], ["-D", "-N", "1", "-Q"], ["-Q", "--drop-duplicate-alignments", "--max-alignments=1"],
                  ["-Q", "--devices", "0", "-I", "-w", "-t", "2", "-M", "600", "-m", "60"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and r.stdout == b"" and b"CLI PARSER ERROR" not in r.stderr, (extra, r.stderr)
    for extra in (["-q"], ["--mapq"], ["-Q1"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr, extra
