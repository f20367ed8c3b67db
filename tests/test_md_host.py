"""The MD tag, host side: the plain-Python yardstick (md_from_cigar, reference_from_md) pinned to hand-written cases, the bound of the
device slab, the tagged SAM/BAM writer, the CLI flag and flx_tag_options. No GPU."""
import ctypes as C
import gzip
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"I": 1, "D": 2, "=": 7, "X": 8}
LETTERS = "NACGTN"          # ranks 1..4 -> ACGT, anything else -> N


# ------------------------------------------------------------------------------------------------ the yardstick
def cigar_words(text):
    """'10=1X' -> BAM words (len << 4 | op)"""
    return [int(n) << 4 | OPS[o] for n, o in re.findall(r"(\d+)([ID=X])", text)]


def md_from_cigar(reference_ranks, start, words):
    """samtools calmd's rule on an extended CIGAR: '=' columns count, every X column emits the count, the reference letter and resets,
    every D op emits the count, '^', its reference letters and resets, I does nothing, the end emits the count"""
    out, count, pos = [], 0, int(start)
    letter = lambda p: LETTERS[int(reference_ranks[p])] if int(reference_ranks[p]) < 6 else "N"
    for w in words:
        op, n = int(w) & 15, int(w) >> 4
        if op == 7:
            count += n
            pos += n
        elif op == 8:
            for _ in range(n):
                out.append(f"{count}{letter(pos)}")
                count = 0
                pos += 1
        elif op == 2:
            if n:
                out.append(f"{count}^" + "".join(letter(pos + i) for i in range(n)))
                count = 0
                pos += n
        elif op != 1:
            raise ValueError(f"op {op}")
    out.append(str(count))
    return "".join(out).encode()


def reference_from_md(read_letters, words, md):
    """the reference side of an alignment from the record alone: the read (forward strand letters of the record), its CIGAR and its MD"""
    toks = re.findall(r"\d+|\^[A-Z]+|[A-Z]", md.decode())
    ti, left = 0, 0            # current token, '=' columns left of a number token
    out, rp = [], 0
    for w in words:
        op, n = int(w) & 15, int(w) >> 4
        if op == 1:
            rp += n
            continue
        while n:
            if op == 7:
                if left == 0:
                    assert toks[ti].isdigit(), (toks[ti], "number expected")
                    left = int(toks[ti])
                    ti += 1
                    assert left > 0, "a '=' column under an empty match count"
                take = min(left, n)
                out.append(read_letters[rp: rp + take])
                rp += take
                left -= take
                n -= take
            else:
                if left == 0 and toks[ti].isdigit():
                    assert int(toks[ti]) == 0, "match columns left in front of a mismatch / deletion"
                    ti += 1
                assert left == 0
                if op == 8:
                    assert len(toks[ti]) == 1 and toks[ti].isalpha(), toks[ti]
                    out.append(toks[ti])
                    ti += 1
                    rp += 1
                    n -= 1
                else:
                    assert toks[ti] == "^" + toks[ti][1:] and len(toks[ti]) == n + 1, (toks[ti], n)
                    out.append(toks[ti][1:])
                    ti += 1
                    n = 0
    assert left == 0 and (ti == len(toks) or (ti == len(toks) - 1 and toks[ti] == "0")), (ti, toks[-3:])
    return "".join(out)


def ranks(s):
    return np.array([{"A": 1, "C": 2, "G": 3, "T": 4}.get(c, 5) for c in s], dtype=np.uint8)


PINNED = [
    # (reference letters, start, CIGAR, MD)
    ("GGGGGGGGGGATTTTTACCCCCCC", 0, "10=1X5=2D6=", b"10A5^AC6"),          # the SAM specification's own example string
    ("ACGT", 0, "2X2=", b"0A0C2"),                                         # X X -> A0C
    ("ACTGG", 0, "2D1X2=", b"0^AC0T2"),                                    # D then X -> ^AC0T
    ("ACGG", 0, "1D3I1D2=", b"0^A0^C2"),                                   # D I D -> ^A0^C
    ("A" * 2000, 0, "2000=", b"2000"),
    ("ACGTACGT", 2, "2=1I2=", b"4"),                                       # an I between two match runs merges them
    ("ACGTACGT", 1, "1X5=1X", b"0C5T0"),                                   # a mismatch in the first and in the last column
    ("ACNTA", 0, "2=1X2=", b"2N2"),
    ("AC", 0, "5I", b"0"),
]


def test_yardstick_on_pinned_cases():
    for ref, start, cig, md in PINNED:
        r = ranks(ref)
        assert md_from_cigar(r, start, cigar_words(cig)) == md, (ref, cig)
        span = sum(n for n, o in ((w >> 4, w & 15) for w in cigar_words(cig)) if o in (2, 7, 8))
        read, rp = [], start
        for w in cigar_words(cig):
            n, o = w >> 4, w & 15
            if o == 7:
                read.append(ref[rp: rp + n])
            elif o == 8:
                read.append("".join("C" if c != "C" else "G" for c in ref[rp: rp + n]))
            elif o == 1:
                read.append("T" * n)
            if o != 1:
                rp += n
        want = "".join(c if c in "ACGT" else "N" for c in ref[start: start + span])
        assert reference_from_md("".join(read), cigar_words(cig), md) == want, (ref, cig)
    assert md_from_cigar([0, 1, 5, 7, 2], 0, cigar_words("5X")) == b"0N0A0N0N0C0"     # ranks outside 1..4 are N


def slab_bound(nm):
    """flx_internal.hpp md_slab_bytes: at most nm events (an X column or a D op) with at most nm letters and one '^' per D op (<= 2 nm
    bytes), nm + 1 numbers of at most six digits (a run of '=' columns is at most the query rows, <= 102 400)"""
    return 8 * nm + 6


def test_slab_bound_holds():
    rng = np.random.default_rng(5)
    ref = rng.integers(1, 5, size=300_000, dtype=np.uint8)
    cases = [[n << 4 | 8] for n in (1, 2, 64, 65, 1000)]                                   # all X
    cases += [[1 << 4 | 8, 1 << 4 | 7] * n for n in (1, 40, 700)]                          # alternating X / =
    cases += [[1 << 4 | 2, 1 << 4 | 7] * n for n in (1, 40, 700)]                          # single-base deletions
    cases += [[1 << 4 | 2, 1 << 4 | 1] * 300, [102_400 << 4 | 7], [99_999 << 4 | 7, 1 << 4 | 8, 2_400 << 4 | 7], [5 << 4 | 1]]
    while len(cases) < 10_000:
        words, rows, last = [], 0, -1
        for _ in range(int(rng.integers(1, 60))):
            op = int(rng.choice([1, 2, 7, 8], p=[0.15, 0.15, 0.5, 0.2]))
            if op == last:
                continue
            n = int(rng.integers(1, 4)) if op != 7 else int(rng.choice([1, 9, 10, 99, 100, 999, 1000, 9999, 10_000]))
            if op != 2 and rows + n > 102_400:
                break
            rows += n if op != 2 else 0
            words.append(n << 4 | op)
            last = op
        if words:
            cases.append(words)
    for words in cases:
        nm = sum(w >> 4 for w in words if w & 15 != 7)
        assert len(md_from_cigar(ref, 17, words)) <= slab_bound(nm), words[:8]


# ------------------------------------------------------------------------------------------------ writer
def _records(rows):
    recs = (capi.Record * len(rows))()
    for i, r in enumerate(rows):
        recs[i] = capi.Record(*r)
    return recs


def _md_refs(refs):
    out = (capi.MdRef * max(1, len(refs)))()
    for i, (o, n) in enumerate(refs):
        out[i] = capi.MdRef(o, n, 0)
    return out


def _write(path, rows, cig, md_refs=None, md_bytes=b"", threads=1, plain=False):
    """records through flx_sam_write_tagged (plain: flx_sam_write); returns the status of the write call"""
    L = capi.lib()
    ref_ids = (C.c_char_p * 2)(b"chrA", b"chrB")
    ref_lens = np.array([100000, 5000], dtype=np.uint64)
    pool = np.array([1, 2, 3, 4, 1, 2, 3, 4, 4, 3, 2, 1], dtype=np.uint8)
    offs = np.array([0, 4, 8, 12], dtype=np.uint64)
    ids = (C.c_char_p * 3)(b"r0", b"r1", b"r2")
    quals = (C.c_char_p * 3)(b"IIII", b"JJJJ", b"")
    cig = np.asarray(cig, dtype=np.uint32)
    recs = _records(rows)
    w = C.c_void_p()
    capi.check(L.flx_sam_open(path.encode(), ref_ids, capi.ptr(ref_lens, capi.u64p), 2, C.byref(w)))
    capi.check(L.flx_sam_set_threads(w, threads))
    args = [w, ids, capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), quals, recs, len(rows), capi.ptr(cig, capi.u32p)]
    if plain:
        rc = L.flx_sam_write(*args)
    else:
        mdb = np.frombuffer(md_bytes + b"\0", dtype=np.uint8)
        rc = L.flx_sam_write_tagged(*args, _md_refs(md_refs) if md_refs is not None else None, capi.ptr(mdb, capi.u8p))
    L.flx_sam_close(w)
    return rc


def bgzf_members(data):
    """the BGZF members of a file, each inflated on its own with Python's gzip"""
    out, off = [], 0
    while off < len(data):
        assert data[off: off + 4] == b"\x1f\x8b\x08\x04", off
        xlen = struct.unpack_from("<H", data, off + 10)[0]
        assert data[off + 12: off + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", data, off + 16)[0] + 1
        assert 12 + xlen == 18
        out.append(gzip.decompress(data[off: off + bsize]))
        off += bsize
    return out


def bam_records(data):
    """[{ref, pos, flag, n_cigar, tags: [(tag, type, value)]}] of a BAM file's bytes"""
    data = b"".join(bgzf_members(data))
    off = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref = struct.unpack_from("<i", data, off)[0]
    off += 4
    for _ in range(n_ref):
        off += 4 + struct.unpack_from("<i", data, off)[0] + 4
    out = []
    while off < len(data):
        bs, ref_id, pos, l_name, mapq, bin_, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", data, off)
        at = off + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        end = off + 4 + bs
        tags = []
        while at < end:
            tag, ty = data[at: at + 2].decode(), chr(data[at + 2])
            at += 3
            if ty == "Z":
                z = data.index(b"\0", at)
                tags.append((tag, ty, data[at:z]))
                at = z + 1
            elif ty == "B":
                sub, cnt = chr(data[at]), struct.unpack_from("<i", data, at + 1)[0]
                assert sub == "I"
                tags.append((tag, ty, cnt))
                at += 5 + 4 * cnt
            else:
                size = {"C": 1, "S": 2, "I": 4}[ty]
                tags.append((tag, ty, int.from_bytes(data[at: at + size], "little")))
                at += size
        assert at == end
        out.append(dict(ref=ref_id, pos=pos, flag=flag, n_cigar=n_cig, tags=tags))
        off = end
    return out


CIG = [4 << 4 | 7, 2 << 4 | 7, 1 << 4 | 8, 1 << 4 | 7, 4 << 4 | 7]
#        read flag ref pos   nm coff clen reserved
ROWS = [(0, 0, 0, 16380, 0, 0, 1, 0), (0, 256, 1, 7, 1, 1, 3, 0), (0, 256 | 16, 0, 900, 1, 1, 3, 0), (1, 4, -1, 0, 0, 0, 0, 0), (2, 16, 1, 40, 0, 4, 1, 0)]
MD_BYTES = b"42A1"
MD_REFS = [(0, 1), (1, 3), (1, 3), (0, 0), (0, 0)]      # "4", "2A1", "2A1", none (unmapped), none (length 0)


def test_writer_md_tag_sam_and_bam(tmp_path):
    for ext in ("sam", "bam"):
        p = lambda n: str(tmp_path / f"{n}.{ext}")
        assert _write(p("plain"), ROWS, CIG, plain=True) == 0
        assert _write(p("null"), ROWS, CIG, None) == 0
        assert _write(p("md"), ROWS, CIG, MD_REFS, MD_BYTES) == 0
        assert open(p("null"), "rb").read() == open(p("plain"), "rb").read()            # md NULL is flx_sam_write
        if ext == "sam":
            body = [l.split("\t") for l in open(p("md")).read().splitlines() if not l.startswith("@")]
            plain = [l.split("\t") for l in open(p("plain")).read().splitlines() if not l.startswith("@")]
            assert [f[11:] for f in body] == [["NM:i:0", "MD:Z:4"], ["NM:i:1", "MD:Z:2A1"], ["NM:i:1", "MD:Z:2A1"], [], ["NM:i:0"]]
            assert [f[:12] for f in body] == [f[:12] for f in plain]
        else:
            got = bam_records(open(p("md"), "rb").read())
            assert [[(t, v) for t, _, v in r["tags"]] for r in got] == [[("NM", 0), ("MD", b"4")], [("NM", 1), ("MD", b"2A1")], [("NM", 1), ("MD", b"2A1")], [],
                                                                          [("NM", 0)]]
            off = bam_records(open(p("plain"), "rb").read())
            assert [{k: v for k, v in r.items() if k != "tags"} for r in got] == [{k: v for k, v in r.items() if k != "tags"} for r in off]
        # an unmapped record never gets the tag, even when it is given one
        refs = list(MD_REFS)
        refs[3] = (0, 1)
        assert _write(p("unmapped"), ROWS, CIG, refs, MD_BYTES) == 0
        assert open(p("unmapped"), "rb").read() == open(p("md"), "rb").read()
        # bytes that would break a SAM line or a BAM string are refused
        for bad in (b"4\tA1", b"4\nA1", b"4a11", b"4\0A1", b"4*A1"):
            assert _write(p("bad"), ROWS, CIG, MD_REFS, bad) == -1, bad                    # FLX_ERR_INVALID
            assert b"MD string" in capi.lib().flx_last_error()


def _many():
    """2000 records in groups that share one CIGAR array and one MD string (as the records of one traced path do), some on their own"""
    rng = np.random.default_rng(9)
    cig, md, rows, refs = [], b"", [], []
    while len(rows) < 2000:
        n_ops = int(rng.integers(20, 400))
        coff, moff = len(cig), len(md)
        cig += [int(rng.integers(1, 30)) << 4 | int(rng.choice([7, 8, 1, 2])) for _ in range(n_ops)]
        s = "".join(f"{int(rng.integers(0, 99))}{'ACGT'[int(rng.integers(0, 4))]}" for _ in range(n_ops // 2)).encode() + b"7"
        md += s
        for _ in range(int(rng.choice([1, 1, 8, 40]))):
            rows.append((int(rng.integers(0, 3)), 256, int(rng.integers(0, 2)), int(rng.integers(0, 4000)), 3, coff, n_ops, 0))
            refs.append((moff, len(s)))
    return rows, cig, refs, md


def test_writer_threads_and_bgzf_members(tmp_path):
    rows, cig, refs, md = _many()
    for ext in ("sam", "bam"):
        files = []
        for threads in (1, 4):
            path = str(tmp_path / f"t{threads}.{ext}")
            assert _write(path, rows, cig, refs, md, threads=threads) == 0
            files.append(open(path, "rb").read())
        assert files[0] == files[1]
    got = bam_records(files[0])                                  # every member inflates with Python's gzip (bgzf_members)
    assert [dict(r["tags"] and [(t, v) for t, _, v in r["tags"]])["MD"] for r in got] == [md[o: o + n] for o, n in refs]
    # the same under zlib's encoder, which the library chooses once per process
    path = str(tmp_path / "zlib.bam")
    env = dict(os.environ, FLX_BGZF_ZLIB="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + sys.path))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    zl = bam_records(open(path, "rb").read())
    assert zl == got
    # announced as repeats, the shared MD strings cost little: the file with MD stays well below the plain file plus every record's MD bytes
    plain = str(tmp_path / "plain.bam")
    assert _write(plain, rows, cig, plain=True) == 0
    assert len(files[0]) - os.path.getsize(plain) < sum(n for _, n in refs) // 2


def test_writer_long_cigar_record_keeps_its_md(tmp_path):
    n = 70_000
    cig = [1 << 4 | (7 if i % 2 == 0 else 8) for i in range(n)]
    md = b"".join(b"1A" for _ in range(n // 2)) + b"0"
    rows = [(0, 256, 0, 10, n // 2, 0, n, 0)]
    path = str(tmp_path / "long.bam")
    assert _write(path, rows, cig, [(0, len(md))], md) == 0
    (rec,) = bam_records(open(path, "rb").read())
    assert rec["n_cigar"] == 2 and [(t, ty) for t, ty, _ in rec["tags"]] == [("NM", "S"), ("MD", "Z"), ("CG", "B")]
    assert rec["tags"][1][2] == md and rec["tags"][2][2] == n
    path = str(tmp_path / "long.sam")
    assert _write(path, rows, cig, [(0, len(md))], md) == 0
    assert open(path).read().splitlines()[-1].split("\t")[11:] == [f"NM:i:{n // 2}", "MD:Z:" + md.decode()]


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_md_tag_flag(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    base = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"),
            "--output", str(tmp_path / "o.sam"), "-e", "2"]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0
    lines = h.stderr.decode().splitlines()
    line = [l for l in lines if "--md-tag" in l]
    assert len(line) == 1 and line[0].startswith("      --md-tag") and "not floxer's" in line[0]
    assert len([l for l in lines if l.startswith("  -")]) == 29                 # the long-only option takes no short spelling
    env = dict(os.environ, FLX_CLI_PARSE_ONLY="1")
    for extra in (["--md-tag"], ["--md-tag", "-D", "-N", "1", "-Q", "-I"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and r.stdout == b"" and b"CLI PARSER ERROR" not in r.stderr, (extra, r.stderr)
    for extra in (["--md-tag", "-w"], ["-w", "--md-tag"], ["--without-cigar", "--md-tag"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr and b"--md-tag" in r.stderr, extra
    r = subprocess.run(base + ["--md"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr


# ------------------------------------------------------------------------------------------------ flx_tag_options
def test_tag_options_validation_and_struct_sizes():
    assert C.sizeof(capi.TagOptions) == 32 and C.sizeof(capi.MdRef) == 16 and C.sizeof(capi.OutputOptions) == 32
    assert set(capi.EXPORTED) >= {"flx_align_reads_with_tags", "flx_align_reads_resident_with_tags", "flx_run_num_md_bytes", "flx_run_copy_md",
                                  "flx_align_batch_md", "flx_sam_write_tagged"}
    L = capi.lib()
    for name in capi.EXPORTED:
        assert hasattr(L, name), name
    p = F.params(error_probability=0.05)
    run = C.c_void_p()

    def call(tags, params=p):
        # (no context: a call that passes the option checks stops at the null context)
        rc = L.flx_align_reads_with_tags(None, C.byref(params), None, None, 0, None, C.byref(tags) if tags is not None else None, C.byref(run))
        return rc, L.flx_last_error().decode()

    null = call(None)
    assert null[0] == -1 and "null argument" in null[1]
    assert call(capi.TagOptions()) == null                              # zeroed is NULL
    assert call(F.tag_options(md=True)) == null                         # md = 1 is accepted
    t = capi.TagOptions()
    t.md = 2
    assert call(t)[0] == -1 and "md must be 0 or 1" in call(t)[1]
    for i in range(7):
        t = F.tag_options(md=True)
        t.reserved[i] = 1
        assert call(t)[0] == -1 and "reserved" in call(t)[1], i
    w = F.params(error_probability=0.05, without_cigar=True)
    rc, err = call(F.tag_options(md=True), w)
    assert rc == -1 and "without_cigar" in err
    assert call(capi.TagOptions(), w) == null                           # without md, without_cigar is as before
    assert L.flx_run_num_md_bytes(None) == 0


if __name__ == "__main__":                                              # the zlib half of test_writer_threads_and_bgzf_members
    rows_, cig_, refs_, md_ = _many()
    sys.exit(_write(sys.argv[1], rows_, cig_, refs_, md_, threads=2))
