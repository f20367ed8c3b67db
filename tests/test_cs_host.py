"""The cs tag, without a GPU: the rule (floxer_amd/csrc/flx_cs.hpp through flx_cs) against the plain Python rule of tests/cs_ref.py and,
through its inverse, against the inputs themselves, on crafted words (minimap2's own example shape among them) and on random valid
paths over ranks 0..5; every refusal; the capacities; the slab bound; the writer for SAM and BAM; the CLI flags; the struct layouts
and symbols; and tests/cs_check.cpp: the header under ASan + UBSan against a column-by-column definition."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import cs_ref as R
from test_md_host import bgzf_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, CAPACITY = -1, -3


def ranks(s):
    return np.array([{"A": 1, "C": 2, "G": 3, "T": 4, "$": 0}.get(c, 5) for c in s.upper()], dtype=np.uint8)


def both_forms(ref, begin, query, cigar, q_off=0):
    """flx_cs on one job, short and long, each checked against cs_ref and through the inverse against the inputs"""
    words = R.cigar_words(cigar)
    out = []
    for long in (False, True):
        (got,) = F.cs_string(ref, query, words, [(0, len(words), 0, len(ref), begin, q_off, len(query) - q_off)], long=long)
        assert got == R.cs_from_cigar(ref, begin, query[q_off:], words, long), (cigar, long)
        out.append(got)
    return out


def bam_records(data):
    """[{ref, pos, flag, n_cigar, tags: [(tag, type, value)]}] of a BAM file's bytes (tag types Z, C, S, I and the signed i)"""
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
            else:
                size = {"C": 1, "S": 2, "I": 4, "i": 4}[ty]
                tags.append((tag, ty, int.from_bytes(data[at: at + size], "little", signed=ty == "i")))
                at += size
        assert at == end
        out.append(dict(ref=ref_id, pos=pos, flag=flag, n_cigar=n_cig, tags=tags))
        off = end
    return out


# ------------------------------------------------------------------------------------------------ the rule
def test_rule_on_crafted_words():
    # the shape of the minimap2 manual's example, :6-ata:10+gtc:4*at:3
    ref = ranks("CGATCG" + "ATA" + "AAATAGAGTA" + "GAAT" + "A" + "TTG")
    qry = ranks("CGATCG" + "AAATAGAGTA" + "GTC" + "GAAT" + "T" + "TTG")
    short, long = both_forms(ref, 0, qry, "6=3D10=3I4=1X3=")
    assert short == b":6-ata:10+gtc:4*at:3"
    assert long == b"=CGATCG-ata=AAATAGAGTA+gtc=GAAT*at=TTG"
    R.check_inverse(short, ref, 0, qry, R.cigar_words("6=3D10=3I4=1X3="), False)
    R.check_inverse(long, ref, 0, qry, R.cigar_words("6=3D10=3I4=1X3="), True, true_path=True)
    assert R.sequences_from_cs(long) == (R.letters(ref), R.letters(qry))
    # begin and the query offset: the walk starts at the window's column `begin` and at the job's first query row
    assert both_forms(ranks("TT" + "ACGT"), 2, ranks("GGG" + "ACCT"), "2=1X1=", q_off=3) == [b":2*gc:1", b"=AC*gc=T"]
    # ranks 0 and 5 and bytes beyond them are n / N; nothing is compared again: an X over equal ranks is emitted as it stands
    ref = np.array([0, 5, 1, 200, 2, 2, 3], dtype=np.uint8)
    qry = np.array([0, 5, 1, 9, 2, 0, 3], dtype=np.uint8)
    assert both_forms(ref, 0, qry, "2=2X1D1I1X1=") == [b":2*aa*nn-c+c*cn:1", b"=NN*aa*nn-c+c*cn=G"]
    # every word emits on its own: neighbouring words of one op do not merge (MD would merge the counts)
    assert both_forms(ranks("ACGTAC"), 0, ranks("ACGTTT"), "2=2=1X1X") == [b":2:2*at*ct", b"=AC=GT*at*ct"]
    assert both_forms(ranks("ACGT"), 0, ranks("TTACGT"), "1I1I4=") == [b"+t+t:4", b"+t+t=ACGT"]
    # a gap as the first and as the last word; a path of gaps only
    assert both_forms(ranks("ACGT"), 1, ranks("TCG"), "1I2=1D") == [b"+t:2-t", b"+t=CG-t"]
    assert both_forms(ranks("ACGT"), 0, ranks("GG"), "4D2I") == [b"-acgt+gg", b"-acgt+gg"]
    # the digits of a count
    rng = np.random.default_rng(3)
    for n in (1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 102400):
        ref = rng.integers(1, 5, size=n + 1, dtype=np.uint8)
        qry = np.concatenate([ref[:n], [ref[n] % 4 + 1]]).astype(np.uint8)
        short, long = both_forms(ref, 0, qry, f"{n}=1X")
        assert short == f":{n}*{R.letter(ref[n]).lower()}{R.letter(qry[n]).lower()}".encode()
        assert len(long) == n + 4 and R.sequences_from_cs(long) == (R.letters(ref), R.letters(qry))
    # the empty path
    assert F.cs_string(ranks("ACGT"), ranks("AC"), [], [(0, 0, 0, 4, 0, 0, 2)]) == [b""]


def random_paths(n_paths, seed, max_words=40):
    """[(ref window, begin, query, words)]: valid paths over ranks 0..5 in which no two neighbouring words share an op (what K5,
    cigar_realign and cigar_left_align write), '=' columns pairing equal letters, X columns whatever the draw gives"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_paths):
        words, last = [], -1
        for _ in range(int(rng.integers(1, max_words))):
            op = int(rng.choice([7, 8, 1, 2], p=[0.4, 0.2, 0.2, 0.2]))
            if op == last:
                continue
            n = int(rng.choice([1, 2, 3, 9, 10, 63, 64, 65, 100, 129]))
            words.append(n << 4 | op)
            last = op
        begin = int(rng.integers(0, 7))
        cols = sum(w >> 4 for w in words if w & 15 != 1)
        rows = sum(w >> 4 for w in words if w & 15 != 2)
        ref = rng.integers(0, 6, size=begin + cols + int(rng.integers(0, 5)), dtype=np.uint8)
        qry = rng.integers(0, 6, size=rows + int(rng.integers(0, 5)), dtype=np.uint8)
        r, q = begin, 0
        for w in words:
            op, n = w & 15, w >> 4
            if op == 7:
                qry[q: q + n] = ref[r: r + n]
            r += n if op != 1 else 0
            q += n if op != 2 else 0
        out.append((ref, begin, qry, words))
    return out


def pack_jobs(paths):
    """the paths as one call: pools with a few letters between the jobs"""
    ref_pool, q_pool, words, jobs = [], [], [], []
    ro = qo = 0
    for ref, begin, qry, w in paths:
        jobs.append((len(words), len(w), ro + 2, len(ref), begin, qo + 3, len(qry)))
        ref_pool += [4, 4] + list(ref)
        q_pool += [3, 3, 3] + list(qry)
        words += w
        ro += 2 + len(ref)
        qo += 3 + len(qry)
    return np.array(ref_pool, np.uint8), np.array(q_pool, np.uint8), words, jobs


def test_rule_on_random_paths_against_the_reference_and_its_inverse():
    paths = random_paths(400, seed=11)
    ref_pool, q_pool, words, jobs = pack_jobs(paths)
    for long in (False, True):
        got = F.cs_string(ref_pool, q_pool, words, jobs, long=long)
        assert len(got) == len(paths)
        for (ref, begin, qry, w), g in zip(paths, got):
            assert g == R.cs_from_cigar(ref, begin, qry, w, long)
            R.check_inverse(g, ref, begin, qry, w, long, true_path=True)
            nm = sum(x >> 4 for x in w if x & 15 != 7)
            rows = sum(x >> 4 for x in w if x & 15 != 2)
            assert len(g) <= R.slab_bound(nm, rows, long)
    assert any(w[0] & 15 == 1 for _, _, _, w in paths) and any(len(w) > 30 for _, _, _, w in paths)


def test_slab_bound_is_reached_where_it_can_be():
    """flx_internal.hpp cs_slab_bytes. Short: 10 nm + 7, reached by one '=' word of 100 000 columns and more (a query has at most
    102 400 rows, so at nm > 0 a second six-digit count does not fit and the bound is not tight). Long: rows + 3 nm + 1, reached by
    = X = X ... = with single X columns."""
    ref = np.full(102400, 2, np.uint8)
    (s,) = F.cs_string(ref, ref, [102400 << 4 | 7], [(0, 1, 0, 102400, 0, 0, 102400)])
    assert len(s) == R.slab_bound(0, 102400, False) == 7
    words = R.cigar_words("3=1X" * 50 + "2=")
    n = sum(w >> 4 for w in words)
    ref, qry = np.full(n, 1, np.uint8), np.full(n, 4, np.uint8)
    (s,) = F.cs_string(ref, qry, words, [(0, len(words), 0, n, 0, 0, n)], long=True)
    assert len(s) == R.slab_bound(50, n, True) == n + 151
    # gap-only and X-only paths stay below it
    for cig in ("50X", "1I1D" * 40, "1D1X" * 40, "64I", "1X"):
        words = R.cigar_words(cig)
        nm = sum(w >> 4 for w in words)
        rows = sum(w >> 4 for w in words if w & 15 != 2)
        ref, qry = np.full(200, 3, np.uint8), np.full(200, 2, np.uint8)
        for long in (False, True):
            (s,) = F.cs_string(ref, qry, words, [(0, len(words), 0, 200, 0, 0, 200)], long=long)
            assert len(s) <= R.slab_bound(nm, rows, long), cig


# ------------------------------------------------------------------------------------------------ refusals and capacities
def _raw_cs(jobs, words, ref, qry, options, cap=None, fn=None, head=()):
    L = capi.lib()
    fn = fn or L.flx_cs
    arr = (capi.CsJob * max(1, len(jobs)))()
    for i, j in enumerate(jobs):
        arr[i] = capi.CsJob(*j)
    w = np.asarray(words, dtype=np.uint32)
    refs = (capi.MdRef * max(1, len(jobs)))()
    out = np.zeros(1 << 16, dtype=np.uint8)
    n = C.c_uint64(len(out) if cap is None else cap)
    rc = fn(*head, capi.ptr(ref, capi.u8p), len(ref), capi.ptr(qry, capi.u8p), len(qry), capi.ptr(w, capi.u32p), len(w), arr, len(jobs),
            C.byref(options) if options is not None else None, capi.ptr(out, capi.u8p), C.byref(n), refs)
    return rc, n.value, L.flx_last_error().decode(), [out[r.offset: r.offset + r.length].tobytes() for r in refs[: len(jobs)]]


def test_every_refusal_of_the_rule_alone():
    ref, qry = ranks("ACGTACGTAC"), ranks("ACGTTCGT")
    words = R.cigar_words("4=1X3=")
    #      coff clen res roff rlen begin qoff qlen res2
    good = (0, 3, 0, 0, 10, 0, 0, 8, 0)
    rc, n, _, got = _raw_cs([good], words, ref, qry, F.cs_options())
    assert rc == 0 and got == [b":4*at:3"] and n == 7
    # the form: 3 and beyond, and here also 0 and NULL (the call is the request)
    for form in (3, 4, 0xFFFFFFFF):
        o = capi.CsOptions()
        o.form = form
        rc, _, err, _ = _raw_cs([good], words, ref, qry, o)
        assert rc == INVALID and "form" in err
    assert _raw_cs([good], words, ref, qry, capi.CsOptions())[0] == INVALID and _raw_cs([good], words, ref, qry, None)[0] == INVALID
    # each reserved word
    for i in range(7):
        for long in (False, True):
            o = F.cs_options(long=long)
            o.reserved[i] = 1
            rc, _, err, _ = _raw_cs([good], words, ref, qry, o)
            assert rc == INVALID and "reserved" in err, i
    bad_jobs = {
        "words outside the pool": (1, 3, 0, 0, 10, 0, 0, 8, 0),
        "word offset outside the pool": (4, 0, 0, 0, 10, 0, 0, 8, 0),
        "window outside the pool": (0, 3, 0, 1, 10, 0, 0, 8, 0),
        "window offset outside the pool": (0, 3, 0, 11, 0, 0, 0, 8, 0),
        "query outside the pool": (0, 3, 0, 0, 10, 0, 1, 8, 0),
        "query offset outside the pool": (0, 3, 0, 0, 10, 0, 9, 0, 0),
        "reserved": (0, 3, 1, 0, 10, 0, 0, 8, 0),
        "reserved2": (0, 3, 0, 0, 10, 0, 0, 8, 1),
        "columns beyond the window": (0, 3, 0, 0, 10, 3, 0, 8, 0),
        "columns beyond a short window": (0, 3, 0, 0, 7, 0, 0, 8, 0),
        "rows beyond the query": (0, 3, 0, 0, 10, 0, 0, 7, 0),
        "rows beyond the query's offset": (0, 3, 0, 0, 10, 0, 1, 7, 0),
    }
    for what, job in bad_jobs.items():
        rc, n, err, _ = _raw_cs([good, job], words, ref, qry, F.cs_options())
        assert rc == INVALID and n == 0, what
    assert "outside its pools" in _raw_cs([bad_jobs["window outside the pool"]], words, ref, qry, F.cs_options())[2]
    assert "do not fit" in _raw_cs([bad_jobs["rows beyond the query"]], words, ref, qry, F.cs_options())[2]
    # a foreign op (M, N, S, H, P and the unassigned codes) and a zero-length word
    for op in (0, 3, 4, 5, 6, 9, 15):
        rc, _, err, _ = _raw_cs([good], [4 << 4 | 7, 1 << 4 | op, 3 << 4 | 7], ref, qry, F.cs_options())
        assert rc == INVALID and "op other than" in err, op
    for op in (7, 8, 1, 2):
        rc, _, err, _ = _raw_cs([good], [4 << 4 | 7, 0 << 4 | op, 4 << 4 | 7], ref, qry, F.cs_options())
        assert rc == INVALID and "length 0" in err, op
    # null arguments
    L = capi.lib()
    n = C.c_uint64(0)
    assert L.flx_cs(None, 0, None, 0, None, 0, None, 0, C.byref(F.cs_options()), None, None, None) == INVALID
    assert L.flx_cs(None, 0, None, 0, None, 0, None, 0, C.byref(F.cs_options()), None, C.byref(n), None) == 0 and n.value == 0
    # flx_cs_batch judges the same things before it looks at the context
    o = capi.CsOptions()
    o.form = 3
    assert _raw_cs([good], words, ref, qry, o, fn=L.flx_cs_batch, head=(None,))[0] == INVALID
    assert "form" in L.flx_last_error().decode()
    assert _raw_cs([good], words, ref, qry, F.cs_options(), fn=L.flx_cs_batch, head=(None,))[0] == INVALID
    assert "null argument" in L.flx_last_error().decode()


def test_capacity_equal_to_the_need_passes_and_one_byte_less_does_not():
    paths = random_paths(5, seed=4, max_words=12)
    ref_pool, q_pool, words, jobs = pack_jobs(paths)
    jobs = [(co, cl, 0, ro, rl, b, qo, ql, 0) for co, cl, ro, rl, b, qo, ql in jobs]
    for long in (False, True):
        want = [R.cs_from_cigar(ref, begin, qry, w, long) for ref, begin, qry, w in paths]
        need = sum(len(s) for s in want)
        rc, n, _, got = _raw_cs(jobs, words, ref_pool, q_pool, F.cs_options(long=long), cap=need)
        assert rc == 0 and n == need and got == want
        rc, n, err, _ = _raw_cs(jobs, words, ref_pool, q_pool, F.cs_options(long=long), cap=need - 1)
        assert rc == CAPACITY and n == need and "too small" in err
        rc, n, _, _ = _raw_cs(jobs, words, ref_pool, q_pool, F.cs_options(long=long), cap=0)
        assert rc == CAPACITY and n == need


def test_options_struct_symbols_and_run_calls_refuse_before_any_work():
    assert C.sizeof(capi.CsOptions) == 32 and C.sizeof(capi.CsJob) == 48 and capi.CsJob is capi.LeftAlignJob
    o = F.cs_options()
    assert (o.form, list(o.reserved)) == (1, [0] * 7) and F.cs_options(long=True).form == 2
    new = {"flx_align_reads_cs", "flx_align_reads_resident_cs", "flx_run_num_cs_bytes", "flx_run_copy_cs", "flx_align_batch_cs", "flx_cs",
           "flx_cs_batch", "flx_sam_write_cs"}
    assert new <= set(capi.EXPORTED)
    header = open(os.path.join(ROOT, "include", "floxer_amd.h")).read()
    assert set(re.findall(r"\b(flx_[a-z0-9_]+)\s*\(", header)) == set(capi.EXPORTED)
    L = capi.lib()
    for name in new:
        assert hasattr(L, name), name
    p = F.params(error_probability=0.05)
    w = F.params(error_probability=0.05, without_cigar=True)
    run = C.c_void_p()

    def calls(cs, params):
        # (no context, no reads: a call that passes the option checks stops at the null argument)
        c = C.byref(cs) if cs is not None else None
        host = L.flx_align_reads_resident_cs(None, C.byref(params), None, None, None, None, None, c, C.byref(run))
        err = L.flx_last_error().decode()
        return host, err

    null = calls(None, p)
    assert null[0] == INVALID and "null argument" in null[1]
    assert calls(capi.CsOptions(), p) == null and calls(F.cs_options(), p) == null and calls(F.cs_options(long=True), p) == null
    assert calls(None, w) == null and calls(capi.CsOptions(), w) == null                 # without cs, without_cigar is as before
    for long in (False, True):
        rc, err = calls(F.cs_options(long=long), w)
        assert rc == INVALID and "without_cigar" in err
    bad = capi.CsOptions()
    bad.form = 3
    assert calls(bad, p)[0] == INVALID and "form" in calls(bad, p)[1]
    for i in range(7):
        bad = F.cs_options()
        bad.reserved[i] = 7
        assert calls(bad, p)[0] == INVALID and "reserved" in calls(bad, p)[1], i
    # the host-pool entry point judges the same way, before it uploads anything
    bad = capi.CsOptions()
    bad.form = 9
    assert L.flx_align_reads_cs(None, C.byref(p), None, None, 0, None, None, None, None, C.byref(bad), C.byref(run)) == INVALID
    assert "form" in L.flx_last_error().decode()
    assert L.flx_align_reads_cs(None, C.byref(w), None, None, 0, None, None, None, None, C.byref(F.cs_options()), C.byref(run)) == INVALID
    assert "without_cigar" in L.flx_last_error().decode()
    # seam 2: the options first, then the context
    n = C.c_uint64(0)
    tail = (None, None, None, None, None, None)
    assert L.flx_align_batch_cs(None, None, 0, None, 0, None, 0, None, None, None, *tail, C.byref(bad), None, None, C.byref(n)) == INVALID
    assert "form" in L.flx_last_error().decode()
    refs = (capi.MdRef * 1)()
    assert L.flx_align_batch_cs(None, None, 0, None, 0, None, 0, None, None, None, *tail, C.byref(F.cs_options()), refs, None, C.byref(n)) == INVALID
    assert "null argument" in L.flx_last_error().decode()
    assert L.flx_run_num_cs_bytes(None) == 0 and L.flx_run_copy_cs(None, None, None) == INVALID


def test_rule_header_against_a_column_by_column_definition_under_sanitizers(tmp_path):
    """tests/cs_check.cpp: flx_cs.hpp on random paths, built with ASan + UBSan and run as a child process"""
    exe = str(tmp_path / "cs_check")
    src = os.path.join(ROOT, "tests", "cs_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------ writer
def _records(rows):
    recs = (capi.Record * len(rows))()
    for i, r in enumerate(rows):
        recs[i] = capi.Record(*r)
    return recs


def _refs(refs):
    out = (capi.MdRef * max(1, len(refs)))()
    for i, (o, n) in enumerate(refs):
        out[i] = capi.MdRef(o, n, 0)
    return out


def _write(path, rows, cig, cs_refs=None, cs_bytes=b"", md_refs=None, md_bytes=b"", scores=None, threads=1, scored=False, sa=False, n_reads=3):
    """records through flx_sam_write_cs (scored: flx_sam_write_scored); returns the status of the write call"""
    L = capi.lib()
    ref_ids = (C.c_char_p * 2)(b"chrA", b"chrB")
    ref_lens = np.array([100000, 5000], dtype=np.uint64)
    pool = np.array([1, 2, 3, 4] * n_reads, dtype=np.uint8)
    offs = np.arange(0, 4 * n_reads + 1, 4).astype(np.uint64)
    ids = (C.c_char_p * n_reads)(*[f"r{i}".encode() for i in range(n_reads)])
    quals = (C.c_char_p * n_reads)(*[b"IIII"] * n_reads)
    cig = np.asarray(cig, dtype=np.uint32)
    recs = _records(rows)
    w = C.c_void_p()
    capi.check(L.flx_sam_open(path.encode(), ref_ids, capi.ptr(ref_lens, capi.u64p), 2, C.byref(w)))
    capi.check(L.flx_sam_set_threads(w, threads))
    capi.check(L.flx_sam_set_sa(w, int(sa)))
    mdb = np.frombuffer(md_bytes + b"\0", dtype=np.uint8)
    sc = np.asarray(scores if scores is not None else [0], dtype=np.int32)
    args = [w, ids, capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), quals, recs, len(rows), capi.ptr(cig, capi.u32p),
            _refs(md_refs) if md_refs is not None else None, capi.ptr(mdb, capi.u8p),
            sc.ctypes.data_as(C.POINTER(C.c_int32)) if scores is not None else None]
    if scored:
        rc = L.flx_sam_write_scored(*args)
    else:
        csb = np.frombuffer(cs_bytes + b"\0", dtype=np.uint8)
        rc = L.flx_sam_write_cs(*args, _refs(cs_refs) if cs_refs is not None else None, capi.ptr(csb, capi.u8p))
    L.flx_sam_close(w)
    return rc


#          S      =      =      X      =      S      =
CIG = [1 << 4 | 4, 3 << 4 | 7, 2 << 4 | 7, 1 << 4 | 8, 1 << 4 | 7, 2 << 4 | 4, 2 << 4 | 7]
#        read flag ref pos   nm coff clen reserved
ROWS = [(0, 0, 0, 16380, 0, 0, 2, 0), (0, 2048, 1, 7, 1, 2, 3, 0), (0, 2048 | 16, 0, 900, 1, 2, 3, 0), (1, 4, -1, 0, 0, 0, 0, 0), (2, 16, 1, 40, 0, 5, 2, 0)]
CS_BYTES = b":3=AC*ga=T"
CS_REFS = [(0, 2), (2, 8), (2, 8), (0, 0), (0, 0)]      # ":3", "=AC*ga=T" twice, none (unmapped), none (length 0)
MD_BYTES = b"32A1"
MD_REFS = [(0, 1), (1, 3), (1, 3), (0, 0), (0, 1)]
SCORES = [6, -1, -1, 0, 4]


def test_writer_cs_tag_sam_and_bam(tmp_path):
    for ext in ("sam", "bam"):
        p = lambda n: str(tmp_path / f"{n}.{ext}")
        full = dict(md_refs=MD_REFS, md_bytes=MD_BYTES, scores=SCORES, sa=True)
        assert _write(p("scored"), ROWS, CIG, scored=True, **full) == 0
        assert _write(p("null"), ROWS, CIG, None, **full) == 0
        assert open(p("null"), "rb").read() == open(p("scored"), "rb").read()          # cs NULL is flx_sam_write_scored
        assert _write(p("bare_scored"), ROWS, CIG, scored=True) == 0 and _write(p("bare_null"), ROWS, CIG, None) == 0
        assert open(p("bare_null"), "rb").read() == open(p("bare_scored"), "rb").read()
        assert _write(p("cs"), ROWS, CIG, CS_REFS, CS_BYTES, **full) == 0
        assert _write(p("bare_cs"), ROWS, CIG, CS_REFS, CS_BYTES) == 0
        if ext == "sam":
            body = [l.split("\t") for l in open(p("cs")).read().splitlines() if not l.startswith("@")]
            off = [l.split("\t") for l in open(p("scored")).read().splitlines() if not l.startswith("@")]
            tags = [[t[:5] for t in f[11:]] for f in body]
            # behind NM / MD / AS and in front of SA; mapped records with a non-zero length only
            assert tags == [["NM:i:", "MD:Z:", "AS:i:", "cs:Z:", "SA:Z:"]] * 3 + [[], ["NM:i:", "MD:Z:", "AS:i:"]]
            assert [f[14] for f in body[:3]] == ["cs:Z::3", "cs:Z:=AC*ga=T", "cs:Z:=AC*ga=T"]
            assert [[t for t in f if not t.startswith("cs:Z:")] for f in body] == off            # every other byte as without it
            bare = [l.split("\t")[11:] for l in open(p("bare_cs")).read().splitlines() if not l.startswith("@")]
            assert bare == [["NM:i:0", "cs:Z::3"], ["NM:i:1", "cs:Z:=AC*ga=T"], ["NM:i:1", "cs:Z:=AC*ga=T"], [], ["NM:i:0"]]
        else:
            got = bam_records(open(p("cs"), "rb").read())
            assert [[t for t, _, _ in r["tags"]] for r in got] == [["NM", "MD", "AS", "cs", "SA"]] * 3 + [[], ["NM", "MD", "AS"]]
            assert [dict((t, v) for t, _, v in r["tags"]).get("cs") for r in got] == [b":3", b"=AC*ga=T", b"=AC*ga=T", None, None]
            off = bam_records(open(p("scored"), "rb").read())
            assert [dict(r, tags=[t for t in r["tags"] if t[0] != "cs"]) for r in got] == off
            bare = bam_records(open(p("bare_cs"), "rb").read())
            assert [[(t, ty) for t, ty, _ in r["tags"]] for r in bare] == [[("NM", "C"), ("cs", "Z")]] * 3 + [[], [("NM", "C")]]
        # an unmapped record never gets the tag, even when it is given one
        refs = list(CS_REFS)
        refs[3] = (0, 2)
        assert _write(p("unmapped"), ROWS, CIG, refs, CS_BYTES, **full) == 0
        assert open(p("unmapped"), "rb").read() == open(p("cs"), "rb").read()
        # every byte of the alphabet passes; bytes outside [0-9:*+=acgtnACGTN-] are refused
        ok = b"0123456789:*+=-acgtnACGTN"
        assert _write(p("alphabet"), ROWS[:1], CIG, [(0, len(ok))], ok) == 0
        for bad in (b":3\t", b":3\n", b":3\0=", b":3~a", b":3^a", b"=AB", b"+x", b"=AC ", b"*Ga;", b":3,", b":3/", b":3<"):
            assert _write(p("bad"), ROWS[:1], CIG, [(0, len(bad))], bad) == INVALID, bad
            assert b"cs string" in capi.lib().flx_last_error()


def _many(n_records=1500):
    """records in groups that share one CIGAR array and one cs string (as the records of one traced path do), some on their own"""
    rng = np.random.default_rng(9)
    cig, cs, rows, refs = [], b"", [], []
    while len(rows) < n_records:
        n_ops = int(rng.integers(20, 300))
        coff, soff = len(cig), len(cs)
        cig += [int(rng.integers(1, 30)) << 4 | int(rng.choice([7, 8, 1, 2])) for _ in range(n_ops)]
        s = "".join(f"={''.join('ACGT'[int(x)] for x in rng.integers(0, 4, size=int(rng.integers(1, 40))))}*{'acgt'[int(rng.integers(0, 4))]}{'acgt'[int(rng.integers(0, 4))]}"
                    for _ in range(n_ops // 2)).encode()
        cs += s
        for _ in range(int(rng.choice([1, 1, 8, 40]))):
            rows.append((int(rng.integers(0, 3)), 256, int(rng.integers(0, 2)), int(rng.integers(0, 4000)), 3, coff, n_ops, 0))
            refs.append((soff, len(s)))
    return rows, cig, refs, cs


def test_writer_output_does_not_depend_on_its_thread_count(tmp_path):
    rows, cig, refs, cs = _many()
    for ext in ("sam", "bam"):
        files = []
        for threads in (1, 4):
            path = str(tmp_path / f"t{threads}.{ext}")
            assert _write(path, rows, cig, refs, cs, threads=threads) == 0
            files.append(open(path, "rb").read())
        assert files[0] == files[1]
        if ext == "sam":
            body = [l.split("\t") for l in files[0].decode().splitlines() if not l.startswith("@")]
            assert [f[-1] for f in body] == ["cs:Z:" + cs[o: o + n].decode() for o, n in refs]
    got = bam_records(files[0])
    assert [dict((t, v) for t, _, v in r["tags"])["cs"] for r in got] == [cs[o: o + n] for o, n in refs]
    # announced as repeats, the shared strings cost little: the file with cs stays well below the plain file plus every record's cs bytes
    plain = str(tmp_path / "plain.bam")
    assert _write(plain, rows, cig, None) == 0
    assert len(files[0]) - os.path.getsize(plain) < sum(n for _, n in refs) // 4


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_cs_flags(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    base = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"),
            "--output", str(tmp_path / "o.sam"), "-e", "2"]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0
    lines = h.stderr.decode().splitlines()
    for flag in ("--cs-tag", "--cs-tag-long"):
        line = [l for l in lines if re.search(rf"^\s+{flag}(\s|$)", l)]
        assert len(line) == 1 and line[0].startswith("      " + flag) and "not floxer's" in line[0], flag      # long spellings only
    env = dict(os.environ, FLX_CLI_PARSE_ONLY="1")
    every = ["-D", "-N", "1", "-Q", "-I", "--md-tag", "--partial-alignments", "--partial-extend", "--sa-tag", "--split-tails", "--left-align-indels", "--realign-affine"]
    for extra in (["--cs-tag"], ["--cs-tag-long"], ["--cs-tag"] + every, ["--cs-tag-long"] + every):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and r.stdout == b"" and b"CLI PARSER ERROR" not in r.stderr, (extra, r.stderr)
    for extra in (["--cs-tag", "--cs-tag-long"], ["--cs-tag-long", "--cs-tag"], ["--cs-tag", "-w"], ["-w", "--cs-tag-long"],
                  ["--without-cigar", "--cs-tag"], ["--cs-tag-long", "--without-cigar"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr and b"--cs-tag" in r.stderr, extra
    for extra in (["--cs"], ["--cs-tag-short"], ["--cs-tag-longer"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr, extra
