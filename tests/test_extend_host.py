"""Extension of partial records and the SA tag, without a GPU: the rule as a numpy DP (the GPU tests compare the kernel with it; here
it is checked against a plain full-matrix DP), struct layouts, exported symbols, the option checks (judged before the context is
looked at), the writer's SA:Z strings on hand-made records (SAM text, BAM through zlib) and the CLI's flag combinations."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
from test_partial_host import READ_LEN, _bam, _write, w, EQ, X, INS, DEL, S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 40


# ------------------------------------------------------------------------------------------------ the rule
def rule(q, t, weight=4, x_drop=100, d_max=1024):
    """q: the query rows in walking order, t: the reference symbols in walking order (all rows / symbols the extension may take).
    D[i][j]: unit-cost edit distance between the first i rows and the first j symbols, D[0][0] = 0; m(i) = min_j D[i][j];
    R(d) = max{i : m(i) <= d}; score(d) = R(d) - weight * d. Scan d = 0, 1, ..: keep the running maximum G and the first d that
    reached it; stop at the first d with G - score(d) > x_drop, R(d) == len(q) or d == d_max. Returns (rows, cols, errors, reason):
    i* = R(d*), the smallest j with D[i*][j] == d*, d*. D is computed over the band |j - i| <= d_max only: D[i][j] >= |j - i|, so
    no value <= d_max lies outside it."""
    q, t = np.asarray(q, dtype=np.int64), np.asarray(t, dtype=np.int64)
    n_rows = len(q)
    t = t[: n_rows + d_max]
    n_cols = len(t)
    row = np.full(n_cols + 1, BIG, dtype=np.int64)
    hi = min(n_cols, d_max)
    row[: hi + 1] = np.arange(hi + 1)

    def next_row(prev, i1):
        lo, hi = max(0, i1 - d_max), min(n_cols, i1 + d_max)
        new = np.full(n_cols + 1, BIG, dtype=np.int64)
        if lo > hi:
            return new
        js = np.arange(lo, hi + 1)
        cand = prev[js] + 1
        d = js >= 1
        cand[d] = np.minimum(cand[d], prev[js[d] - 1] + (t[js[d] - 1] != q[i1 - 1]))
        new[lo: hi + 1] = np.minimum(np.minimum.accumulate(cand - js) + js, BIG)
        return new

    i, ahead = 0, None
    best = None                                               # (G, d*, i*, j*)
    d = 0
    while True:
        while i < n_rows:
            if ahead is None:
                ahead = next_row(row, i + 1)
            if ahead.min() > d:
                break
            row, ahead, i = ahead, None, i + 1
        score = i - weight * d
        if best is None or score > best[0]:
            at = np.flatnonzero(row == d)
            assert len(at), "m(R(d*)) == d* at every new maximum"
            best = (score, d, i, int(at[0]))
        if best[0] - score > x_drop:
            reason = 1
            break
        if i == n_rows:
            reason = 2
            break
        if d == d_max:
            reason = 3
            break
        d += 1
    return best[2], best[3], best[1], reason


def rule_full_matrix(q, t, weight, x_drop, d_max):
    """the same statement on the whole matrix, cell by cell"""
    n, m = len(q), len(t)
    D = np.zeros((n + 1, m + 1), dtype=np.int64)
    D[0] = np.arange(m + 1)
    D[:, 0] = np.arange(n + 1)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            D[i, j] = min(D[i - 1, j - 1] + (q[i - 1] != t[j - 1]), D[i - 1, j] + 1, D[i, j - 1] + 1)
    mins = D.min(axis=1)
    assert (np.diff(mins) >= 0).all() and (np.diff(mins) <= 1).all()      # m is non-decreasing and grows by at most 1 per row
    G = None
    for d in range(d_max + 1):
        R = int(np.flatnonzero(mins <= d)[-1])
        score = R - weight * d
        if G is None or score > G:
            G, d_star, i_star = score, d, R
        if G - score > x_drop or R == n or d == d_max:
            break
    return i_star, int(np.flatnonzero(D[i_star] == d_star)[0]), d_star


def test_the_numpy_rule_is_the_full_matrix_rule():
    rng = np.random.default_rng(3)
    for case in range(40):
        n = int(rng.integers(0, 60))
        t = rng.integers(1, 5, size=int(rng.integers(0, 80)))
        q = t[:n].copy() if case % 2 else rng.integers(1, 5, size=n)
        for p in rng.integers(0, max(1, len(q)), size=len(q) // 6):
            q[p] = 1 + q[p] % 4
        if case % 3 == 0 and len(q) > 10:
            q = np.delete(q, 5)
        for weight, x_drop, d_max in ((4, 100, 1024), (2, 6, 1024), (8, 3, 4), (1, 1, 1024), (4, 100, 0)):
            assert rule(q, t, weight, x_drop, d_max)[:3] == rule_full_matrix(q, t, weight, x_drop, d_max), (case, weight, x_drop, d_max)


# ------------------------------------------------------------------------------------------------ layouts, symbols, options
def test_struct_layouts_and_exported_symbols():
    assert C.sizeof(capi.ExtendOptions) == 32 and C.sizeof(capi.RunOptions) == 64
    assert C.sizeof(capi.ExtendJob) == 40 and C.sizeof(capi.ExtendResult) == 16
    assert [getattr(capi.ExtendOptions, f).offset for f in ("enable", "error_weight", "x_drop", "max_errors", "reserved")] == [0, 4, 8, 12, 16]
    assert [getattr(capi.RunOptions, f).offset for f in ("output", "tags", "partial", "extend", "reserved")] == [0, 8, 16, 24, 32]
    assert [getattr(capi.ExtendJob, f).offset for f in ("text_pos", "q_pos", "ref_limit", "row_limit", "direction", "error_weight", "x_drop", "max_errors")] == \
           [0, 8, 16, 20, 24, 28, 32, 36]
    assert set(capi.EXPORTED) >= {"flx_extend_batch", "flx_sam_set_sa"}
    for name in capi.EXPORTED:
        assert hasattr(capi.lib(), name), name
    o = F.extend_options()
    assert (o.enable, o.error_weight, o.x_drop, o.max_errors, list(o.reserved)) == (1, 0, 0, 0, [0] * 4)
    o = F.extend_options(error_weight=2, x_drop=30, max_errors=16, enable=False)
    assert (o.enable, o.error_weight, o.x_drop, o.max_errors) == (0, 2, 30, 16)
    with pytest.raises(F.FloxerError):
        F.extend_options(x_drop=-1)


def test_options_are_judged_before_the_context_is_looked_at():
    L = capi.lib()
    p = F.params(error_probability=0.05)
    run = C.c_void_p()
    pool = np.ones(8, dtype=np.uint8)
    offs = np.array([0, 8], dtype=np.uint64)

    def call(partial, extend, reserved=None):
        bundle = capi.RunOptions()
        if partial is not None:
            bundle.partial = C.pointer(partial)
        if extend is not None:
            bundle.extend = C.pointer(extend)
        if reserved is not None:
            bundle.reserved[reserved] = 1
        # (no context at all: the options are judged first)
        a = L.flx_align_reads_opt(None, C.byref(p), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), 1, C.byref(bundle), C.byref(run))
        ea = L.flx_last_error()
        b = L.flx_align_reads_resident_opt(None, C.byref(p), None, C.byref(bundle), C.byref(run))
        assert a == b == -1
        return ea + b"|" + L.flx_last_error()

    part = F.partial_options()
    for k in range(4):
        e = F.extend_options()
        e.reserved[k] = 1
        assert call(part, e).count(b"flx_extend_options: the reserved fields") == 2, k
    e = F.extend_options()
    e.enable = 2
    assert call(part, e).count(b"flx_extend_options: enable must be 0 or 1") == 2
    for k in range(4):
        assert call(part, F.extend_options(), reserved=k).count(b"reserved pointers") == 2, k
    # extend without partial: no struct, a zeroed one, one switched off
    for partial in (None, capi.PartialOptions(), F.partial_options(enable=False)):
        assert call(partial, F.extend_options()).count(b"needs flx_partial_options.enable") == 2
    assert call(part, F.extend_options(max_errors=4094)).count(b"max_errors") == 2          # does not fit the kernel's LDS
    assert call(part, F.extend_options(error_weight=65536)).count(b"error_weight") == 2
    assert call(part, F.extend_options(x_drop=(1 << 30) + 1)).count(b"x_drop") == 2
    # -w follows from partial
    p.without_cigar = 1
    assert call(part, F.extend_options()).count(b"without_cigar") == 2
    p.without_cigar = 0
    # valid, or off: the refusal is the null context's
    for partial, extend in ((part, F.extend_options(max_errors=4093, error_weight=65535, x_drop=1 << 30)), (None, F.extend_options(enable=False)),
                            (None, capi.ExtendOptions()), (part, None)):
        msg = call(partial, extend)
        assert b"flx_extend_options" not in msg and b"null" in msg
    # the kernel's hook judges its jobs before the context as well? No: it needs the context's text length. A null context is refused.
    job = (capi.ExtendJob * 1)(capi.ExtendJob(0, 0, 1, 1, 1, 0, 0, 0))
    res = (capi.ExtendResult * 1)()
    assert L.flx_extend_batch(None, None, 0, capi.ptr(pool, capi.u8p), 8, job, 1, res) == -1 and b"null" in L.flx_last_error()


# ------------------------------------------------------------------------------------------------ the writer's SA tag
def _sa_case():
    # r0 (40 bases): a primary on chrA + and two supplementaries (chrB -, chrA +); r1 unmapped; r2 (30 bases): a single primary with a
    # clip (no 2048 record: no SA)
    cig = np.array([w(5, S), w(30, EQ), w(1, X), w(1, EQ), w(3, S),
                    w(8, S), w(10, EQ), w(2, DEL), w(3, X), w(19, EQ),
                    w(20, EQ), w(2, INS), w(4, EQ), w(4, S),
                    w(30, S), w(4, EQ), w(1, X), w(1, INS), w(4, EQ)], dtype=np.uint32)
    #        read flag       ref pos    nm coff clen reserved (MAPQ)
    rows = [(0, 0,          0, 16350, 1, 0, 5, 60),
            (0, 2048 | 16,  1, 700,   5, 5, 5, 3),
            (0, 2048,       0, 99,    2, 14, 5, 0),
            (1, 4,         -1, 0,     0, 0, 0, 0),
            (2, 16,         0, 16370, 2, 10, 4, 17)]
    entry = [("chrA,16351,+,5S32M3S,{q},1;", 60), ("chrB,701,-,8S10M2D22M,{q},5;", 3), ("chrA,100,+,30S5M1I4M,{q},2;", 0)]
    return cig, rows, entry


def _sa_want(entry, from_records):
    e = [s.format(q=q if from_records else 255) for s, q in entry]
    return [e[1] + e[2], e[0] + e[2], e[0] + e[1], None, None]


def _write_sa(path, rows, cig, threads, sa, mapq):
    """_write of test_partial_host (the same reads, names and qualities) with the writer's two switches; sa None: never touched"""
    L = capi.lib()
    ref_ids = (C.c_char_p * 2)(b"chrA", b"chrB")
    ref_lens = np.array([100000, 50000], dtype=np.uint64)
    pool = np.random.default_rng(5).integers(1, 5, size=sum(READ_LEN), dtype=np.uint8)
    offs = np.cumsum([0] + READ_LEN).astype(np.uint64)
    ids = (C.c_char_p * 3)(b"r0", b"r1", b"r2")
    quals = (C.c_char_p * 3)(b"I" * 40, b"J" * 12, b"")
    recs = (capi.Record * len(rows))(*[capi.Record(*r) for r in rows])
    h = C.c_void_p()
    capi.check(L.flx_sam_open(path.encode(), ref_ids, capi.ptr(ref_lens, capi.u64p), 2, C.byref(h)))
    capi.check(L.flx_sam_set_threads(h, threads))
    if sa is not None:
        capi.check(L.flx_sam_set_sa(h, sa))
    capi.check(L.flx_sam_set_mapq(h, int(mapq)))
    rc = L.flx_sam_write(h, ids, capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), quals, recs, len(rows), capi.ptr(cig, capi.u32p))
    capi.check(L.flx_sam_close(h))
    assert rc == 0, L.flx_last_error()


def test_writer_sa_strings_in_sam_and_bam(tmp_path):
    cig, rows, entry = _sa_case()
    for from_records in (False, True):
        want = _sa_want(entry, from_records)
        files = {}
        for ext in ("sam", "bam"):
            for threads in (1, 4):
                path = str(tmp_path / f"sa{int(from_records)}_{threads}.{ext}")
                _write_sa(path, rows, cig, threads, 1, from_records)
                files[ext, threads] = open(path, "rb").read()
            assert files[ext, 1] == files[ext, 4]                        # the same bytes with 1 and 4 writer threads
        body = [l.split("\t") for l in files["sam", 1].decode().splitlines() if not l.startswith("@")]
        bam = _bam(str(tmp_path / f"sa{int(from_records)}_1.bam"))
        assert len(body) == len(bam) == len(rows)
        for f, b, r, sa in zip(body, bam, rows, want):
            assert int(f[4]) == (r[7] if from_records else 255)
            if r[1] & 4:
                assert len(f) == 11 and b["tags"] == b""
                continue
            assert f[11] == f"NM:i:{r[4]}" and b["tags"][:4] == b"NMC" + bytes([r[4]])
            if sa is None:                                              # no SA on a read without a 2048 record
                assert len(f) == 12 and len(b["tags"]) == 4
            else:                                                       # behind NM; the read's other records in written order
                assert f[12:] == ["SA:Z:" + sa] and b["tags"][4:] == b"SAZ" + sa.encode() + b"\0"
        # = / X runs are merged into M, both strands occur, the ops are S M I D only
        assert all(set(c for c in s.split(",")[3] if not c.isdigit()) <= set("SMID") for x in want if x for s in x.split(";") if s)
        assert any(",-," in x for x in want if x) and any(",+," in x for x in want if x)


def test_writer_sa_behind_md_and_off_is_byte_identical(tmp_path):
    cig, rows, entry = _sa_case()
    L = capi.lib()
    # off (never set, or set to 0): the bytes of a writer that knows nothing of the tag
    for ext in ("sam", "bam"):
        plain = str(tmp_path / f"plain.{ext}")
        _write(plain, rows, cig, 2)
        for k, sa in enumerate((None, 0)):
            path = str(tmp_path / f"off{k}.{ext}")
            _write_sa(path, rows, cig, 2, sa, False)
            assert open(path, "rb").read() == open(plain, "rb").read(), (ext, sa)
    # with MD: NM, MD, SA in this order
    md = [b"30A1", b"10^AC0A0C0G19", b"9", None, b"24"]
    ref_ids = (C.c_char_p * 2)(b"chrA", b"chrB")
    ref_lens = np.array([100000, 50000], dtype=np.uint64)
    pool = np.ones(82, dtype=np.uint8)
    offs = np.array([0, 40, 52, 82], dtype=np.uint64)
    ids = (C.c_char_p * 3)(b"r0", b"r1", b"r2")
    recs = (capi.Record * len(rows))(*[capi.Record(*r) for r in rows])
    refs = (capi.MdRef * len(rows))()
    blob = b""
    for i, m in enumerate(md):
        refs[i] = capi.MdRef(len(blob), len(m or b""), 0)
        blob += m or b""
    buf = np.frombuffer(blob, dtype=np.uint8).copy()
    want = _sa_want(entry, False)
    for ext in ("sam", "bam"):
        path = str(tmp_path / f"md.{ext}")
        h = C.c_void_p()
        capi.check(L.flx_sam_open(path.encode(), ref_ids, capi.ptr(ref_lens, capi.u64p), 2, C.byref(h)))
        capi.check(L.flx_sam_set_sa(h, 1))
        capi.check(L.flx_sam_write_tagged(h, ids, capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), None, recs, len(rows), capi.ptr(cig, capi.u32p),
                                          refs, capi.ptr(buf, capi.u8p)))
        capi.check(L.flx_sam_close(h))
        if ext == "sam":
            body = [l.split("\t") for l in open(path).read().splitlines() if not l.startswith("@")]
            for f, m, sa in zip(body, md, want):
                assert f[11:] == ([] if m is None else [f[11], "MD:Z:" + m.decode()] + (["SA:Z:" + sa] if sa else []))
        else:
            for b, m, sa in zip(_bam(path), md, want):
                assert b["tags"][4:] == (b"" if m is None else b"MDZ" + m + b"\0" + (b"SAZ" + sa.encode() + b"\0" if sa else b""))
    assert L.flx_sam_set_sa(None, 1) == -1


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_flags(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    base = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"),
            "--output", str(tmp_path / "o.sam"), "-e", "2"]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0
    for name in ("--partial-extend ", "--partial-extend-weight <value>", "--partial-extend-xdrop <value>", "--partial-extend-max-errors <value>", "--sa-tag"):
        line = [l for l in h.stderr.decode().splitlines() if l.strip().startswith(name)]
        assert len(line) == 1 and line[0].startswith("      --") and "not floxer's" in line[0], name        # long spellings only
    env = dict(os.environ, FLX_CLI_PARSE_ONLY="1")               # the options are parsed, then only the reader runs (no GPU)
    pa = "--partial-alignments"
    for extra in ([pa, "--partial-extend"], [pa, "--sa-tag"], [pa, "--partial-extend", "--sa-tag", "-Q", "--md-tag"],
                  [pa, "--partial-extend", "--partial-extend-weight", "2", "--partial-extend-xdrop=30", "--partial-extend-max-errors", "4093"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and b"CLI PARSER ERROR" not in r.stderr, (extra, r.stderr)
    for extra in (["--partial-extend"], ["--sa-tag"], [pa, "--partial-extend-weight", "2"], [pa, "--partial-extend-xdrop", "30"],
                  [pa, "--partial-extend-max-errors", "16"], [pa, "--partial-extend", "--partial-extend-max-errors", "4094"],
                  [pa, "--partial-extend", "--partial-extend-weight", "0"], [pa, "--partial-extend", "--partial-extend-xdrop", "x"],
                  [pa, "--partial-extend", "-w"], ["--partial-extend", "--sa-tag"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr, extra
