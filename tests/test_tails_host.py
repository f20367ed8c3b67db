"""Chimeric tails of reads mapped in full, without a GPU: the rule (floxer_amd/csrc/flx_tails.hpp through flx_cigar_tails) against a plain
Python restatement of it - a loop over the boundaries - on hand-made and random CIGARs, struct layouts, exported symbols, option
defaults, the option checks (judged before the context is looked at), the CLI's flag combinations, and tests/tails_check.cpp: the rule
header under ASan + UBSan against definitions that look at every pair of boundaries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INS, DEL, EQ, X, SOFT = 1, 2, 7, 8, 4
W, XDROP, MIN_ROWS = 4, 100, 100                                 # the defaults (include/floxer_amd.h)


def w(n, op):
    return (n << 4) | op


# ------------------------------------------------------------------------------------------------ the rule
def rule(words, weight=W, x_drop=XDROP, min_rows=MIN_ROWS):
    """Boundary t = 0..T lies behind word t. rows / cols / err: the query consumed, the reference consumed, the lengths of X, I and D;
    S = rows - weight * err. Right tail: G = max S, t_R the smallest t with S_t = G; it exists iff G - S_T > x_drop and
    rows_T - rows_tR >= min_rows. Left tail: g = min S, t_L the largest t with S_t = g; it exists iff -g > x_drop and
    rows_tL >= min_rows. Both and t_L >= t_R: neither. Returns the eight numbers (zeros: absent), None for an invalid CIGAR."""
    rows, cols, err, S = [0], [0], [0], [0]
    for word in words:
        op, n = int(word) & 15, int(word) >> 4
        if op not in (EQ, X, INS, DEL):
            return None
        rows.append(rows[-1] + (n if op in (EQ, X, INS) else 0))
        cols.append(cols[-1] + (n if op in (EQ, X, DEL) else 0))
        err.append(err[-1] + (n if op in (X, INS, DEL) else 0))
        S.append(rows[-1] - weight * err[-1])
    if sum(int(word) >> 4 for word in words) >= 1 << 32:
        return None
    T = len(words)
    G, g = max(S), min(S)
    t_r = min(t for t in range(T + 1) if S[t] == G)
    t_l = max(t for t in range(T + 1) if S[t] == g)
    right = G - S[T] > x_drop and rows[T] - rows[t_r] >= min_rows
    left = -g > x_drop and rows[t_l] >= min_rows
    if left and right and t_l >= t_r:
        left = right = False
    out = [0] * 8
    if left:
        out[:4] = [rows[t_l], cols[t_l], err[t_l], t_l]
    if right:
        out[4:] = [rows[T] - rows[t_r], cols[T] - cols[t_r], err[T] - err[t_r], T - t_r]
    return out


class Cases:
    """lays CIGARs into one pool of words; (name, job, expected eight numbers)"""

    def __init__(self):
        self.words, self.jobs, self.want, self.names = [w(7, SOFT)], [], [], []      # (a word in front that no job may read)

    def add(self, name, words, weight=0, x_drop=0, min_rows=0):
        self.jobs.append((len(self.words), len(words), weight, x_drop, min_rows))
        self.want.append(rule(words, weight or W, x_drop or XDROP, min_rows or MIN_ROWS))
        assert self.want[-1] is not None, name
        self.names.append(name)
        self.words += [int(x) for x in words]

    def check(self, got):
        res = {}
        for name, g, e in zip(self.names, got.tolist(), self.want):
            assert g == e, (name, g, e)
            res[name] = g
        return res


def edge_cases():
    c = Cases()
    c.add("no tail", [w(1000, EQ), w(2, X), w(500, EQ)])
    c.add("right only", [w(1000, EQ), w(150, X)])
    c.add("left only", [w(150, X), w(1000, EQ)])
    c.add("both", [w(150, X), w(1000, EQ), w(1, DEL), w(400, EQ), w(90, INS), w(5, EQ), w(60, X)])
    c.add("tie of the maximum: the first wins", [w(500, EQ), w(1, X), w(3, EQ), w(200, X)])
    c.add("tie of the minimum: the last wins", [w(200, X), w(3, EQ), w(1, X), w(500, EQ)])
    c.add("maximum at boundary 0", [w(90, X), w(150, EQ)])
    c.add("a drop of exactly X", [w(1000, EQ), w(33, X)], x_drop=99, min_rows=10)
    c.add("a drop of X + 1", [w(1000, EQ), w(33, X)], x_drop=98, min_rows=10)
    c.add("one row short of min_tail_rows", [w(1000, EQ), w(99, X)])
    c.add("exactly min_tail_rows", [w(1000, EQ), w(100, X)])
    c.add("left tail one row short", [w(99, INS), w(1000, EQ)])
    c.add("t_L >= t_R", [w(200, X), w(50, EQ)])
    c.add("t_L >= t_R in the middle", [w(300, EQ), w(400, X), w(300, EQ)])
    big = (1 << 28) - 1
    # (scores beyond 2^31 and products error_weight * errors beyond 2^31; the second one's scores go down to -1.2e14)
    c.add("64-bit arithmetic", [w(big, EQ)] * 10 + [w(40000, X), w(big, EQ), w(big, EQ), w(1000, X)], weight=65535, x_drop=1 << 30, min_rows=(1 << 19) - 1)
    c.add("64-bit arithmetic, t_L >= t_R", [w(big, X), w(big, EQ)] * 7, weight=65535)
    c.add("T = 0", [])
    c.add("one word", [w(700, EQ)])
    c.add("one word of errors", [w(700, X)])
    c.add("deletions at the end", [w(1000, EQ), w(300, DEL)])                # no rows behind the maximum; the minimum at the end makes all of it a left tail
    c.add("other conventions", [w(40, X), w(300, EQ), w(30, INS)], weight=2, x_drop=29, min_rows=25)
    return c


def test_the_edge_cases_are_what_they_say():
    """not vacuous: the hand-made cases of the Python rule come out as their names say"""
    c = edge_cases()
    r = dict(zip(c.names, c.want))
    assert r["no tail"] == [0] * 8 and r["T = 0"] == [0] * 8 and r["one word"] == [0] * 8
    assert r["right only"] == [0, 0, 0, 0, 150, 150, 150, 1] and r["left only"] == [150, 150, 150, 1, 0, 0, 0, 0]
    assert r["both"] == [150, 150, 150, 1, 155, 65, 150, 3]
    assert r["tie of the maximum: the first wins"] == [0, 0, 0, 0, 204, 204, 201, 3]
    assert r["tie of the minimum: the last wins"] == [204, 204, 201, 3, 0, 0, 0, 0]
    assert r["maximum at boundary 0"] == [0, 0, 0, 0, 240, 240, 90, 2]
    assert r["a drop of exactly X"] == [0] * 8 and r["a drop of X + 1"] == [0, 0, 0, 0, 33, 33, 33, 1]
    assert r["one row short of min_tail_rows"] == [0] * 8 and r["exactly min_tail_rows"][4:] == [100, 100, 100, 1]
    assert r["left tail one row short"] == [0] * 8
    assert r["t_L >= t_R"] == [0] * 8 and r["t_L >= t_R in the middle"] == [0] * 8
    big = (1 << 28) - 1
    assert r["64-bit arithmetic"] == [0, 0, 0, 0, 41000 + 2 * big, 41000 + 2 * big, 41000, 4] and r["64-bit arithmetic, t_L >= t_R"] == [0] * 8
    assert r["one word of errors"] == [0] * 8 and r["deletions at the end"] == [1000, 1300, 300, 2, 0, 0, 0, 0]
    assert r["other conventions"] == [40, 40, 40, 1, 30, 0, 30, 1]


def random_cases(seed, n, max_words):
    rng = np.random.default_rng(seed)
    c = Cases()
    for i in range(n):
        T = int(rng.integers(1, max_words + 1))
        junk = (rng.random() < 0.4, rng.random() < 0.4)
        words = []
        for t in range(T):
            in_junk = (junk[0] and t < T // 6) or (junk[1] and t >= T - T // 6)
            if t % 2 == 0 and not in_junk:
                words.append(w(int(rng.integers(1, 120)), EQ))
            elif in_junk and rng.random() < 0.25:
                words.append(w(int(rng.integers(1, 4)), EQ))
            else:
                words.append(w(int(rng.integers(1, 25 if in_junk else 4)), (X, INS, DEL)[int(rng.integers(0, 3))]))
        if i % 4 == 0:
            c.add(f"random {i}", words, int(rng.integers(1, 9)), int(rng.integers(1, 200)), int(rng.integers(1, 150)))
        else:
            c.add(f"random {i}", words)
    return c


def test_host_rule_on_hand_made_cases():
    c = edge_cases()
    c.check(F.cigar_tails(c.words, c.jobs))


def test_host_rule_on_500_random_cigars():
    c = random_cases(7, 500, 300)
    c.check(F.cigar_tails(c.words, c.jobs))
    kinds = [(any(x[:4]), any(x[4:])) for x in c.want]
    assert kinds.count((True, False)) > 20 and kinds.count((False, True)) > 20 and kinds.count((True, True)) > 5 and kinds.count((False, False)) > 100


def test_bad_jobs_are_refused():
    words = [w(10, EQ), w(3, X), w(5, SOFT), w(4, 0), w(9, EQ)]
    for bad in ((0, 6), (6, 0), (4, 2), (1 << 40, 1), (1, 2), (3, 1), (0, 1, 65536), (0, 1, 0, (1 << 30) + 1), (0, 1, 0, 0, 1 << 19)):
        with pytest.raises(F.FloxerError):
            F.cigar_tails(words, [(0, 2), bad])
    big = [w((1 << 28) - 1, EQ)] * 17
    with pytest.raises(F.FloxerError, match="2\\^32"):
        F.cigar_tails(big, [(0, 17)])
    assert F.cigar_tails(big, [(0, 16), (1, 16)]).tolist() == [[0] * 8] * 2
    assert F.cigar_tails(words, [(0, 2), (4, 1), (5, 0), (0, 0), (0, 2, 65535, 1 << 30, (1 << 19) - 1)]).tolist() == [[0] * 8] * 5
    assert F.cigar_tails([], []).shape == (0, 8) and F.cigar_tails([], [(0, 0)]).tolist() == [[0] * 8]
    # the kernel's seam judges its jobs on the host as well, and a null context is refused
    L = capi.lib()
    pool = np.array(words, dtype=np.uint32)
    job = (capi.TailJob * 1)(capi.TailJob(0, 2, 0, 0, 0))
    res = (capi.TailResult * 1)()
    assert L.flx_cigar_tails_batch(None, capi.ptr(pool, capi.u32p), len(pool), job, 1, res) == -1 and b"null" in L.flx_last_error()
    assert L.flx_cigar_tails(None, 0, job, 1, res) == -1 and b"outside the pool" in L.flx_last_error()
    assert L.flx_cigar_tails(capi.ptr(pool, capi.u32p), len(pool), None, 1, res) == -1 and b"null" in L.flx_last_error()


# ------------------------------------------------------------------------------------------------ layouts, symbols, options
def test_struct_layouts_exported_symbols_and_defaults():
    assert C.sizeof(capi.SplitOptions) == 32 and C.sizeof(capi.TailJob) == 24 and C.sizeof(capi.TailResult) == 32
    assert [getattr(capi.SplitOptions, f).offset for f in ("enable", "error_weight", "x_drop", "min_tail_rows", "reserved")] == [0, 4, 8, 12, 16]
    assert [getattr(capi.TailJob, f).offset for f in ("cigar_offset", "cigar_length", "error_weight", "x_drop", "min_tail_rows")] == [0, 8, 12, 16, 20]
    assert [getattr(capi.TailResult, f).offset for f in F.TAIL_FIELDS] == list(range(0, 32, 4))
    assert C.sizeof(capi.RunOptions) == 64 and C.sizeof(capi.PathCounters) == 128        # the frozen structs keep their sizes
    new = {"flx_align_reads_split", "flx_align_reads_resident_split", "flx_cigar_tails", "flx_cigar_tails_batch"}
    assert set(capi.EXPORTED) >= new
    for name in capi.EXPORTED:
        assert hasattr(capi.lib(), name), name
    o = F.split_options()
    assert (o.enable, o.error_weight, o.x_drop, o.min_tail_rows, list(o.reserved)) == (1, 0, 0, 0, [0] * 4)
    o = F.split_options(error_weight=2, x_drop=30, min_tail_rows=50, enable=False)
    assert (o.enable, o.error_weight, o.x_drop, o.min_tail_rows) == (0, 2, 30, 50)
    with pytest.raises(F.FloxerError):
        F.split_options(min_tail_rows=-1)
    # a zero in a job's last three fields is the default
    words = [w(1000, EQ), w(150, X)]
    assert F.cigar_tails(words, [(0, 2), (0, 2, W, XDROP, MIN_ROWS), (0, 2, 0, 0, 151)]).tolist() == [[0, 0, 0, 0, 150, 150, 150, 1]] * 2 + [[0] * 8]


def test_options_are_judged_before_the_context_is_looked_at():
    L = capi.lib()
    p = F.params(error_probability=0.05)
    run = C.c_void_p()
    pool = np.ones(8, dtype=np.uint8)
    offs = np.array([0, 8], dtype=np.uint64)
    one = F.output_options(max_alignments=1)

    def call(split, partial=None, output=None, bundle=True, extend=None):
        b = capi.RunOptions()
        if partial is not None:
            b.partial = C.pointer(partial)
        if output is not None:
            b.output = C.pointer(output)
        if extend is not None:
            b.extend = C.pointer(extend)
        bp = C.byref(b) if bundle else None
        sp = C.byref(split) if split is not None else None
        # (no context at all: the options are judged first)
        a = L.flx_align_reads_split(None, C.byref(p), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), 1, bp, sp, C.byref(run))
        ea = L.flx_last_error()
        r = L.flx_align_reads_resident_split(None, C.byref(p), None, bp, sp, C.byref(run))
        assert a == r == -1
        return ea + b"|" + L.flx_last_error()

    part = F.partial_options()
    for k in range(4):
        s = F.split_options()
        s.reserved[k] = 1
        assert call(s, part, one).count(b"flx_split_options: the reserved fields") == 2, k
    s = F.split_options()
    s.enable = 2
    assert call(s, part, one).count(b"flx_split_options: enable must be 0 or 1") == 2
    assert call(F.split_options(error_weight=65536), part, one).count(b"error_weight") == 2
    assert call(F.split_options(x_drop=(1 << 30) + 1), part, one).count(b"x_drop") == 2
    assert call(F.split_options(min_tail_rows=1 << 19), part, one).count(b"min_tail_rows") == 2
    # split without partial: no bundle, no struct, a zeroed one, one switched off
    assert call(F.split_options(), bundle=False).count(b"needs flx_partial_options.enable") == 2
    for partial in (None, capi.PartialOptions(), F.partial_options(enable=False)):
        assert call(F.split_options(), partial, one).count(b"needs flx_partial_options.enable") == 2
    # split without -N 1
    for output in (None, capi.OutputOptions(), F.output_options(max_alignments=2), F.output_options(drop_duplicates=True)):
        assert call(F.split_options(), part, output).count(b"max_alignments_per_read == 1") == 2
    # split with without_cigar
    p.without_cigar = 1
    assert call(F.split_options(), part, one).count(b"flx_split_options.enable needs the CIGAR's trace") == 2
    p.without_cigar = 0
    # the bundle's own refusals still come
    e = F.extend_options()
    e.reserved[0] = 1
    assert call(F.split_options(), part, one, extend=e).count(b"flx_extend_options: the reserved fields") == 2
    # valid, or off (then it needs nothing): the refusal is the null context's
    for split, partial, output in ((F.split_options(error_weight=65535, x_drop=1 << 30, min_tail_rows=(1 << 19) - 1), part, one), (None, None, None),
                                   (capi.SplitOptions(), None, None), (F.split_options(enable=False, x_drop=7), None, F.output_options(max_alignments=3))):
        msg = call(split, partial, output)
        assert b"flx_split_options" not in msg and b"null" in msg, msg


# ------------------------------------------------------------------------------------------------ the rule header under sanitizers
def test_rule_header_against_a_quadratic_search_under_sanitizers(tmp_path):
    """tests/tails_check.cpp: flx_tails.hpp on 20 000 random CIGARs, built with ASan + UBSan"""
    exe = str(tmp_path / "tails_check")
    src = os.path.join(ROOT, "tests", "tails_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_flags(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    base = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"),
            "--output", str(tmp_path / "o.sam"), "-e", "2"]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0
    for name in ("--split-tails ", "--split-tails-weight <value>", "--split-tails-xdrop <value>", "--split-tails-min-rows <value>"):
        line = [l for l in h.stderr.decode().splitlines() if l.strip().startswith(name)]
        assert len(line) == 1 and line[0].startswith("      --") and "not floxer's" in line[0], name        # long spellings only
    env = dict(os.environ, FLX_CLI_PARSE_ONLY="1")               # the options are parsed, then only the reader runs (no GPU)
    ok = ["--partial-alignments", "-N", "1", "--split-tails"]
    for extra in (ok, ok + ["--sa-tag", "--partial-extend", "-Q", "--md-tag", "-D"],
                  ok + ["--split-tails-weight", "2", "--split-tails-xdrop=30", "--split-tails-min-rows", "524287"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and b"CLI PARSER ERROR" not in r.stderr, (extra, r.stderr)
    pa = "--partial-alignments"
    for extra in (["--split-tails"], ["-N", "1", "--split-tails"], [pa, "--split-tails"], [pa, "-N", "2", "--split-tails"], ok + ["-w"],
                  [pa, "-N", "1", "--split-tails-weight", "2"], [pa, "-N", "1", "--split-tails-xdrop", "30"], [pa, "-N", "1", "--split-tails-min-rows", "50"],
                  ok + ["--split-tails-weight", "0"], ok + ["--split-tails-weight", "65536"], ok + ["--split-tails-xdrop", "x"],
                  ok + ["--split-tails-min-rows", "524288"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr, extra
