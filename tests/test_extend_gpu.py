"""Extension of partial records on the GPU. The kernel alone (ed_extend through flx_extend_batch) against the numpy statement of the
rule in test_extend_host.py, (rows, cols, errors) exactly; then the pipeline on the shapes of test_partial_gpu.py: every kept record's
extended interval is the rule's, computed from the un-extended record's end cells, and the record passes the column-by-column check."""
import os
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
from floxer_amd import simulate as S
import oracle_lib as O
from test_extend_host import rule
from test_partial_gpu import (CHROM, LEN, RATE, Chimera, by_read, check_record, chimera_ok, letters, make_break_at_30, make_halves, mutate, oriented,
                              root_children, same, words_of)

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, XDROP, DMAX = 4, 100, 1024                                   # the defaults (include/floxer_amd.h)


# ------------------------------------------------------------------------------------------------ the kernel alone
class Jobs:
    """lays (query rows, reference symbols) pairs, given in walking order, into one query pool and one reference pool"""

    def __init__(self):
        rng = np.random.default_rng(77)
        self.q, self.t, self.jobs, self.want, self.names = [rng.integers(1, 5, size=9)], [rng.integers(1, 5, size=5)], [], [], []
        self.nq, self.nt = 9, 5

    def add(self, name, q, t, direction=1, w=0, x=0, dm=0, row_limit=None, ref_limit=None):
        q, t = np.asarray(q, dtype=np.uint8), np.asarray(t, dtype=np.uint8)
        il = len(q) if row_limit is None else row_limit
        jl = len(t) if ref_limit is None else ref_limit
        if direction == 1:
            qp, tp = self.nq, self.nt
            self.q.append(q), self.t.append(t)
        else:
            qp, tp = self.nq + len(q) - 1, self.nt + len(t) - 1
            self.q.append(q[::-1]), self.t.append(t[::-1])
        self.nq, self.nt = self.nq + len(q), self.nt + len(t)
        self.jobs.append((tp, jl, qp, il, direction, w, x, dm))
        self.want.append(rule(q[:il], t[:jl], w or W, x or XDROP, dm or DMAX))
        self.names.append(name)

    def both(self, name, q, t, **kw):
        self.add(name + " +", q, t, 1, **kw)
        self.add(name + " -", q, t, -1, **kw)

    def run(self, ctx, own_pool=True):
        q, t = np.concatenate(self.q), np.concatenate(self.t)
        got = F.extend_batch(ctx, q, self.jobs, reference_pool=t if own_pool else None)
        for name, g, e in zip(self.names, got.tolist(), self.want):
            assert tuple(g) == tuple(e), (name, g, e)
        return got


def other(x):
    return 1 + x % 4


def with_errors(rng, t, positions, kind="X"):
    """t with one edit at each of the (ascending, well separated) positions: X substitution, I an extra query base, D a base left out"""
    q = list(t)
    for p in sorted(positions, reverse=True):
        if kind == "X":
            q[p] = other(q[p])
        elif kind == "I":
            q.insert(p, other(q[p]))
        else:
            del q[p]
    return np.array(q, dtype=np.uint8)


@pytest.fixture(scope="module")
def small_ctx():
    ref = np.random.default_rng(5).integers(1, 5, size=6000, dtype=np.uint8)
    ctx = F.context(F.fmindex([ref]))
    yield ctx, ref
    ctx.close()


@gpu
def test_kernel_matches_the_rule_on_its_edge_cases(small_ctx):
    ctx, _ = small_ctx
    rng = np.random.default_rng(11)
    rnd = lambda n: rng.integers(1, 5, size=n, dtype=np.uint8)
    J = Jobs()
    t = rnd(400)
    J.both("all matches up to row_limit", t[:300], t)
    J.both("all matches, no room at all", t[:0], t)
    J.both("no reference symbols", t[:50], t[:0])
    q = rnd(300)
    q[0] = other(t[0])
    J.both("first symbol mismatch, then random", q, t)
    for run in (7, 8, 9, 63, 64, 65):                              # the compare-word boundaries
        t = rnd(run + 300)
        q = np.concatenate([with_errors(rng, t[: run + 60], [run]), rnd(200)])
        J.both(f"match run of {run}", q, t)
        J.both(f"match run of {run}, then the last row", t[:run], t)
        J.both(f"match run of {run}, then the last symbol", t[: run + 30], t[:run])
    t = rnd(500)
    J.both("ref_limit reached before the rows", t[:200], t, ref_limit=50)
    J.both("row_limit cuts the rows", t[:200], t, row_limit=64)
    for n_err in (31, 32, 33, 70):                                # the wavefront outgrows one stride of 64 diagonals
        t = rnd(12 * n_err + 40)
        q = with_errors(rng, t, [12 * e + 11 for e in range(n_err)], "XID"[n_err % 3])
        J.both(f"{n_err} errors", q, t)
    for kind in "ID":                                             # drift to kappa = -40 / +40
        t = rnd(15 * 40 + 60)
        J.both(f"{kind}-only drift", with_errors(rng, t, [15 * e + 14 for e in range(40)], kind), t)
    # a valley of 30 random rows, then 500 rows that match again on the same diagonal: behind the x-drop the rule does not look
    t = rnd(700)
    q = np.concatenate([t[:60], rnd(30), t[90:590]])
    J.both("valley deeper than x_drop", q, t, x=20)
    J.both("the same valley within x_drop", q, t, x=400)
    t = rnd(600)
    q = with_errors(rng, t, [10 * e + 9 for e in range(40)])
    J.both("max_errors hit", q, t, dm=16)
    t = rnd(400)
    q = with_errors(rng, t, [5 * e + 4 for e in range(60)])
    J.both("error_weight 2", q, t, w=2)
    J.both("error_weight 8", q, t, w=8)
    got = J.run(ctx)
    res = dict(zip(J.names, got.tolist()))
    # not vacuous: what the cases are about did happen
    assert res["all matches up to row_limit +"] == [300, 300, 0, 2] and res["first symbol mismatch, then random +"][:3] == [0, 0, 0]
    assert res["ref_limit reached before the rows +"][:3] == [50, 50, 0] and res["row_limit cuts the rows -"] == [64, 64, 0, 2]
    for n_err in (31, 32, 33, 70):
        assert res[f"{n_err} errors +"][2] == n_err and res[f"{n_err} errors -"][2] == n_err
    assert res["I-only drift +"][0] - res["I-only drift +"][1] == 40 and res["D-only drift -"][1] - res["D-only drift -"][0] == 40
    assert res["valley deeper than x_drop +"] == [60, 60, 0, 1] and res["the same valley within x_drop +"][0] == 590
    assert res["max_errors hit +"][2:] == [16, 3] and res["max_errors hit +"][0] == 169
    assert res["error_weight 2 +"][0] > 200 and res["error_weight 8 +"][0] == 4
    # direction -1 on mirrored inputs gives the mirrored result: the same numbers
    for name in J.names:
        if name.endswith(" +"):
            assert res[name][:3] == res[name[:-1] + "-"][:3], name


def matrix(q, t):
    """D[i][j], the unit-cost edit distance between the first i rows and the first j symbols (D[0][0] = 0), every cell, row by row"""
    q, t = np.asarray(q, dtype=np.int64), np.asarray(t, dtype=np.int64)
    js = np.arange(len(t) + 1)
    D = np.zeros((len(q) + 1, len(t) + 1), dtype=np.int64)
    D[0] = js
    for i in range(1, len(q) + 1):
        cand = D[i - 1] + 1
        cand[1:] = np.minimum(cand[1:], D[i - 1][:-1] + (t != q[i - 1]))
        D[i] = np.minimum.accumulate(cand - js) + js
    return D


def scan(D, weight):
    """per d = 0 .. m(last row): (R(d), score(d), the running maximum's drop G(d) - score(d)) read off the matrix"""
    mins = D.min(axis=1)
    out, G = [], None
    for d in range(int(mins[-1]) + 1):
        R = int(np.flatnonzero(mins <= d)[-1])
        score = R - weight * d
        G = score if G is None else max(G, score)
        out.append((R, score, G - score))
    return out


@gpu
def test_kernel_ties_of_the_diagonal_the_drop_and_the_stop_reasons(small_ctx):
    """three situations the random jobs do not hold, each shown on the full matrix before the kernel is asked: two diagonals that reach
    R(d*) (the smallest column wins), a drop of exactly x_drop in front of a new maximum (the scan goes on: the test is strict), and a
    step at which the drop exceeds x_drop and the last row is reached together (the reason is the x-drop, which is asked first)."""
    ctx, _ = small_ctx
    rng = np.random.default_rng(21)
    rnd = lambda n: rng.integers(1, 5, size=n, dtype=np.uint8)
    J = Jobs()
    # 1. behind 30 exact rows: a substitution on diagonal 0 or a deleted symbol on diagonal +1, then 20 rows of one letter on either
    P = rnd(30)
    P[-1] = 2
    q = np.concatenate([P, np.full(20, 1), np.full(40, 3)]).astype(np.uint8)
    t = np.concatenate([P, [2], np.full(21, 1), np.full(60, 4)]).astype(np.uint8)
    i1, j1, d1, _ = rule(q, t)
    D = matrix(q, t)
    assert (i1, d1) == (50, 1) and np.flatnonzero(D[i1] == d1).tolist() == [50, 51] and j1 == 50
    J.both("two diagonals reach R(1)", q, t)
    # 2. a valley of 8 substitutions, exactly x_drop deep, and 232 exact rows behind it
    t = rnd(400)
    q = np.concatenate([t[:60], [other(x) for x in t[60:68]], t[68:300]]).astype(np.uint8)
    steps = scan(matrix(q, t), W)
    depth = max(drop for _, _, drop in steps)
    floor = [d for d, (_, _, drop) in enumerate(steps) if drop == depth]
    assert depth > 0 and floor and steps[-1][0] == 300 and steps[-1][2] == 0 and len(steps) - 1 > floor[-1]      # the last d is the new maximum
    assert rule(q, t, W, depth, DMAX) == (300, 300, len(steps) - 1, 2) and rule(q, t, W, depth - 1, DMAX)[:3] == (60, 60, 0)
    J.both("a drop of exactly x_drop, then a new maximum", q, t, x=depth)
    J.both("a drop of x_drop + 1", q, t, x=depth - 1)
    # 3. 60 exact rows and 30 substituted ones to the last row; x_drop one below the drop at the d that reaches it
    t = rnd(200)
    q = np.concatenate([t[:60], [other(x) for x in t[60:90]]]).astype(np.uint8)
    steps = scan(matrix(q, t), W)
    d_last = len(steps) - 1
    assert steps[d_last][0] == 90 and all(R < 90 for R, _, _ in steps[:-1])
    x = steps[d_last][2] - 1
    assert x >= 1 and all(drop <= x for _, _, drop in steps[:-1])                 # no earlier step stops the scan
    assert rule(q, t, W, x, DMAX) == (60, 60, 0, 1) and rule(q, t, W, x + 1, DMAX) == (60, 60, 0, 2)
    J.both("the drop and the last row in one step", q, t, x=x)
    J.both("the last row one step before the drop", q, t, x=x + 1)
    J.run(ctx)


@gpu
def test_kernel_300_random_jobs_in_one_launch_and_the_contexts_text(small_ctx):
    ctx, ref = small_ctx
    rng = np.random.default_rng(12)
    J = Jobs()
    for n in range(300):
        L = int(rng.integers(100, 400))
        t = rng.integers(1, 5, size=L + 150, dtype=np.uint8)
        q = list(t[:L])
        for _ in range(max(1, int(L * rng.uniform(0.01, 0.15)))):
            p = int(rng.integers(0, len(q)))
            kind = int(rng.integers(0, 3))
            if kind == 0:
                q[p] = other(q[p])
            elif kind == 1:
                q.insert(p, int(rng.integers(1, 5)))
            else:
                del q[p]
        q = np.concatenate([np.array(q, dtype=np.uint8), rng.integers(1, 5, size=150, dtype=np.uint8)])
        J.add(f"random {n}", q, t, 1 if n % 2 else -1)
    got = J.run(ctx)
    assert (got[:, 0] > 80).sum() > 200
    # ref_pool NULL: the context's text. Rows of the reference itself, with errors, in both directions, up to the text's ends
    q = with_errors(rng, ref[1000:1400], [50, 51, 200, 333])
    qpool = np.concatenate([q, ref[:300]])
    jobs = [(1000, 5000, 0, 400, 1, 0, 0, 0), (1399, 1400, 399, 400, -1, 0, 0, 0), (299, 300, 699, 300, -1, 0, 0, 0), (5700, 300, 400, 300, 1, 0, 0, 0)]
    got = F.extend_batch(ctx, qpool, jobs).tolist()
    assert got[0] == list(rule(q, ref[1000:])) and got[1] == list(rule(q[::-1], ref[:1400][::-1])) and got[0][:3] == [400, 400, 4]
    assert got[2] == [300, 300, 0, 2] and got[3] == list(rule(ref[:300], ref[5700:]))
    # jobs outside their pools and bad values are refused
    for bad in ((5000, 1100, 0, 10, 1, 0, 0, 0), (10, 12, 0, 10, -1, 0, 0, 0), (0, 10, 695, 10, 1, 0, 0, 0), (0, 10, 5, 7, -1, 0, 0, 0),
                (0, 10, 0, 10, 0, 0, 0, 0), (0, 10, 0, 10, 1, 0, 0, 4094), (0, 10, 0, 10, 1, 65536, 0, 0)):
        with pytest.raises(F.FloxerError):
            F.extend_batch(ctx, qpool, [bad])


# ------------------------------------------------------------------------------------------------ the pipeline
def make_break_at(rng, chroms, brk, second_strand=0):
    """two loci joined at row brk, 1 % errors on either side; second_strand 1: the second part comes from the other strand (an
    fr-chimera whose break lies inside a node). What comes out is not given here: the rule decides."""
    k, _ = root_children()
    ca, cb = (int(x) for x in rng.integers(0, len(chroms), size=2))
    pa, pb = int(rng.integers(1000, CHROM // 2 - LEN)), int(rng.integers(CHROM // 2, CHROM - LEN - 1000))
    sa = mutate(rng, chroms[ca][pa: pa + brk], brk // 100)
    sb = mutate(rng, chroms[cb][pb: pb + LEN - brk], (LEN - brk) // 100)
    read = np.concatenate([sa, O.revcomp(sb) if second_strand else sb])
    win = lambda ch, p, o: (o, ch, p - LEN - k, p + 2 * LEN + k)
    return Chimera(read, [], [win(ca, pa, 0), win(cb, pb, second_strand)] + ([win(ca, pa, 1), win(cb, pb, 0)] if second_strand else []))


def build_batch():
    pool, chroms = S.make_genome_fast(CHROM, 2, seed=41)
    (rp, ro), _ = S.make_reads_fast(pool, [CHROM, CHROM], 6, 3000, 0.04, seed=42)
    reads = [rp[int(ro[i]): int(ro[i + 1])].copy() for i in range(6)]
    rng = np.random.default_rng(47)
    k, _ = root_children()
    groups = dict(halves=[], at1800=[], at4100=[], fr=[])

    def draw(group, make, *a):
        for _ in range(20):
            c = make(rng, chroms, *a)
            if chimera_ok(chroms, k, c):
                groups[group].append(len(reads))
                reads.append(c.read)
                return
        raise AssertionError("no chimera that the CPU agrees with in 20 draws")

    for kind in ("ff", "rr", "fr"):
        draw("halves", make_halves, kind, 0.5)
    for _ in range(2):
        draw("at1800", make_break_at_30)
        draw("at4100", make_break_at, 4100)
    draw("fr", make_break_at, 1800, 1)
    reads.append(rng.integers(1, 5, size=LEN, dtype=np.uint8))          # unmapped, and no part of it aligns anywhere
    reads += [np.zeros(0, np.uint8), np.array([1, 2, 3], np.uint8)]     # skipped
    return chroms, reads, groups


@pytest.fixture(scope="module")
def world():
    chroms, reads, groups = build_batch()
    ctx = F.context(F.fmindex(chroms))
    p = F.params(error_probability=RATE)
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_stats()
    ctx.path_counters(reset=True)
    base = F.aligner(ctx, p, F.output_options(mapq=True), md=True, partial=F.partial_options()).align_reads(reads)
    stats_off, pc_off = ctx.kernel_stats(), ctx.path_counters(reset=True)
    ext = F.aligner(ctx, p, F.output_options(mapq=True), md=True, partial=F.partial_options(), extend=F.extend_options()).align_reads(reads)
    stats_on, pc_on = ctx.kernel_stats(), ctx.path_counters(reset=True)
    ctx.enable_kernel_timing(False)
    yield dict(chroms=chroms, reads=reads, groups=groups, ctx=ctx, p=p, base=base, ext=ext, stats_off=stats_off, stats_on=stats_on, pc_off=pc_off, pc_on=pc_on)
    ctx.close()


def core_of(rec):
    """(oriented from, oriented to, reference end) of a record"""
    ops = words_of(rec[5])
    lead = ops[0][0] if ops[0][1] == "S" else 0
    trail = ops[-1][0] if ops[-1][1] == "S" and len(ops) > 1 else 0
    span = sum(n for n, op in ops if op in "=XD")
    rows = sum(n for n, op in ops if op in "=XI")
    return lead, lead + rows - 1, rec[3] + span, trail


def expected_moves(chroms, read, recs, options=(W, XDROP, DMAX)):
    """the rule on both ends of every record of a read (its un-extended records): [((iL, jL, dL), (iR, jR, dR))]"""
    n = len(read)
    fwd = []
    for rec in recs:
        frm, to, _, _ = core_of(rec)
        fwd.append((n - 1 - to, n - 1 - frm) if rec[1] & 16 else (frm, to))
    out = []
    for rec, (f, t) in zip(recs, fwd):
        left, right = f, n - 1 - t
        for of, ot in fwd:
            if ot < f:
                left = min(left, f - 1 - ot)
            elif of > t:
                right = min(right, of - 1 - t)
        rc = bool(rec[1] & 16)
        q = oriented(read, 1 if rc else 0)
        frm, to, ref_end, _ = core_of(rec)
        rows_right, rows_left = (left, right) if rc else (right, left)
        ref = chroms[rec[2]]
        r = rule(q[to + 1: to + 1 + rows_right], ref[ref_end: ref_end + rows_right + DMAX], *options)
        lo = max(0, rec[3] - rows_left - DMAX)
        l = rule(q[frm - rows_left: frm][::-1], ref[lo: rec[3]][::-1], *options)
        out.append((l[:3], r[:3]))
    return out


def check_extended(chroms, reads, base, ext, read_ids, options=(W, XDROP, DMAX)):
    rb, re_ = by_read(base), by_read(ext)
    moved = 0
    for i in read_ids:
        recs, new = [r for _, r in rb[i]], [r for _, r in re_[i]]
        assert [r[1] for r in recs] == [r[1] for r in new] and [r[2] for r in recs] == [r[2] for r in new], i      # flags, order, references
        for rec, got, (jb, _), (je, _), (l, r) in zip(recs, new, rb[i], re_[i], expected_moves(chroms, reads[i], recs, options)):
            frm, to, _, _ = core_of(rec)
            fwd, ori = check_record(chroms, reads[i], got, ext.md[je] if ext.md else None)
            assert ori == (frm - l[0], to + r[0]), (i, rec[:5], ori, l, r)
            assert got[4] <= rec[4] + l[2] + r[2], (i, got[4], rec[4], l, r)
            if l[0] == 0 and r[0] == 0:                              # did not move: its words, byte for byte
                assert got == rec and (ext.md is None or ext.md[je] == base.md[jb])
            else:
                moved += 1
            assert int(ext.mapq[je]) == int(base.mapq[jb])            # MAPQ keeps the value computed before the extension
    return moved


@gpu
def test_extended_intervals_are_the_rules_and_records_check_out(world):
    w = world
    g = w["groups"]
    chim = g["halves"] + g["at1800"] + g["at4100"] + g["fr"]
    moved = check_extended(w["chroms"], w["reads"], w["base"], w["ext"], chim)
    assert moved >= 2 * (len(g["at1800"]) + len(g["at4100"]) + len(g["fr"]))
    iv = w["ext"].query_intervals([len(r) for r in w["reads"]])
    rows = by_read(w["ext"])
    for i in g["at1800"] + g["fr"]:                                  # the two records now meet at the break, within x_drop rows on each side
        (a, b) = sorted(tuple(iv[j]) for j, _ in rows[i])
        assert len(rows[i]) == 2 and abs(a[1] + 1 - 1800) <= XDROP and abs(b[0] - 1800) <= XDROP, (i, a, b)
    for i in g["at4100"]:
        (a, b) = sorted(tuple(iv[j]) for j, _ in rows[i])
        assert len(rows[i]) == 2 and abs(a[1] + 1 - 4100) <= XDROP and abs(b[0] - 4100) <= XDROP, (i, a, b)
    for i in g["fr"]:
        assert sorted(r[1] & 16 for _, r in rows[i]) == [0, 16]
    # the un-extended run left the well-aligning bases clipped: this is what the option is for
    iv0 = w["base"].query_intervals([len(r) for r in w["reads"]])
    for i in g["at1800"]:
        (a, b) = sorted(tuple(iv0[j]) for j, _ in by_read(w["base"])[i])
        assert b[0] - a[1] > 1000


@gpu
def test_everything_else_is_unchanged_and_off_launches_nothing(world):
    w = world
    base, ext, reads = w["base"], w["ext"], w["reads"]
    rb, re_ = by_read(base), by_read(ext)
    n = len(reads)
    for i in list(range(6)) + [n - 3]:                              # mapped reads and the random read: word for word
        assert [r for _, r in rb[i]] == [r for _, r in re_[i]]
        for (j, _), (j0, _) in zip(re_[i], rb[i]):
            a, b = ext.rows[j], base.rows[j0]
            assert (ext.cigars[a[5]: a[5] + a[6]] == base.cigars[b[5]: b[5] + b[6]]).all() and ext.md[j] == base.md[j0] and ext.mapq[j] == base.mapq[j0]
    assert [r[1] for _, r in re_[n - 3]] == [4] and ext.skipped.tolist() == base.skipped.tolist() and ext.skipped.tolist()[-2:] == [1, 1]
    assert len(ext.raw) == len(base.raw) and (ext.raw["read"] == base.raw["read"]).all() and (ext.raw["flag"] == base.raw["flag"]).all()
    for key in ("reads_rescued", "partial_records", "records", "reads", "root_alignments_found"):
        assert w["pc_on"][key] == w["pc_off"][key], key
    assert w["pc_on"]["reads_rescued"] == sum(len(v) for v in w["groups"].values())
    # with the option off the kernel statistics hold no ed_extend launch; with it on one launch per slice, its work in wavefront cells
    assert "ed_extend" not in w["stats_off"]
    st = w["stats_on"]["ed_extend"]
    assert st["launches"] == 1 and st["work_units"] > 0 and st["device_ms"] > 0
    # a NULL or zeroed extend struct, or enable = 0, is the un-extended run
    for e in (capi.ExtendOptions(), F.extend_options(enable=False)):
        off = F.aligner(w["ctx"], w["p"], F.output_options(mapq=True), md=True, partial=F.partial_options(), extend=e).align_reads(reads)
        same(off, base)
        assert off.md == base.md and off.mapq.tolist() == base.mapq.tolist()
        # (every record's words, not the whole pools: a trace job's slab is 2 NM + 2 words and those the CIGAR does not fill are unset)
        for a, b in zip(off.rows, base.rows):
            assert (off.cigars[a[5]: a[5] + a[6]] == base.cigars[b[5]: b[5] + b[6]]).all()
    with pytest.raises(F.FloxerError, match="needs flx_partial_options"):
        F.aligner(w["ctx"], w["p"], extend=F.extend_options()).align_reads(reads)


@gpu
def test_same_records_for_resident_reads_a_cut_batch_and_other_parameters(world, monkeypatch):
    w = world
    ctx, p, reads, ext = w["ctx"], w["p"], w["reads"], w["ext"]
    al = F.aligner(ctx, p, F.output_options(mapq=True), md=True, partial=F.partial_options(), extend=F.extend_options())
    rr = F.resident_reads(ctx, reads)
    resident = al.align_reads(rr)
    rr.close()
    monkeypatch.setenv("FLX_CHUNK_READS", str((len(reads) + 1) // 2))
    cut = al.align_reads(reads)
    monkeypatch.delenv("FLX_CHUNK_READS")
    for other_run in (resident, cut):
        same(other_run, ext)
        assert other_run.md == ext.md and other_run.mapq.tolist() == ext.mapq.tolist()
    # other conventions: the rule with them
    g = w["groups"]
    chim = g["at1800"][:1] + g["at4100"][:1] + g["fr"]
    opts = (2, 30, 16)
    base = F.aligner(ctx, p, partial=F.partial_options()).align_reads(reads)
    run = F.aligner(ctx, p, partial=F.partial_options(), extend=F.extend_options(*opts)).align_reads(reads)
    assert check_extended(w["chroms"], reads, base, run, chim, opts) >= 1


def sa_strings(records, names, mapqs):
    """the SA:Z value of every record, from the run's records: the read's other records in written order"""
    def entry(r, q):
        ops, merged = words_of(r[5]), []
        for n, op in ops:
            op = "M" if op in "=X" else op
            if merged and merged[-1][1] == op == "M":
                merged[-1] = (merged[-1][0] + n, "M")
            else:
                merged.append((n, op))
        return f"{names[r[2]]},{r[3] + 1},{'-' if r[1] & 16 else '+'},{''.join(f'{n}{op}' for n, op in merged)},{q},{r[4]};"
    out = []
    for i, r in enumerate(records):
        mates = [j for j, o in enumerate(records) if o[0] == r[0]]
        out.append("".join(entry(records[j], mapqs[j]) for j in mates if j != i) if any(records[j][1] & 2048 for j in mates) else None)
    return out


@gpu
def test_cli_writes_the_librarys_records_with_sa(world, tmp_path):
    w = world
    chroms, reads, ext = w["chroms"], w["reads"], w["ext"]
    keep = [i for i, r in enumerate(reads) if len(r) > 100]
    fasta, fastq = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq")
    with open(fasta, "w") as f:
        for i, c in enumerate(chroms):
            f.write(f">chr{i}\n" + "\n".join(letters(c[o: o + 100]) for o in range(0, len(c), 100)) + "\n")
    with open(fastq, "w") as f:
        for i in keep:
            f.write(f"@read{i}\n{letters(reads[i])}\n+\n{'I' * len(reads[i])}\n")
    assert keep == list(range(len(keep)))                            # (the skipped reads are the last two: read indices are the file's)
    recs = [r for r in ext.records() if r[0] in keep]
    names = [f"chr{i}" for i in range(len(chroms))]
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    for with_q in (False, True):
        out = str(tmp_path / f"out{int(with_q)}.sam")
        r = subprocess.run([exe, "--reference", fasta, "--queries", fastq, "--output", out, "--error-probability", str(RATE), "--threads", "2",
                            "--partial-alignments", "--partial-extend", "--sa-tag", "--md-tag"] + (["-Q"] if with_q else []),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        mapqs = ext.mapq.tolist() if with_q else [255] * len(recs)
        want_sa = sa_strings(recs, names, mapqs)
        got = []
        for line in open(out).read().splitlines():
            if line.startswith("@"):
                continue
            f = line.split("\t")
            tags = dict((t[:2], t[5:]) for t in f[11:])
            assert [t[:2] for t in f[11:]] == [k for k in ("NM", "MD", "SA") if k in tags]
            got.append(((int(f[0][4:]), int(f[1]), -1 if f[2] == "*" else names.index(f[2]), int(f[3]) - 1, int(tags.get("NM", 0)), "" if f[5] == "*" else f[5]),
                        int(f[4]), tags.get("MD"), tags.get("SA")))
        assert [x[0] for x in got] == recs
        assert [x[1] for x in got] == mapqs
        assert [x[2] for x in got] == [m.decode() if m else None for m in ext.md[: len(recs)]]
        assert [x[3] for x in got] == want_sa
        assert sum(1 for s in want_sa if s) == 2 * sum(len(v) for v in w["groups"].values())
