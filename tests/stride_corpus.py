"""Stride corpus: periodic inputs that run every capped launch past its grid. Most kernels behind the DP stages give one wave (or one
thread) to one job and cap the grid (floxer_amd.grid_caps()); behind the cap a wave takes its next job in a loop and carries state over.
The corpus takes a list of P distinct small cases, P odd and hence coprime with every cap (the caps are powers of two), and cycles
them: job i is case i mod P. The job a wave takes in its next turn, i + cap, is then another case than the one it has just left, and
over a launch every ordered pair (case a, then case (a + cap) mod P) occurs in some wave. With n = 2 cap + P jobs every wave takes two
jobs and the first P waves three. Every expected value is a function of the case alone, so a reference runs P times, not n times.

Three kinds of cases:
  - PathCase: a true path over its own letters (reference window, query, first column) with optional soft clips, a strand and tail
    parameters. The passes over CIGAR words share them: cs, left-align and tails through the doors of the kernels alone, coverage,
    pileup, sv, errprof and the sort keys as records over one small world (text, lengths, reads) in which every case has its place.
  - align cases: (window, query, allowed errors) for the DP and traceback, whose own words md_build, cs_build and cigar_left_align
    then read; the expected paths are the oracle's.
  - extend cases: (query rows, reference symbols, parameters, direction) for ed_extend, laid out by test_extend_gpu.Jobs.
Nothing here needs a GPU."""
import numpy as np

import floxer_amd as F
import leftalign_ref as LA

EQ, X, INS, DEL, SOFT = 7, 8, 1, 2, 4
FLAGS = (0, 16, 2048, 2064)                                              # every one of them counts in every side object
COMPLEMENT = np.array([0, 4, 3, 2, 1, 5], dtype=np.uint8)
# (error_weight, x_drop, min_tail_rows) of the path cases in period order, 0: the defaults; chosen so that left tails, right tails and no
# tail all occur among paths this short
TAIL_PARAMS = ((0, 0, 0), (2, 2, 2), (2, 5, 3), (4, 3, 2), (1, 2, 1), (3, 4, 2), (2, 5, 3), (0, 0, 0), (3, 4, 2))


def caps():
    return F.grid_caps()


def n_jobs(cap, period, waves_per_block=1):
    """every wave takes two jobs, the first `period` waves three"""
    return 2 * cap * waves_per_block + period


def multiplicity(n, period):
    """how often each case occurs among jobs 0 .. n - 1"""
    return [n // period + (1 if c < n % period else 0) for c in range(period)]


def follower(a, cap, period):
    """the case a wave takes directly behind case a"""
    return (a + cap) % period


# ------------------------------------------------------------------------------------------------ path cases
class PathCase:
    def __init__(self, name, path, ref, qry, begin, lead=0, trail=0):
        self.name, self.path, self.begin, self.lead, self.trail = name, [(int(op), int(ln)) for op, ln in path], int(begin), int(lead), int(trail)
        self.ref, self.qry = np.asarray(ref, dtype=np.uint8), np.asarray(qry, dtype=np.uint8)

    def words(self):
        """the path's words, as the doors of the kernels alone take them"""
        return LA.words_of(self.path)

    def record_words(self):
        """the words of the case's record: the path between its soft clips"""
        return [(n << 4) | SOFT for n in (self.lead,) if n] + [int(w) for w in self.words()] + [(n << 4) | SOFT for n in (self.trail,) if n]

    def columns(self):
        return sum(ln for op, ln in self.path if op != INS)

    def key(self):
        return (tuple(self.path), self.ref.tobytes(), self.qry.tobytes(), self.begin, self.lead, self.trail)


def _true_path(name, path, seed, begin=2, ref=None, lead=0, trail=0):
    """letters that make the words true: a random window over A C G T (or the given one), the query read off it through the path"""
    rng = np.random.default_rng(seed)
    cols = sum(ln for op, ln in path if op != INS)
    if ref is None:
        ref = rng.integers(1, 5, size=begin + cols + 3)
    ref = np.asarray(ref, dtype=np.uint8)
    assert len(ref) >= begin + cols
    qry, r = [], begin
    for op, ln in path:
        if op == EQ:
            qry += [int(x) for x in ref[r: r + ln]]
        elif op == X:
            qry += [int(x) % 4 + 1 for x in ref[r: r + ln]]
        elif op == INS:
            qry += [int(x) for x in rng.integers(1, 5, size=ln)]
        if op != INS:
            r += ln
    return PathCase(name, path, ref, qry, begin, lead, trail)


def _alternating(n_words, long_at=21):
    """n_words words, '=' and X / I / D in turn; the word at long_at is three long (a gap: 21 // 2 % 3 == 1, an insertion)"""
    out = []
    for t in range(n_words):
        if t % 2 == 0:
            out.append((EQ, 1 + t % 3))
        else:
            out.append(((X, INS, DEL)[(t // 2) % 3], 3 if t == long_at else 1 + (t // 2) % 2))
    return out


def path_cases():
    """the P cases of the passes over CIGAR words, in period order"""
    a_run = [2, 3] + [1] * 20 + [4, 2, 3]                                # C G A x 20 T C G
    shift_ref = np.random.default_rng(8).integers(1, 5, size=40)
    shift_ref[8: 20] = 4                                                 # a run of twelve T: the deletion behind it moves left through it
    shift_ref[7] = 1
    return [
        _true_path("one_word", [(EQ, 37)], 1),
        _true_path("words_64", _alternating(64), 2, lead=5),             # exactly one pass; ends with an insertion
        _true_path("words_96", _alternating(96), 3, begin=0),            # two passes, carries at the end of the first; ends with a deletion
        # two deletions in one run of A: the second crosses the '=' between them whole and merges with the first (word by word)
        _true_path("merge", [(EQ, 4), (DEL, 1), (EQ, 3), (DEL, 2), (EQ, 6), (X, 1), (EQ, 4)], 4, begin=1, ref=a_run),
        _true_path("long_words", [(EQ, 100), (X, 70), (EQ, 3), (DEL, 70), (EQ, 2), (INS, 66), (EQ, 64)], 5, lead=3, trail=7),
        _true_path("open_match_run", [(EQ, 5), (X, 1), (EQ, 30)], 6),
        _true_path("ins_last", [(EQ, 8), (INS, 3), (EQ, 4), (DEL, 2), (X, 2), (EQ, 1), (INS, 5)], 7, trail=4),
        _true_path("shift", [(EQ, 14), (DEL, 3), (EQ, 9)], 8, begin=3, ref=shift_ref),
        _true_path("x_first", [(X, 3), (EQ, 10), (DEL, 1), (EQ, 1)], 9, begin=0),
    ]


def merges(case):
    """the rule joins two words of one op somewhere on the case's path: the kernel takes its word-by-word branch there"""
    out = LA.left_align(case.path, case.ref, case.qry, case.begin)
    return sum(op != EQ for op, _ in out) < sum(op != EQ for op, _ in case.path)


def pack_paths(cases):
    """(reference pool, query pool, words, jobs) of one period, as flx_left_align / flx_cs take them"""
    return LA.pack_jobs([(c.path, c.ref, c.qry, c.begin) for c in cases])


def cycle(period_items, n):
    """job i is item i mod P"""
    p = len(period_items)
    return [period_items[i % p] for i in range(n)]


def tail_jobs(cases):
    """one period of (cigar_offset, cigar_length, error_weight, x_drop, min_tail_rows) over pack_paths' words"""
    _, _, _, jobs = pack_paths(cases)
    return [(j[0], j[1]) + TAIL_PARAMS[i % len(TAIL_PARAMS)] for i, j in enumerate(jobs)]


# ------------------------------------------------------------------------------------------------ the cases as records
class World:
    """every case's window at its place in one of two sequences; one record and one read per case"""

    def __init__(self, cases):
        self.cases = cases
        parts, self.place = [[], []], []
        for c, case in enumerate(cases):
            ref = c % 2
            self.place.append((ref, sum(len(p) for p in parts[ref])))
            parts[ref].append(case.ref)
        self.text = [np.concatenate(p) for p in parts]
        self.lengths = [len(t) for t in self.text]
        self.concat = np.concatenate(self.text)
        rng = np.random.default_rng(99)
        self.rec = np.zeros(len(cases), dtype=F._REC_DTYPE)
        pool, self.reads = [], []
        for c, case in enumerate(cases):
            ws = case.record_words()
            flag = FLAGS[c % len(FLAGS)]
            nm = sum(ln for op, ln in case.path if op != EQ)
            self.rec[c] = (c, flag, self.place[c][0], self.place[c][1] + case.begin, nm, len(pool), len(ws), 0)
            pool += ws
            seq = np.concatenate([rng.integers(1, 5, size=case.lead), case.qry, rng.integers(1, 5, size=case.trail)]).astype(np.uint8)
            self.reads.append(COMPLEMENT[seq[::-1]] if flag & 16 else seq)      # (as given: SEQ is its reverse complement on the reverse strand)
        self.words = np.array(pool, dtype=np.uint32)
        self.read_lengths = [len(r) for r in self.reads]

    def records(self, n):
        """n records, record i the record of case i mod P; they share the period's words and reads"""
        p = len(self.rec)
        return np.tile(self.rec, n // p + 1)[:n].copy()


def sv_cases(cases, min_length):
    """the cases whose record carries at least one D or I word of min_length or more"""
    return [c for c in cases if any(op in (INS, DEL) and ln >= min_length for op, ln in c.path)]


# ------------------------------------------------------------------------------------------------ align cases
def align_cases():
    """[(name, window, query, allowed errors)]: the query is a stretch of the window with the named edits"""
    rng = np.random.default_rng(41)
    out = []

    def sub(q, at):                                                      # a letter that its column and both neighbours do not hold
        q0 = q.copy()
        for p in at:
            q[p] = min(set((1, 2, 3, 4)) - {int(q0[max(p - 1, 0)]), int(q0[p]), int(q0[min(p + 1, len(q0) - 1)])})
        return q

    def case(name, n, edit, k, flank=8, prep=None, ref_edit=None):
        w = rng.integers(1, 5, size=n + 2 * flank).astype(np.uint8)
        if prep:
            prep(w, flank)
        q = np.asarray(edit(w[flank: flank + n].copy()), dtype=np.uint8)
        if ref_edit:
            ref_edit(w, flank)
        out.append((name, w, q, k))

    case("perfect", 60, lambda q: q, 2)

    def same_behind(n):
        def f(w, flank):                                                 # the base behind the stretch repeats its last one: the changed last
            w[flank + n] = w[flank + n - 1]                              # query symbol matches neither, the column stays a mismatch
        return f
    case("subs_and_last", 96, lambda q: sub(q, list(range(1, 93, 3)) + [95]), 34, ref_edit=same_behind(96))
    case("subs_dense", 140, lambda q: sub(q, list(range(2, 140, 3))), 50)

    def clean_70(w, flank):
        free = sorted(set((1, 2, 3, 4)) - {int(w[flank + 119]), int(w[flank + 190])})    # (the stretch holds neither of the letters next to it, so
        w[flank + 120: flank + 190] = [free[i % 2] for i in range(70)]                   # the deletion stays one op; 120 rows on either side: no
    case("ragged_right", 310, lambda q: np.concatenate([q[:120], q[190:]]), 72, prep=clean_70)  # path that mismatches one side instead is cheaper)

    def run_of_a(w, flank):
        w[flank + 20: flank + 32] = 1
        w[flank + 19], w[flank + 32] = 2, 3
    case("del_in_a_run", 70, lambda q: np.concatenate([q[:24], q[26:]]), 3, prep=run_of_a)

    def long_x_ref(w, flank):
        w[flank + 29: flank + 101] = [3] + [1] * 70 + [4]

    def long_x_query(q):
        q[30:100] = 2
        return q
    case("x_run_70", 130, long_x_query, 72, prep=long_x_ref)
    case("ins_and_subs", 80, lambda q: sub(np.concatenate([q[:30], rng.integers(1, 5, size=3).astype(np.uint8), q[30:]]), [10, 60]), 6)
    return out


def tile_align_jobs(cases, n):
    """(reference pool, query pool, jobs) of n jobs, job i case i mod P; every tile of the period has its own stretch of the pools, so no
    two jobs are equal in (ref_offset, query_offset, n, m, k) and none is folded into another"""
    p = len(cases)
    tiles = n // p + 1
    ref_tile, q_tile = np.concatenate([c[1] for c in cases]), np.concatenate([c[2] for c in cases])
    ro = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])])
    qo = np.concatenate([[0], np.cumsum([len(c[2]) for c in cases])])
    jobs = []
    for i in range(n):
        t, c = divmod(i, p)
        jobs.append((t * len(ref_tile) + int(ro[c]), len(cases[c][1]), t * len(q_tile) + int(qo[c]), len(cases[c][2]), cases[c][3], F.MODE_WITH_CIGAR))
    return np.tile(ref_tile, tiles), np.tile(q_tile, tiles), jobs


# ------------------------------------------------------------------------------------------------ extend cases
def extend_cases():
    """[(name, query rows, reference symbols, direction, keyword arguments of test_extend_gpu.Jobs.add)] in walking order"""
    rng = np.random.default_rng(17)
    rnd = lambda n: rng.integers(1, 5, size=n, dtype=np.uint8)

    def with_subs(t, at):
        q = t.copy()
        for p in at:
            q[p] = 1 + q[p] % 4
        return q
    out = []
    t = rnd(90)
    both = lambda name, q, t, **kw: out.extend([(name + " +", q, t, 1, kw), (name + " -", q, t, -1, kw)])
    both("no error, the rows run out", t[:40], t)                        # stops at d = 0
    t = rnd(260)
    both("runs to its d_max", with_subs(t[:200], [8 * e + 7 for e in range(24)]), t, dm=6)
    t = rnd(200)
    both("stopped by the x-drop", np.concatenate([t[:30], rnd(25), t[55:120]]), t, x=10)
    t = rnd(300)
    both("wide: twenty errors up to the last row", with_subs(t[:260], [12 * e + 11 for e in range(20)]), t)
    t = rnd(120)
    both("the row limit cuts the rows", with_subs(t[:100], [20, 50]), t, row_limit=64)
    out.append(("no rows at all", t[:0], t, 1, {}))
    return out


# ------------------------------------------------------------------------------------------------ the 2^14-block group
SV_BIG = dict(min_length=1, max_distance=2, min_support=1)
SV_BIG_LENGTHS = [200_000]


def sv_big_records(n_signatures):
    """Records with about two thousand qualifying D words each, n_signatures signatures in all, n_signatures >= 4 194 304 + 300. In key
    order: 2048 clusters of 2000 members, 2048 of 40, 2048 of 7, 100 single signatures, one chain cluster that begins 1948 signatures
    in front of element 4 194 304 and ends 200 behind it, then 30 single signatures and pairs up to the end. Returns (distinct records
    as (pos, [words], copies), records, words, read lengths)."""
    w = lambda op, n: (n << 4) | op
    spaced = lambda k, d, gap: [x for _ in range(k) for x in (w(EQ, gap), w(DEL, d))]
    bulk = spaced(2048, 3, 7)                                            # a deletion every ten columns: no two are neighbours
    rest = n_signatures - (2000 + 40 + 7) * 2048
    chain = rest - 100 - 100                                             # a deletion every second column: one chain, one cluster
    assert chain > 64 + 300
    tail = rest - 100 - chain                                            # thirty singles, pairs behind them
    pairs = (tail - 30) // 2
    assert tail == 30 + 2 * pairs
    pair_words = [x for _ in range(pairs) for x in (w(EQ, 9), w(DEL, 1), w(EQ, 1), w(DEL, 1))]
    distinct = [(0, bulk, 2000), (30_000, bulk, 40), (60_000, bulk, 7), (90_000, spaced(100, 1, 9), 1), (100_000, spaced(chain, 1, 1), 1),
                (120_000, spaced(30, 1, 9) + pair_words, 1)]
    pool, rows, read_lengths = [], [], []
    for pos, words, copies in distinct:
        off = len(pool)
        pool += words
        for _ in range(copies):
            rows.append((len(rows), FLAGS[len(rows) % 2], 0, pos, 0, off, len(words), 0))      # (forward and reverse: a deletion is the same on both)
            read_lengths.append(sum(x >> 4 for x in words if x & 15 == EQ))
    return distinct, np.array(rows, dtype=F._REC_DTYPE), np.array(pool, dtype=np.uint32), read_lengths
