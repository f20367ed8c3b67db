"""Named alignment cases built against the structure of the DP and traceback kernels (K3/K4/K5, flx_device.hip). TEST INFRASTRUCTURE ONLY.

A case is (name, cls, ref, query, k, props): one reference window, one query, the allowed errors, and what the construction promises about
the alignment (checked on the CPU oracle's matrix DP by test_align_corpus_host.py, never on the product). The corpus is built for a launch
shape (W words per lane, R lanes per job): the query rows sit on the shape's boundaries - 64WRt - 1, 64WRt, 64WRt + 1 (t revolutions of the
ring: the last word group ends a revolution, or is the only one of the next) and 64W(Rt + 1) + 17 - and the reference slack is chosen so
that a job of more than R word groups really waits in that shape (ring_delay > 0) while the shape still holds it (delay + 1 <= 128 hand-over
slots). One DP matrix stays at or below 2 * 10^7 cells.

Classes:
  gap       one planted run of deletions (D: reference columns without a row) or insertions (I: rows without a column) in otherwise exact
            sequence. The run's letters are 4, everything else is drawn from 1..3: a row can never match a column of the run, so no other
            path is cheaper than the run itself. Also two runs 100 rows apart, and a run plus 5 % substitutions.
  band      the optimal path on the band's extreme diagonals -k and n - m + k.
  ties      homopolymers, tandem repeats with a unit removed or added, two-letter sequences: many equally good paths.
  runs      2 NM + 1 CIGAR runs with k = NM: the CIGAR slab of 2 NM + 2 words is used to its last but one word.
  thresholds  k = 0, k = m, k = 2m, n = 0, and for every case with an alignment its twin with k = NM - 1, which has none.
"""
import collections
import functools
import re
import zlib

import numpy as np

import oracle_lib as O

Case = collections.namedtuple("Case", "name cls ref query k props")

MAX_CELLS = 2 * 10 ** 7
RING_QUEUE_MAX = 128
WORDS_PER_LANE = (1, 2, 3, 4, 5, 6, 8, 13, 25)
# one shape per W for the forced-shape tests: two lanes (a hand-over between two lanes and through the queue). (25, 2) is the one shape that
# holds a 1100-column deletion run in a ring that waits: k = L + 2 makes its band 3L + 4 diagonals wide, and a ring waits at most 127 blocks
# beyond its 64W(R - 1) rows
SHAPES = ((1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (6, 2), (8, 2), (13, 2), (25, 2))

D_RUNS = (1, 15, 16, 17, 48, 128, 129, 400, 700, 1100)
I_RUNS = (1, 47, 48, 49, 64, 65, 511, 512, 513, 700)


# ------------------------------------------------------------------------------------------------ the ring schedule (flx_internal.hpp)
def ring_group_blocks(n, m, k, W, Lg, pad, g):
    band_hi = n - m + k
    r0, r1 = max(64 * W * g - pad, 0), 64 * W * (g + 1) - pad
    b_lo = max(r0 - k, 0) >> 4
    b_hi = min(r1 - 1 + band_hi, n - 1) >> 4
    if g + 1 < Lg:
        b_hi = max(b_hi, max(r1 - k, 0) >> 4)
    return b_lo, b_hi


def groups_of(m, W):
    return ((m + 63) // 64 + W - 1) // W


def ring_delay(n, m, k, W, R):
    if n == 0 or m == 0 or n + k < m:
        return 0
    Lg = groups_of(m, W)
    pad = Lg * 64 * W - m
    delay = 0
    for g in range(0, Lg - R):
        _, hi0 = ring_group_blocks(n, m, k, W, Lg, pad, g)
        lo1, _ = ring_group_blocks(n, m, k, W, Lg, pad, g + R)
        delay = max(delay, hi0 - lo1 + 1 - R)
    return delay


def never_waits(n, m, k, W, R):
    """what the host asks of a shape whose ring is not to wait (choose_align_shape)"""
    return groups_of(m, W) <= R or 64 * W * (R - 1) + R + 1 > n - m + 2 * k


def shape_holds(n, m, k, W, R):
    return never_waits(n, m, k, W, R) or ring_delay(n, m, k, W, R) + 1 <= RING_QUEUE_MAX


# ------------------------------------------------------------------------------------------------ helpers
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _rand(rng, n, letters=(1, 2, 3)):
    return rng.choice(np.array(letters, dtype=np.uint8), size=max(int(n), 0)).astype(np.uint8)


def _cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts]).astype(np.uint8)


def rows_for(W, R, need=0):
    """the shape's boundary sizes, in the first revolution count t that leaves `need` rows"""
    t = max(1, -(-(need + 1) // (64 * W * R)))
    return [64 * W * R * t - 1, 64 * W * R * t, 64 * W * R * t + 1, 64 * W * (R * t + 1) + 17]


def boundary_row(m, W, group, lo, hi):
    """the first row of a 64-row word (of a 64W-row word group) in [lo, hi] nearest the middle of the query; rows are right-aligned in their
    groups"""
    unit = 64 * W if group else 64
    pad = groups_of(m, W) * 64 * W - m
    rows = [unit * j - pad for j in range(1, (m + pad) // unit + 1) if lo <= unit * j - pad <= hi]
    if not rows:
        return None
    return min(rows, key=lambda r: abs(r - m // 2))


def _slack(W, R, m, cols, k):
    """reference slack (beyond `cols` columns) with which a job of more than R groups waits in the shape (W, R), a few columns otherwise, less
    where the cell cap asks for it"""
    slack = 8
    if groups_of(m, W) > R:
        width = cols + slack - m + 2 * k
        need = 64 * W * (R - 1) + R + 1 + 72          # (blocks past the point where the ring may start to wait: the twin's narrower band waits as well)
        slack += max(0, need - width)
    while slack > 0 and (m + 1) * (cols + slack + 1) > MAX_CELLS:
        slack -= 1
    return slack


class _Builder:
    def __init__(self, W, R, forced):
        self.W, self.R, self.forced = W, R, forced
        self.cases, self.names, self.dropped = [], set(), []
        self._size = 0

    def next_rows(self, need=0, odd=False):
        """the shape's sizes in turn, so that every kind of size meets every class"""
        for _ in range(4):
            m = rows_for(self.W, self.R, need)[self._size % 4]
            self._size += 1
            if (m + 1) * (m + 65) > MAX_CELLS:
                m = rows_for(self.W, self.R, need)[2]       # (the largest size is beyond the cell cap: 64WRt + 1 has a group more than 64WRt as well)
            if (not odd or m % 2) and (m + 1) * (m + 65) <= MAX_CELLS:
                return m
        return None                                 # (no size of that revolution fits the cell cap)

    def add(self, name, cls, ref, query, k, **props):
        ref, query = np.ascontiguousarray(ref, dtype=np.uint8), np.ascontiguousarray(query, dtype=np.uint8)
        n, m = len(ref), len(query)
        assert name not in self.names, name
        assert m >= 1 and (m + 1) * (n + 1) <= MAX_CELLS, (name, m, n)
        if self.forced and not shape_holds(n, m, k, self.W, self.R):
            self.dropped.append(name)
            return None
        self.names.add(name)
        c = Case(name, cls, ref, query, int(k), props)
        self.cases.append(c)
        return c


# ------------------------------------------------------------------------------------------------ gap runs
def _gap(B, tag, kind, L, place, subs=0.0):
    W, R = B.W, B.R
    name = f"gap_{kind}{L}_{place}{tag}"
    rng = _rng(f"{name}_{W}_{R}")
    # rows: both flanks must cost more to move than the run does (a flank of f rows against the run's letters costs f)
    # (every other four cases in the ring's second revolution: all four sizes then have more groups than lanes)
    m = B.next_rows(need=max(2 * L + 8 + (L if kind == "I" else 0), 64 * W * R + 1 if B._size % 8 >= 4 and (128 * W * R + 1) * (128 * W * R + 65) <= MAX_CELLS else 0))
    if kind == "D" and 3 * L + 4 > 64 * W * (R - 1) + 16 * 100 and groups_of(rows_for(W, R, 2 * L + 8)[2], W) == R + 1:
        m = rows_for(W, R, 2 * L + 8)[2]            # (a run that only a wide shape's ring can wait for: the size that has R + 1 groups)
    if m is None:
        B.dropped.append(name)
        return
    body = m - (L if kind == "I" else 0)            # rows that have a column
    # pos: rows in front of the run. A deletion run keeps more rows than its own length on either side (nearer an end it is absorbed by the
    # free end); an insertion run's rows straddle the boundary, a deletion run sits between the boundary's two rows.
    if place in ("word", "group"):
        lo, hi = (L + 1, m - L - 1) if kind == "D" else ((L + 1) // 2 + 1, m - L // 2 - 1)
        r = boundary_row(m, W, place == "group", lo, hi) or boundary_row(m, W, False, lo, hi) or m // 2
        pos = r if kind == "D" else r - (L + 1) // 2
    else:
        pos = {"first": L + 1 if kind == "D" else 1, "last": body - L - 1 if kind == "D" else body - 1}.get(place, body // 2 + 3)
    b = _rand(rng, body)
    run = np.full(L, 4, dtype=np.uint8)
    if kind == "D":
        query, core = b, _cat(b[:pos], run, b[pos:])
    else:
        query, core = _cat(b[:pos], run, b[pos:]), b
    k = L + 2
    if subs:
        rows = [r for r in rng.choice(m, size=max(1, int(subs * m)), replace=False) if query[r] != 4]
        query = query.copy()
        for r in rows:
            query[r] = query[r] % 3 + 1
        k += len(rows)
    slack = _slack(W, R, m, len(core), k)
    left = 0 if (kind == "I" and place == "first") else min(slack, 8)
    if place == "colbegin":
        left += (-(left + pos)) % 16
    elif place == "colend":
        left += (-(left + pos + L)) % 16
    right = 0 if (kind == "I" and place == "last") else max(slack - left, 0)
    ref = _cat(_rand(rng, left), core, _rand(rng, right))
    if (m + 1) * (len(ref) + 1) > MAX_CELLS:
        B.dropped.append(name)
        return
    B.add(name, "gap", ref, query, k, planted=(kind, L), substitutions=bool(subs))


def _two_runs(B, first, second, L1, L2):
    W, R = B.W, B.R
    name = f"gap_{first}{L1}_then_{second}{L2}"
    rng = _rng(f"{name}_{W}_{R}")
    m = B.next_rows(need=2 * (L1 + L2) + 200)
    if m is None:
        B.dropped.append(name)
        return
    n_ins = L1 if first == "I" else L2
    body = m - n_ins
    b = _rand(rng, body)
    p1 = body // 2 - 50
    p2 = p1 + 100
    four = lambda L: np.full(L, 4, dtype=np.uint8)
    if first == "I":
        query, core = _cat(b[:p1], four(L1), b[p1:]), _cat(b[:p2], four(L2), b[p2:])
    else:
        query, core = _cat(b[:p2], four(L2), b[p2:]), _cat(b[:p1], four(L1), b[p1:])
    k = L1 + L2 + 2
    slack = _slack(W, R, m, len(core), k)
    ref = _cat(_rand(rng, min(slack, 8)), core, _rand(rng, max(slack - 8, 0)))
    B.add(name, "gap", ref, query, k, planted=("I", n_ins), planted2=("D", L1 + L2 - n_ins), substitutions=False)


D_PLACES = ("first", "last", "word", "group", "colbegin", "colend")
I_PLACES = ("first", "last", "word", "group", "colbegin")


def _places(B, places, i):
    """every placement for one and two words per lane; wider shapes (a matrix there has millions of cells, and a test is to take seconds) give
    every run length two placements (W >= 13: one), in turn, so that every length and every placement is present in every corpus"""
    if B.W <= 2:
        return places
    per = 1 if B.W >= 13 else 2
    return tuple(places[(i * per + j) % len(places)] for j in range(per))


def _gap_cases(B):
    for i, L in enumerate(D_RUNS):
        for place in _places(B, D_PLACES, i):
            _gap(B, "", "D", L, place)
    for i, L in enumerate(I_RUNS):
        for place in _places(B, I_PLACES, i):
            _gap(B, "", "I", L, place)
    _two_runs(B, "I", "D", 49, 17)
    _two_runs(B, "D", "I", 17, 49)
    _gap(B, "_subs", "D", 48, "group", subs=0.05)
    _gap(B, "_subs", "I", 65, "word", subs=0.05)


# ------------------------------------------------------------------------------------------------ band edges
def _band_cases(B):
    W, R = B.W, B.R
    for k in (1, 16, 17, 64 * W, 64 * W + 1):
        for left, right in ((0, 0), (0, 1), (1, 0), (1, 1)):
            # (three and more words per lane: unequal slacks for k = 17 only; W >= 13: slack for k = 17 only - seconds per test)
            if (W >= 3 and left != right and k != 17) or (W >= 13 and (left or right) and k != 17):
                continue
            for kind in ("lead_ins", "trail_ins", "dels"):
                name = f"band_{kind}_k{k}_l{left}r{right}"
                rng = _rng(f"{name}_{W}_{R}")
                m = B.next_rows(need=2 * k + 16)
                if m is None:
                    B.dropped.append(name)
                    continue
                four = np.full(k, 4, dtype=np.uint8)
                if kind == "lead_ins":            # k insertions at column 0: n + k == m, the path runs down diagonal -k
                    body = _rand(rng, m - k)
                    query, core = _cat(four, body), body
                elif kind == "trail_ins":         # k insertions at column n: the path starts on diagonal n - m + k
                    body = _rand(rng, m - k)
                    query, core = _cat(body, four), body
                else:                             # n == m + k and exactly k deletions, one every few rows
                    query = _rand(rng, m)
                    step = max(2, (m - 2) // (k + 1))
                    cuts = [1 + step * (i + 1) for i in range(k)]
                    cuts = [min(c, m - 1) for c in cuts]
                    parts, last = [], 0
                    for c in cuts:
                        parts += [query[last:c], [4]]
                        last = c
                    core = _cat(*parts, query[last:])
                ref = _cat(_rand(rng, left), core, _rand(rng, right))
                if (m + 1) * (len(ref) + 1) > MAX_CELLS:
                    B.dropped.append(name)
                    continue
                forced_ends = left == 0 and right == 0
                # (without slack NM == k forces k insertions / k deletions and both ends; with a column of slack other paths may be as cheap,
                # but NM <= k leaves the path no more than the slack away from either end: ends_within)
                props = dict(begin0=kind != "trail_ins", end_n=kind != "lead_ins", planted=("I", k) if kind != "dels" else ("D", 1)) if forced_ends else {}
                B.add(name, "band", ref, query, k, ends_within=left + right, **props)


# ------------------------------------------------------------------------------------------------ ties
def _tie_cases(B):
    W, R = B.W, B.R
    need = 64 * W * R + 1                           # more than one revolution: every tie case has more groups than lanes
    beyond_cap = (2 * need + 1) * (2 * need + 65) > MAX_CELLS      # (W = 25: the second revolution does not fit; 64WR + 1 rows have R + 1 groups)
    wide = W >= 13
    for letter in (1,) if wide else (1, 3):
        name = f"ties_homopolymer_in_longer_{letter}"
        m = need if beyond_cap else B.next_rows(need)
        k = 3
        n = m + _slack(W, R, m, m, k)
        B.add(name, "ties", np.full(n, letter), np.full(m, letter), k)
    for d in (5,) if wide else (1, 5):
        name = f"ties_homopolymer_shorter_run_{d}"
        rng = _rng(f"{name}_{W}_{R}")
        m = need if beyond_cap else B.next_rows(need)
        k = d + 2
        slack = _slack(W, R, m, m - d, k)
        ref = _cat(_rand(rng, slack // 2 + d, (2, 3)), np.full(m - d, 1), _rand(rng, slack - slack // 2 + d, (2, 3)))
        B.add(name, "ties", ref, np.full(m, 1), k)
    for period, unit_letters in ((2, (1, 2)), (7, None)):
        for change in ((-1,) if period == 2 else (1,)) if wide else (-1, 1):
            name = f"ties_tandem_p{period}_{'removed' if change < 0 else 'added'}"
            rng = _rng(f"{name}_{W}_{R}")
            m = need if beyond_cap else B.next_rows(need)
            unit = np.array(unit_letters, dtype=np.uint8) if unit_letters else np.array([1, 2, 2, 3, 1, 3, 2], dtype=np.uint8)
            flank = 40
            copies_q = (m - 2 * flank) // period
            f1, f2 = _rand(rng, flank, (3, 4) if period == 2 else (4,)), _rand(rng, m - flank - copies_q * period, (3, 4) if period == 2 else (4,))
            query = _cat(f1, np.tile(unit, copies_q), f2)
            core = _cat(f1, np.tile(unit, copies_q - change), f2)      # the query has one unit fewer / more than the reference
            k = period + 2
            slack = _slack(W, R, m, len(core), k)
            ref = _cat(_rand(rng, slack // 2, (3, 4) if period == 2 else (4,)), core, _rand(rng, slack - slack // 2, (3, 4) if period == 2 else (4,)))
            B.add(name, "ties", ref, query, k)
    for rep in range(1 if wide else 2):
        name = f"ties_two_letters_{rep}"
        rng = _rng(f"{name}_{W}_{R}")
        m = need if beyond_cap else B.next_rows(need)
        query = _rand(rng, m, (1, 2))
        core, edits = [], 0
        for c in query:
            r = rng.random()
            if r < 0.03:
                edits += 1                          # the row has no column
                continue
            if r < 0.06:
                core.append(int(rng.integers(1, 3)))
                edits += 1                          # a column without a row
            core.append(3 - int(c) if r >= 0.06 and r < 0.10 else int(c))
            edits += 1 if r >= 0.06 and r < 0.10 else 0
        slack = _slack(W, R, m, len(core), edits)
        ref = _cat(_rand(rng, slack // 2, (1, 2)), core, _rand(rng, slack - slack // 2, (1, 2)))
        B.add(name, "ties", ref, query, edits)


# ------------------------------------------------------------------------------------------------ run count
def _run_cases(B):
    W, R = B.W, B.R
    for form, every in (("dense", 2), ("sparse", 5)):
        for rep in range(2 if form == "dense" else 1):
            name = f"runs_{form}_{rep}"
            rng = _rng(f"{name}_{W}_{R}")
            m = B.next_rows(need=201, odd=True)
            core = _rand(rng, m, (1, 2, 3, 4))
            query = core.copy()
            rows = list(range(1, m - 1, every))     # isolated, none at either end: '=' X '=' ... X '='
            query[rows] = 5                         # N in the query only: a substitution wherever it is aligned
            k = len(rows)
            slack = _slack(W, R, m, m, k) if rep == 0 else 0
            ref = _cat(_rand(rng, slack // 2, (1, 2, 3, 4)), core, _rand(rng, slack - slack // 2, (1, 2, 3, 4)))
            B.add(name, "runs", ref, query, k, runs=2 * k + 1)


# ------------------------------------------------------------------------------------------------ thresholds
def _threshold_cases(B):
    W, R = B.W, B.R
    sizes = (rows_for(W, R)[1:3] if W >= 13 else rows_for(W, R)) + ([1, 63, 64, 65] if W == 1 else [])
    for m in sizes:
        rng = _rng(f"thr_{m}_{W}_{R}")
        q = _rand(rng, m, (1, 2, 3, 4))
        B.add(f"thr_exact_k0_m{m}", "thresholds", q, q, 0)
        slack = _slack(W, R, m, m, 0)
        B.add(f"thr_exact_k0_slack_m{m}", "thresholds", _cat(_rand(rng, slack // 2, (1, 2, 3, 4)), q, _rand(rng, slack - slack // 2, (1, 2, 3, 4))), q, 0)
        B.add(f"thr_n0_m{m}", "thresholds", np.zeros(0, np.uint8), q, m)                       # no column: m insertions
        if m <= 65 * max(W, 2) or not B.forced:
            noisy = q.copy()
            noisy[::7] = noisy[::7] % 4 + 1
            ref = _cat(_rand(rng, 5, (1, 2, 3, 4)), noisy, _rand(rng, 5, (1, 2, 3, 4)))
            for mult in (1, 2):
                if (m + 1) * (len(ref) + 1) <= MAX_CELLS and m * mult <= 3000:
                    B.add(f"thr_k{mult}m_m{m}", "thresholds", ref, q, mult * m)


@functools.lru_cache(maxsize=None)
def score(ref_bytes, query_bytes, k):
    """NM of a case at its k by the oracle's matrix DP, None if there is no alignment (cached per case)"""
    res = O.align(np.frombuffer(ref_bytes, np.uint8), np.frombuffer(query_bytes, np.uint8), k, mode=0, algo=0)
    return None if res is None else int(res[0])


def nm_of(case):
    return score(case.ref.tobytes(), case.query.tobytes(), case.k)


def _twins(B):
    """for every case with an alignment the same pair with k = NM - 1: no alignment (n + k == m - 1 among them: the twins of the leading
    insertions and of n == 0)"""
    for c in list(B.cases):
        nm = nm_of(c)
        assert nm is not None, f"{c.name}: the construction has no alignment within k = {c.k}"
        if nm == 0:
            continue
        B.add(f"twin_{c.name}", "thresholds", c.ref, c.query, nm - 1, twin_of=c.name)


@functools.lru_cache(maxsize=None)
def _built(W, R, forced):
    B = _Builder(W, R, forced)
    _gap_cases(B)
    _band_cases(B)
    _tie_cases(B)
    _run_cases(B)
    _threshold_cases(B)
    _twins(B)
    return tuple(B.cases), tuple(B.dropped)


def corpus(W, R, forced=True):
    """the cases for shape (W, R); forced: only those the shape holds (FLX_FORCE_SHAPE falls back to the default shape for the others)"""
    return _built(W, R, forced)[0]


def dropped(W, R, forced=True):
    """names of the cases left out of corpus(W, R): the forced shape does not hold them, or no size of the shape fits the cell cap"""
    return _built(W, R, forced)[1]


def whole():
    """the corpus of the default-shape tests: everything built for one and for two words per lane, the cases no forced shape holds included"""
    out = []
    for W, R in ((1, 2), (2, 2)):
        out += [c._replace(name=f"w{W}_{c.name}", props=dict(c.props, **({"twin_of": f"w{W}_{c.props['twin_of']}"} if "twin_of" in c.props else {})))
                for c in corpus(W, R, forced=False)]
    return tuple(out)


# ------------------------------------------------------------------------------------------------ expectations and batches
@functools.lru_cache(maxsize=None)
def _expected(ref_bytes, query_bytes, k, mode, algo):
    return O.align(np.frombuffer(ref_bytes, np.uint8), np.frombuffer(query_bytes, np.uint8), k, mode=mode, algo=algo)


def expected(case, mode, algo=0):
    """the oracle's answer (algo 0: the matrix DP that defines the semantics) in align_batch's form for the mode"""
    exp = _expected(case.ref.tobytes(), case.query.tobytes(), case.k, mode, algo)
    if exp is None:
        return None
    if mode == 0:
        return (exp[0], 0, "")
    if mode == 1:
        return (exp[0], exp[1], "")
    return exp


def batch(cases, modes=(0, 1, 2), tail=0):
    """(reference pool, query pool, jobs, (case, mode) per job): every case once in the pools, one job per mode; `tail` symbols after the
    last reference window (0: it ends at the pool's last byte)"""
    refs, queries, jobs, what = [], [], [], []
    ro = qo = 0
    for c in cases:
        for mode in modes:
            jobs.append((ro, len(c.ref), qo, len(c.query), c.k, mode))
            what.append((c, mode))
        refs.append(c.ref)
        queries.append(c.query)
        ro += len(c.ref)
        qo += len(c.query)
    refs.append(np.full(tail, 1, dtype=np.uint8))
    return _cat(*refs), _cat(*queries), jobs, what


def cigar_runs(cigar):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", cigar)]
