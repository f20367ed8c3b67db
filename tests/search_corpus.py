"""A text and named seeds built against the structure of the seeding kernels (K1, flx_search.hip): the 4-bit LDS windows of the text
walk (TxWinAccess, the window fill of fm_search_text_kernel) and the work sharing of the filter walk. TEST INFRASTRUCTURE ONLY.

A case is (name, cls, seed, k, props): the seed's symbols, its allowed errors, and what the construction promises about it (checked on
the CPU oracle by test_search_corpus_host.py, never on the product). One text of about 300 kb in three sequences; every seed has
k <= 3 and at most 200 symbols, so the walk with keys is taken. props["locus"] = (sequence, position, errors): the oracle must report a
group of that many errors with a row at that place. A substitution at a seed's first symbol is reported as an insertion, one position
further right (the walk keeps no substitution at either end of an alignment); one at its last symbol leaves the position alone.

Classes:
  lengths   planted strings with 0..k substitutions, for k = 0..3, at the lengths around the two window sizes of the text walk (64 and 160 symbols)
  shift     one seed at sequence pool offsets 0..7 mod 8 (the seed window starts at the offset rounded down to 4: qshift)
  edges     occurrences at the first and last positions of the text and on either side of a sequence delimiter, exact and with an error
            at the first / the last symbol: the walk reads the symbol beyond the occurrence (the text's padding, a delimiter)
  runs      a unit of 40 and one of 120 symbols, copies with one substitution at p; every copy's own string with one error allowed: the
            forced runs on either side of the other copies' substitutions take every length mod 8, to the right and to the left. Copies with
            two substitutions 7, 8 and 9 symbols apart.
  symbols   a run of N beside an occurrence, an N inside the seed on an N of the text, seeds from the two edges of a homopolymer
  filler    light seeds that give a launch its majority of short or of long seeds, and the heavy launch its five waves
  heavy     seeds of three errors inside tandem arrays and inside a family of 300 symbols with diverged copies (the recipe of the
            repeat-rich reference of test_gpu_parity.py, scaled down): the seeds of the family walk thousands of steps, to a few hundred
            rows on either side of the hard cap of 500; those of the tandem arrays pass every hard cap with their first groups. The
            longest seeds of their launch and so the last the launch queue hands out (flx_seeding.cpp orders a launch by errors,
            then by length)
  cap       seeds whose rows, one per group, are exactly the hard cap, one more, and twice it, for hard caps 60 and 500: copies of a unit
            with three substitutions at places of their own; the oracle counts the rows of every copy, and copies of one row are kept
            until the count is met

Launches (name -> the cases of one call): "short" and "long" hold the first five classes and differ in their filler - in "short" most
seeds have at most 64 symbols (the 64-symbol windows; longer seeds read memory), in "long" most have more (the 160-symbol windows; the
seeds of 161 and 200 symbols read memory); "heavy" holds cap, filler and heavy, all of three errors.
"""
import collections
import functools
import types
import zlib

import numpy as np

import oracle_lib as O

Case = collections.namedtuple("Case", "name cls seed k props")

TEXT_LIMIT = 330_000
LENGTHS = (24, 36, 63, 64, 65, 98, 147, 159, 160, 161, 200)
WIN_SHORT, WIN_LONG = 64, 160          # TX_WIN_MAXLEN of the two text kernels
EDGE_LEN, UNIT_SHORT, UNIT_LONG = 36, 40, 120
CAP_UNIT, LIGHT_LEN, HEAVY_LEN = 40, 44, 60
CAP_HARDS = (60, 500)
CAP_PRE, CAP_SPACER = 2, 10
N_HEAVY_FAMILY, N_HEAVY_TANDEM, N_LIGHT = 52, 12, 1050
HEAVY_STEPS = 2000                     # steps (rank queries for all symbols) of the oracle's walk every heavy seed of the family must take at least
NO_CAP = 2 ** 40
# (hard cap, soft cap) of the sharing tests, erase on, count_first / round_robin
CONFIGS = [(60, 7), (500, 50)]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _rand(rng, n):
    return rng.integers(1, 5, size=n).astype(np.uint8)


def _sub(seq, positions, rng=None):
    """a copy with another of the four letters at each position"""
    c = np.array(seq, dtype=np.uint8)
    for p in positions:
        c[p] = (int(c[p]) - 1 + (int(rng.integers(1, 4)) if rng is not None else 1)) % 4 + 1
    return c


# the parts a seed of k errors is cut into and the part each search of the scheme starts with (the optimum search schemes of the
# reference, search.cpp:328-350): the first part of every search is walked without an error
PARTS = {0: 1, 1: 2, 2: 4, 3: 5}
FIRST_PARTS = {0: (0,), 1: (0, 1), 2: (0, 2, 3), 3: (0, 2, 3, 4)}


def first_parts(length, k):
    """[from, to) of the part each search starts with"""
    P = PARTS[k]
    counts = [length // P + (1 if p < length % P else 0) for p in range(P)]
    starts = np.concatenate([[0], np.cumsum(counts)]).tolist()
    return [(starts[p], starts[p + 1]) for p in FIRST_PARTS[k]]


class _Text:
    def __init__(self, n_refs):
        self.refs = [[] for _ in range(n_refs)]
        self.lens = [0] * n_refs

    def put(self, r, piece):
        """appends to sequence r; the piece's position in it"""
        piece = np.asarray(piece, dtype=np.uint8)
        at = self.lens[r]
        self.refs[r].append(piece)
        self.lens[r] += len(piece)
        return at

    def done(self):
        return [np.concatenate(r) for r in self.refs]


# ------------------------------------------------------------------------------------------------ cap: counts met by asking the oracle
class _CapFamily:
    """copies of a unit with three substitutions each at places of their own, searched with three errors: one group of one row per copy"""

    def __init__(self, name, target):
        self.rng, self.name, self.target = _rng(name), name, target
        self.unit = _rand(self.rng, CAP_UNIT)
        self.keys, self.copies = set(), []

    def add(self):
        while True:
            key = tuple(sorted((int(self.rng.integers(4, 36)), int(self.rng.integers(1, 4))) for _ in range(3)))
            if len({p for p, _ in key}) == 3 and key not in self.keys:
                break
        self.keys.add(key)
        c = self.unit.copy()
        for p, d in key:
            c[p] = (c[p] - 1 + d) % 4 + 1
        self.copies.append(np.concatenate([_rand(self.rng, CAP_PRE), c, _rand(self.rng, CAP_SPACER)]))

    def rows(self, per_copy=False):
        """rows over all groups the oracle finds for the unit in a text that holds only this family (or that number copy by copy)"""
        lead = 200
        idx = O.Index([np.concatenate([_rand(self.rng, lead)] + self.copies)])
        g = idx.search_groups(self.unit, 3, n=NO_CAP)[0]
        if not per_copy:
            return int(g[:, 1].sum())
        each = [0] * len(self.copies)
        for lb, ln, _ in g:
            for row in range(int(lb), int(lb + ln)):
                each[(idx.locate(row)[1] - lead) // len(self.copies[0])] += 1
        return each

    def dial(self):
        """half as many copies again as rows are wanted; the oracle counts every copy's rows (a copy whose substitutions lie side by side is
        found along several paths and counts once for each), and the first `target` copies of one row stay"""
        for _ in range(self.target + self.target // 2 + 8):
            self.add()
        each = self.rows(per_copy=True)
        self.copies = [c for c, n in zip(self.copies, each) if n == 1][: self.target]
        if len(self.copies) != self.target or self.rows() != self.target:
            raise RuntimeError(f"family {self.name}: the oracle's row count does not reach {self.target}")
        return self


def cap_targets():
    """name -> rows of the seed over all groups"""
    out = {}
    for hard in CAP_HARDS:
        out[f"cap_{hard}_at"] = hard
        out[f"cap_{hard}_over"] = hard + 1
        out[f"cap_{hard}_far"] = 2 * hard
    return out


# ------------------------------------------------------------------------------------------------ heavy: the repeat-rich recipe, scaled down
def _heavy_region(rng):
    """(text, the family's consensus, [(from, to)] of the tandem arrays in the text)"""
    family = _rand(rng, 300)
    parts, arrays, total = [], [], 0

    def push(piece):
        nonlocal total
        parts.append(np.asarray(piece, dtype=np.uint8))
        total += len(piece)

    for unit_len in (5, 11, 23, 47):
        push(_rand(rng, 150))
        unit = _rand(rng, unit_len)
        piece = np.tile(unit, 1500 // unit_len + 1)
        arrays.append((total, total + len(piece)))
        push(piece)
    # family copies, 5..30 % diverged (mismatches and small indels). More than in the recipe: with three errors a close copy is found along
    # dozens of paths, and the seeds are to stay near the hard cap of 500 rows, some below it and some above, while their walks stay long
    for _ in range(200):
        c = family.copy()
        for _ in range(int(rng.integers(15, 90))):
            p = int(rng.integers(0, len(c)))
            t = int(rng.integers(0, 3))
            if t == 0:
                c[p] = rng.integers(1, 5)
            elif t == 1:
                c = np.delete(c, p)
            else:
                c = np.insert(c, p, rng.integers(1, 5))
        push(c)
        push(_rand(rng, int(rng.integers(20, 120))))
    return np.concatenate(parts), family, arrays


# ------------------------------------------------------------------------------------------------ the corpus
@functools.lru_cache(maxsize=1)
def build():
    """the corpus, built once and shared"""
    return _build()


def _build():
    """refs: three sequences; cases: every case; pool, seeds [(offset, length, errors, leaf)]: all cases in one pool, seeds[i] of cases[i];
    launches: name -> case indices"""
    T = _Text(3)
    cases, aligned = [], {}

    def case(name, cls, seed, k, align=None, **props):
        cases.append(Case(name, cls, np.asarray(seed, dtype=np.uint8), k, props))
        if align is not None:
            aligned[name] = align

    # ---- edges at the start of the text: the first sequence starts with random symbols
    rng = _rng("edges")
    T.put(0, _rand(rng, 400))
    T.put(1, _rand(rng, 400))                                      # (right behind the first delimiter)

    def edge(name, r, pos, seq):
        case(f"edges_{name}_exact0", "edges", seq, 0, locus=(r, pos, 0))
        case(f"edges_{name}_exact", "edges", seq, 1, locus=(r, pos, 0))
        case(f"edges_{name}_first", "edges", _sub(seq, [0], rng), 1, locus=(r, pos + 1, 1))
        case(f"edges_{name}_last", "edges", _sub(seq, [EDGE_LEN - 1], rng), 1, locus=(r, pos, 1))

    # ---- lengths
    rng = _rng("lengths")
    for ln in LENGTHS:
        for k in range(4):
            for s in range(k + 1):
                planted = _rand(rng, ln)
                T.put(0, _rand(rng, 7))
                pos = T.put(0, planted)
                # substitutions away from the ends and from each other
                where = [int(x) for x in (np.arange(s) * (ln - 8) // max(s, 1) + 4 + rng.integers(0, 3, size=s))]
                case(f"lengths_{ln}_k{k}_s{s}", "lengths", _sub(planted, where, rng), k, locus=(0, pos, s), subs=where)
    # ---- shift: one locus, the seed at every pool offset mod 8
    rng = _rng("shift")
    for ln, k, where in ((36, 1, [17]), (147, 2, [30, 100])):
        planted = _rand(rng, ln)
        T.put(0, _rand(rng, 5))
        pos = T.put(0, planted)
        seq = _sub(planted, where, rng)
        for off in range(8):
            case(f"shift_{ln}_off{off}", "shift", seq, k, align=off, locus=(0, pos, len(where)), pool_offset_mod8=off)
    # ---- runs
    rng = _rng("runs")
    for unit_len, where in ((UNIT_SHORT, list(range(UNIT_SHORT))),
                            (UNIT_LONG, list(range(8)) + list(range(UNIT_LONG // 2 - 4, UNIT_LONG // 2 + 4)) + list(range(UNIT_LONG - 8, UNIT_LONG)))):
        unit = _rand(rng, unit_len)
        for p in where:
            c = _sub(unit, [p], rng)
            T.put(0, _rand(rng, 9))
            pos = T.put(0, c)
            case(f"runs_{unit_len}_p{p}", "runs", c, 1, locus=(0, pos, 0), sub_at=p)
        case(f"runs_{unit_len}_unit", "runs", unit, 1, copies=len(where))          # not in the text: every copy with one error
        if unit_len == UNIT_SHORT:
            for d in (7, 8, 9):
                c = _sub(unit, [10, 10 + d], rng)
                T.put(0, _rand(rng, 9))
                pos = T.put(0, c)
                case(f"runs_{unit_len}_apart{d}", "runs", c, 2, locus=(0, pos, 0), subs=[10, 10 + d])
            case(f"runs_{unit_len}_unit_k2", "runs", unit, 2, copies=len(where) + 3)
    # ---- symbols
    rng = _rng("symbols")
    left, right = _rand(rng, EDGE_LEN), _rand(rng, EDGE_LEN)
    T.put(1, _rand(rng, 11))
    pos_l = T.put(1, left)
    T.put(1, np.full(12, 5, np.uint8))
    pos_r = T.put(1, right)
    case("symbols_left_of_n_run", "symbols", left, 1, locus=(1, pos_l, 0))
    case("symbols_left_of_n_run_last", "symbols", _sub(left, [EDGE_LEN - 1], rng), 1, locus=(1, pos_l, 1))
    case("symbols_right_of_n_run", "symbols", right, 1, locus=(1, pos_r, 0))
    case("symbols_right_of_n_run_first", "symbols", _sub(right, [0], rng), 1, locus=(1, pos_r + 1, 1))
    case("symbols_into_n_run", "symbols", np.concatenate([left[6:], np.full(6, 5, np.uint8)]), 1, locus=(1, pos_l + 6, 0))
    with_n = _rand(rng, UNIT_SHORT)
    with_n[20] = 5
    T.put(1, _rand(rng, 13))
    pos = T.put(1, with_n)
    case("symbols_n_on_n", "symbols", with_n, 1, locus=(1, pos, 0))
    case("symbols_n_on_n_k0", "symbols", with_n, 0, locus=(1, pos, 0))
    case("symbols_n_on_n_sub", "symbols", _sub(with_n, [30], rng), 2, locus=(1, pos, 1))
    before, after = _rand(rng, 30), _rand(rng, 30)
    before[-1], after[0] = 2, 3                                    # (the homopolymer of A ends where it is written to end)
    T.put(1, _rand(rng, 3))
    pos = T.put(1, before)
    T.put(1, np.full(60, 1, np.uint8))
    T.put(1, after)
    case("symbols_into_homopolymer", "symbols", np.concatenate([before[12:], np.full(18, 1, np.uint8)]), 1, locus=(1, pos + 12, 0))
    case("symbols_out_of_homopolymer", "symbols", np.concatenate([np.full(18, 1, np.uint8), after[:18]]), 1, locus=(1, pos + 30 + 42, 0))
    # ---- cap
    for name, target in cap_targets().items():
        f = _CapFamily(name, target).dial()
        T.put(1, _rand(f.rng, 50))
        for c in f.copies:
            T.put(1, c)
        case(name, "cap", f.unit, 3, rows=target)
    # ---- heavy
    rng = _rng("heavy")
    region, family, arrays = _heavy_region(rng)
    T.put(2, _rand(rng, 300))
    T.put(2, region)
    for i in range(N_HEAVY_FAMILY):
        at = int(rng.integers(0, len(family) - HEAVY_LEN))
        case(f"heavy_family_{i}", "heavy", family[at:at + HEAVY_LEN], 3, steps=HEAVY_STEPS)
    for i in range(N_HEAVY_TANDEM):
        a, b = arrays[i % len(arrays)]
        at = int(rng.integers(a, b - HEAVY_LEN))
        case(f"heavy_tandem_{i}", "heavy", _sub(region[at:at + HEAVY_LEN], [int(rng.integers(5, HEAVY_LEN - 5))], rng), 3, rows_over=2 * max(CAP_HARDS))
    # ---- random text behind everything, the three sequences to a third of the text each; the last symbols of the text and the
    #      symbols in front of the two delimiters stay random
    rng = _rng("filler")
    third = (TEXT_LIMIT - 30_000) // 3
    random_from = list(T.lens)
    for r in range(3):
        T.put(r, _rand(rng, max(third - T.lens[r], 400)))
    refs = T.done()
    rng = _rng("edges")
    for p in (0, 1, 3, 4, 5, 7):
        edge(f"start{p}", 0, p, refs[0][p:p + EDGE_LEN])
    for d in (1, 2, 5):                                            # ending at the text's last symbol but d - 1
        p = len(refs[2]) - EDGE_LEN - (d - 1)
        edge(f"end{d}", 2, p, refs[2][p:p + EDGE_LEN])
    edge("behind_delimiter", 1, 0, refs[1][:EDGE_LEN])
    p = len(refs[0]) - EDGE_LEN
    edge("in_front_of_delimiter", 0, p, refs[0][p:])
    edge("in_front_of_delimiter2", 1, len(refs[1]) - EDGE_LEN, refs[1][len(refs[1]) - EDGE_LEN:])
    # ---- filler: substrings of the random text, one substitution in every other one
    def fill(cls_name, n, lens, k, r):
        src = refs[r]
        for i in range(n):
            ln = lens[i % len(lens)]
            at = int(rng.integers(random_from[r] + 10, len(src) - ln - 50))      # (the random end of the sequence)
            seq = src[at:at + ln]
            if i % 2:
                seq = _sub(seq, [int(rng.integers(4, ln - 4))], rng)
            case(f"{cls_name}_{i}", "filler", seq, k, locus=(r, at, i % 2))
    fill("filler_short", 60, (30, 48), 1, 0)
    fill("filler_long", 260, (98, 130, 147), 1, 0)
    fill("filler_light", N_LIGHT, (LIGHT_LEN,), 3, 2)

    names = [c.name for c in cases]
    base = [i for i, c in enumerate(cases) if c.cls in ("lengths", "shift", "edges", "runs", "symbols")]
    pick = lambda prefix: [i for i, n in enumerate(names) if n.startswith(prefix)]
    launches = {
        "short": base + pick("filler_short"),
        "long": base + pick("filler_long"),
        "heavy": [i for i, c in enumerate(cases) if c.cls == "cap"] + pick("filler_light") + [i for i, c in enumerate(cases) if c.cls == "heavy"],
    }
    # ---- the pool: every case's symbols, the shift cases at their offset mod 8
    rng = _rng("pool")
    pool, seeds, at = [], [], 0
    for i, c in enumerate(cases):
        if c.name in aligned:
            pad = (aligned[c.name] - at) % 8
            pool.append(_rand(rng, pad))
            at += pad
        seeds.append((at, len(c.seed), c.k, i))
        pool.append(c.seed)
        at += len(c.seed)
    corpus = types.SimpleNamespace(refs=refs, cases=cases, pool=np.concatenate(pool), seeds=seeds, launches=launches)
    # ---- the searches of a seed that start on a part with exactly one occurrence in the text: the walk is down to one row inside that part
    #      at the latest, with two or more symbols to go, and queues the subtree below for the walk against the text (fm_step: nlen == 1,
    #      len - x >= 2, no delimiter in the seed). Asked of the oracle per part; a seed without errors is one part, taken without its last two symbols.
    idx = O.Index(refs)
    for i in launches["short"] + launches["long"]:
        c = cases[i]
        if "one_row_starts" in c.props:
            continue
        n = 0
        if not np.any(c.seed == 0):
            for a, b in first_parts(len(c.seed), c.k):
                g = idx.search_groups(c.seed[a:b - 2] if c.k == 0 else c.seed[a:b], 0, n=NO_CAP)[0]
                n += len(g) == 1 and int(g[0, 1]) == 1
        c.props["one_row_starts"] = n
    corpus.index = idx
    return corpus


def oracle_index():
    return build().index


def launch_seeds(launch):
    """(pool, seeds [(offset, length, errors, leaf)]) of a launch, the leaf the seed's place in the launch"""
    c = build()
    return c.pool, [(c.seeds[i][0], c.seeds[i][1], c.seeds[i][2], at) for at, i in enumerate(c.launches[launch])]


def is_long_launch(launch):
    """restated from flx_seeding.cpp, not imported: the larger windows when more than half of the seeds have more than 64 symbols"""
    c = build()
    lens = [len(c.cases[i].seed) for i in c.launches[launch]]
    return 2 * sum(ln > WIN_SHORT for ln in lens) > len(lens)


@functools.lru_cache(maxsize=None)
def groups(launch):
    """the oracle's groups (lb, len, errors) and walk counters of every seed of a launch, without a cap"""
    pool, seeds = launch_seeds(launch)
    return [oracle_index().search_groups(pool[off:off + ln], k, n=NO_CAP) for off, ln, k, _ in seeds]


@functools.lru_cache(maxsize=None)
def expected(launch, hard, soft):
    """the oracle's (anchors, stats) of a launch: count_first, round_robin, erase on. Computed once and shared: do not change them."""
    pool, seeds = launch_seeds(launch)
    return oracle_index().search_seeds(pool, seeds, hard=hard, soft=soft, order=1, choice=0, erase=True)
