"""A text, named seeds and reads built against the bookkeeping of the ordered FM-index walk (K1', fm_search_ordered_kernel of
flx_search_ordered.hip): its seed queue, its hit-slot ranges, the cap on a seed's rows, its frame stack and the seed lengths that turn a
launch to it by themselves. TEST INFRASTRUCTURE ONLY.

A case is (name, cls, seed, k, props) as in search_corpus.py: the seed's symbols, its allowed errors, and what the construction promises
about it (checked on the CPU oracle by test_ordered_corpus_host.py, never on the product). A launch is (name, cls, text, members, caps):
the cases of one call, the text they are searched in ("own": the text built here, about 170 kb in two sequences; "search": the text of
search_corpus.py, whose cases and cached expectations are used as they are) and the row caps (max_hits) of its raw-emission runs.
ABSENT, one 8-mer, occurs nowhere in the own text: every random piece is drawn again until it and its junction are free of it.

Classes:
  queue    launches of n exact seeds of one occurrence (k = 0, 24..40 symbols) for n on either side of the 64 seeds a wave grabs at a time
           and of the 256 seeds per wave of a launch (one, two and three waves; the wave count follows from the seed count alone);
           queue_mixed: about 200 seeds of every length 24..40 with a few k = 2 seeds among them, so that lanes go idle a few at a time and
           one assignment serves some from the old range and some from a new grab; queue_tail_1 / queue_tail_63: a last grab of 1 / 63 seeds
  slots    single-wave launches whose hits (groups) over all seeds are exactly 1, 63, 64, 65, 127, 128, 129: k = 1 seeds of several groups
           each, topped up with k = 0 seeds of one; slots_ballot: 40 copies of one k = 1 seed in front of 40 copies of one k = 0 seed - the
           copies walk in lockstep, every group of the k = 1 seed is a ballot of 40 hits, and the second finds 24 slots left in the range of
           64; slots_heavy (text "search"): the heavy seeds of search_corpus.py, some with more than 255 groups and the tandem ones with
           more than 1000, so that a hit's ordinal does not fit the byte below it
  cap      units of which the text holds R exact copies (random spacers between them), so that the first group of the unit's search has R
           rows: R = 2, 7, 64 with one error, searched with caps R - 1, R, R + 1 and 1; R = 7 with three errors. Every family also has one
           copy with a substitution in the part that the scheme's first search walks without errors: only a later search finds it, and a
           cap that the first search meets loses it (props["variant"])
  tiny     the prefixes of 1..12 symbols of one string with 0..3 errors each (all four letters follow every proper prefix of it in the text;
           a seed with fewer symbols than its scheme has parts has no search at all), 12 and 20 symbols of a homopolymer inside a run of
           200 (deletion children stack frames without advancing in the seed), seeds with N and with rank 0 (a read's '$' on a sequence
           delimiter), seeds that begin with ABSENT (the k-mer table ends their first search at once)
  length   prefixes of 16383, 16384 and 16999 symbols of one locus with k = 0..3 errors and s = 0..k substitutions. A seed longer than 16383
           symbols turns its launch to the ordered walk. What the walk costs is set by the errors the seed leaves unused: with one spare
           error every node it passes branches (4.7 cursor extensions per symbol measured on the oracle: 76 668 for k = 1, s = 0 at 16383
           symbols, nothing to place), with two spare errors an insertion and a deletion a few symbols apart re-synchronise and each such
           pair walks on to the seed's end (46 M extensions for k = 2, s = 0 without a cap, 2.3 M under the default cap of 501 rows). So:
           the seeds with s == k have their substitutions where the budget opens (see _long_subs) and stay below EXT_LIMIT = 60 000
           extensions of the oracle under every cap; they form the launches "length" (all three lengths) and "length_keyed" (16383 only:
           the walk with keys still takes it). The seeds with s < k cannot meet that limit under a cap above 1 wherever their substitutions
           are; they form "length_spare", searched with a cap of one row only (first_reported with a soft cap of 1, the raw hook with
           max_hits 1), where the first hit ends the walk after one pass over the seed. The limit holds for every long seed under
           every cap it is searched with, and the host test asserts it.
  reads    (reads(): a genome of its own, about 200 kb) two reads of 33 000..35 000 symbols, one of them reverse complemented, for
           query_errors = 5 and seed_errors = 2: two leaves of about 17 000 symbols, each with two substitutions where its budget opens;
           beside them six reads of 1.2 kb
"""
import collections
import functools
import types
import zlib

import numpy as np

import oracle_lib as O
import search_corpus as SC

Case = collections.namedtuple("Case", "name cls seed k props")
Launch = collections.namedtuple("Launch", "name cls text members caps")

NO_CAP = 2 ** 31                                                   # (the raw hook's largest; no seed here has that many rows)
CAPS = (1, 50, 501, NO_CAP)
ABSENT = np.array([1, 2, 3, 4, 4, 3, 2, 1], dtype=np.uint8)
GRAB, SEEDS_PER_WAVE, HIT_GRAB = 64, 256, 64                       # FM_GRAB, FM_SEEDS_PER_WAVE, FM_HIT_GRAB of flx_search_ordered.hip
QUEUE_COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
QUEUE_TAILS = {"queue_tail_1": 193, "queue_tail_63": 191}
SLOT_TOTALS = (1, 63, 64, 65, 127, 128, 129)
BALLOT = 40
CAP_FAMILIES = (("cap_r2_k1", 2, 1), ("cap_r7_k1", 7, 1), ("cap_r64_k1", 64, 1), ("cap_r7_k3", 7, 3))      # (name, R, k)
CAP_UNIT = 40
TINY_MAX = 12
KEYED_MAX = 0x3FFF                                                 # fm_search_max_keyed_length()
LONG_LENGTHS = (KEYED_MAX, KEYED_MAX + 1, 16999)
EXT_LIMIT = 60_000
READ_PARAMS = dict(query_errors=5, seed_errors=2)
# (hard cap, soft cap) of the device selection behind the ordered walk: those of search_corpus.py and one with tiny caps
CONFIGS = SC.CONFIGS + [(5, 3)]
# every launch, by name (known without building the corpus: tests are parametrised over them); a launch's class is its name's first word
LAUNCHES = tuple([f"queue_{n}" for n in QUEUE_COUNTS] + list(QUEUE_TAILS) + ["queue_mixed"] + [f"slots_{t}" for t in SLOT_TOTALS] +
                 ["slots_ballot", "slots_heavy", "cap", "tiny", "length", "length_keyed", "length_spare"])


def _rng(name):
    return np.random.default_rng(zlib.crc32(("ordered_" + name).encode()))


def _has(seq, word):
    n = len(word)
    if len(seq) < n:
        return False
    hit = np.ones(len(seq) - n + 1, dtype=bool)
    for j in range(n):
        hit &= seq[j:len(seq) - n + 1 + j] == word[j]
    return bool(hit.any())


def _rand(rng, n):
    """random letters without ABSENT"""
    while True:
        s = rng.integers(1, 5, size=n).astype(np.uint8)
        if not _has(s, ABSENT):
            return s


_sub = SC._sub
revcomp = lambda r: (5 - np.asarray(r, dtype=np.uint8)[::-1]).astype(np.uint8)          # A C G T = 1 2 3 4


class _Text:
    """sequences grown piece by piece; no junction ever holds ABSENT"""

    def __init__(self, n_refs, rng):
        self.refs = [np.zeros(0, np.uint8) for _ in range(n_refs)]
        self.rng = rng

    def plant(self, r, piece, gap=9):
        """`gap` random symbols and the piece behind them; the piece's position in sequence r"""
        piece = np.asarray(piece, dtype=np.uint8)
        tail = self.refs[r][-7:]
        while True:
            g = _rand(self.rng, gap)
            if not _has(np.concatenate([tail, g, piece[:7]]), ABSENT):
                break
        at = len(self.refs[r]) + gap
        self.refs[r] = np.concatenate([self.refs[r], g, piece])
        return at

    def free(self, r, n):
        self.plant(r, np.zeros(0, np.uint8), gap=n)


def long_parts(length, k):
    """[from, to) of the parts the scheme of k errors cuts a seed into"""
    P = SC.PARTS[k]
    counts = [length // P + (1 if p < length % P else 0) for p in range(P)]
    starts = np.concatenate([[0], np.cumsum(counts)]).tolist()
    return [(starts[p], starts[p + 1]) for p in range(P)]


def _long_subs(length, k):
    """where k substitutions leave no search of the optimum scheme a spare error over a long stretch: every search but one dies in the
    part it walks without errors or right behind it, and that one meets each substitution at the first symbol at which its upper
    bound rises.
      k = 1: searches (0 1), (1 0): the first symbol of part 1 - the first search takes it as its first symbol with a budget, the second dies on it
      k = 2: searches (0 1 2 3), (2 1 0 3), (3 2 1 0): the last symbol of part 1 and the first of part 3 - the second search meets them where
             its bounds 0 1 1 2 rise; the first dies at the end of its exact parts 0 1, the third on its first symbol
      k = 3: searches (0 1 2 3 4), (2 1 0 3 4), (3 2 1 0 4), (4 3 2 1 0): the last symbol of part 1, the first of part 3 and of part 4 - the second
             search (bounds 0 1 1 2 3); the first dies at the end of part 1, the third and fourth on their first symbol"""
    parts = long_parts(length, k)
    if k == 0:
        return []
    if k == 1:
        return [parts[1][0]]
    return [parts[1][1] - 1, parts[3][0]] + ([parts[4][0]] if k == 3 else [])


def _cap_variant_at(k):
    """a place in the part(s) the first search of the scheme walks without an error (part 0; parts 0 and 1 for two and three errors)"""
    return long_parts(CAP_UNIT, k)[0][1] - 3


@functools.lru_cache(maxsize=1)
def build():
    """the corpus, built once and shared"""
    return _build()


def _build():
    rng = _rng("text")
    T = _Text(2, rng)
    cases = []

    def case(name, cls, seed, k, **props):
        cases.append(Case(name, cls, np.asarray(seed, dtype=np.uint8), k, props))
        return len(cases) - 1

    T.free(0, 300)
    T.free(1, 300)
    # ---- length: one locus; every long seed is a prefix of it with its substitutions
    locus = _rand(rng, max(LONG_LENGTHS))
    long_at = T.plant(0, locus)
    # ---- cap: R exact copies and one variant per family
    families = {}
    for name, R, k in CAP_FAMILIES:
        unit = _rand(rng, CAP_UNIT)
        at = [T.plant(1, unit, gap=int(rng.integers(15, 30))) for _ in range(R)]
        variant = T.plant(1, _sub(unit, [_cap_variant_at(k)], rng), gap=21)
        families[name] = (unit, at, variant)
    # ---- tiny: a string of TINY_MAX symbols; behind each of its proper prefixes every letter
    tiny = _rand(rng, TINY_MAX)
    tiny_at = T.plant(1, tiny)
    for j in range(1, TINY_MAX):
        for c in range(1, 5):
            if c != tiny[j]:
                T.plant(1, np.concatenate([tiny[:j], [c]]), gap=5)
    before, after = _rand(rng, 30), _rand(rng, 30)
    before[-1], after[0] = 2, 3                                    # (the run of A ends where it is written to end)
    T.plant(1, before)
    homo_at = T.plant(1, np.full(200, 1, np.uint8), gap=0)
    T.plant(1, after, gap=0)
    with_n = _rand(rng, 12)
    with_n[5] = 5
    n_at = T.plant(1, with_n)
    # ---- random text behind it, from which the exact seeds are cut
    exact_from = len(T.refs[1]) + 50
    T.free(1, 45_000)
    T.free(0, 110_000)
    refs = T.refs
    assert not any(_has(r, ABSENT) for r in refs)
    idx = O.Index(refs)
    groups_of = lambda seq, k, n=NO_CAP: idx.search_groups(seq, k, n=n)[0]

    # ---- queue / slots: exact seeds of one occurrence from the random text of sequence 1, lengths 24..40 in turn
    rng = _rng("exact")
    exact, k1 = [], []
    at = exact_from
    for i in range(max(QUEUE_COUNTS)):
        ln = 24 + i % 17
        exact.append(case(f"exact_{i}", "queue", refs[1][at:at + ln], 0, locus=(1, at, 0), rows=1))
        at += ln + int(rng.integers(3, 9))
    for i in range(48):
        ln = 28 + i % 9
        seq = refs[1][at:at + ln]
        k1.append(case(f"slots_k1_{i}", "slots", seq, 1, locus=(1, at, 0), groups=len(groups_of(seq, 1))))
        at += ln + int(rng.integers(3, 9))
    k2 = []
    for i in range(8):
        seq = refs[1][at:at + 32]
        k2.append(case(f"queue_k2_{i}", "queue", _sub(seq, [9 + i], rng), 2, locus=(1, at, 1)))
        at += 40
    assert at < len(refs[1]) - 100
    launches = {}

    def launch(name, cls, members, caps=CAPS, text="own"):
        launches[name] = Launch(name, cls, text, list(members), tuple(caps))

    for n in QUEUE_COUNTS:
        launch(f"queue_{n}", "queue", exact[:n])
    for name, n in QUEUE_TAILS.items():
        launch(name, "queue", exact[300:300 + n])
    # k = 2 seeds spread among k = 0 seeds of every length (the launch itself is ordered by errors, then by length: the k = 2 seeds go
    # out first and finish among the others)
    mixed = list(exact[100:292])
    for i, c in enumerate(k2):
        mixed.insert(7 + 23 * i, c)
    launch("queue_mixed", "queue", mixed)
    for total in SLOT_TOTALS:
        members, have = [], 0
        for c in k1[total % 5:]:                                   # (another start for every total: other seeds, other ballots)
            g = cases[c].props["groups"]
            if total >= 63 and have + g <= total and len(members) < 24:
                members.append(c)
                have += g
        members += exact[400:400 + total - have]
        launch(f"slots_{total}", "slots", members)
    launch("slots_ballot", "slots", [k1[3]] * BALLOT + [exact[500]] * BALLOT)
    # ---- cap
    cap_members = []
    for name, R, k in CAP_FAMILIES:
        unit, at, variant = families[name]
        caps = sorted({1, R - 1, R, R + 1} - {0})
        cap_members.append(case(name, "cap", unit, k, R=R, caps=caps, copies=[(1, a) for a in at], variant=(1, variant)))
    launch("cap", "cap", cap_members, caps=sorted({c for i in cap_members for c in cases[i].props["caps"]}) + [NO_CAP])
    # ---- tiny
    tiny_members = []
    for ln in range(1, TINY_MAX + 1):
        for k in range(4):
            tiny_members.append(case(f"tiny_{ln}_k{k}", "tiny", tiny[:ln], k, locus=(1, tiny_at, 0), searches=len(SC.FIRST_PARTS[k]) if ln >= SC.PARTS[k] else 0))
    for ln in (12, 20):
        for k in range(4):
            tiny_members.append(case(f"tiny_homopolymer_{ln}_k{k}", "tiny", np.full(ln, 1, np.uint8), k, run=(1, homo_at, 200)))
    for k in range(3):
        tiny_members.append(case(f"tiny_n_k{k}", "tiny", with_n, k, locus=(1, n_at, 0)))
        tiny_members.append(case(f"tiny_n_off_k{k}", "tiny", np.concatenate([tiny[:6], [5], tiny[7:]]), k))       # an N where the text has none
        tiny_members.append(case(f"tiny_delimiter_k{k}", "tiny", np.concatenate([refs[0][-5:], [0], refs[1][:5]]), k))
        tiny_members.append(case(f"tiny_delimiter_first_k{k}", "tiny", np.concatenate([[0], refs[1][:9]]), k))
        tiny_members.append(case(f"tiny_delimiter_last_k{k}", "tiny", np.concatenate([refs[0][-9:], [0]]), k))
    for k in range(4):
        tiny_members.append(case(f"tiny_absent_k{k}", "tiny", ABSENT, k, absent=True))
        tiny_members.append(case(f"tiny_absent_then_text_k{k}", "tiny", np.concatenate([ABSENT, refs[1][exact_from:exact_from + 16]]), k, absent=True))
    launch("tiny", "tiny", tiny_members)
    # ---- length
    full, keyed, spare = [], [], []
    for ln in LONG_LENGTHS:
        for k in range(4):
            for s in range(k + 1):
                where = _long_subs(ln, k)[:s] if s < k else _long_subs(ln, k)
                c = case(f"length_{ln}_k{k}_s{s}", "length", _sub(locus[:ln], where, rng), k, locus=(0, long_at, s), subs=where)
                if s == k:
                    full.append(c)
                    if ln <= KEYED_MAX:
                        keyed.append(c)
                else:
                    spare.append(c)
    launch("length", "length", full, caps=(1, 50, 501, NO_CAP))
    launch("length_keyed", "length", keyed, caps=(501,))
    launch("length_spare", "length", spare, caps=(1,))
    # ---- slots_heavy: the heavy seeds of search_corpus.py in its own text
    sc = SC.build()
    launch("slots_heavy", "slots", [i for i in sc.launches["heavy"] if sc.cases[i].cls == "heavy"], caps=(1, 501, NO_CAP), text="search")

    pool, seeds, at = [], [], 0
    for i, c in enumerate(cases):
        seeds.append((at, len(c.seed), c.k, i))
        pool.append(c.seed)
        at += len(c.seed)
    return types.SimpleNamespace(refs=refs, cases=cases, pool=np.concatenate(pool), seeds=seeds, launches=launches, index=idx)


def launch_cases(name):
    """the cases of a launch (those of search_corpus.py for a launch in its text)"""
    c = build()
    L = c.launches[name]
    src = SC.build().cases if L.text == "search" else c.cases
    return [src[i] for i in L.members]


def launch_seeds(name):
    """(pool, seeds [(offset, length, errors, leaf)]) of a launch, the leaf the seed's place in the launch"""
    c = build()
    L = c.launches[name]
    src = SC.build() if L.text == "search" else c
    return src.pool, [(src.seeds[i][0], src.seeds[i][1], src.seeds[i][2], at) for at, i in enumerate(L.members)]


def text_refs(text):
    return SC.build().refs if text == "search" else build().refs


def oracle_index(text="own"):
    return SC.oracle_index() if text == "search" else build().index


def launches_of(*classes):
    return [n for n in LAUNCHES if n.split("_")[0] in classes]


@functools.lru_cache(maxsize=None)
def groups(name, cap=NO_CAP):
    """the oracle's (groups (lb, len, errors), walk counters) of every seed of a launch under a cap on its rows. Computed once and
    shared: do not change them."""
    pool, seeds = launch_seeds(name)
    idx = oracle_index(build().launches[name].text)
    return [idx.search_groups(pool[off:off + ln], k, n=cap) for off, ln, k, _ in seeds]


ORDER = {"errors_first": 0, "count_first": 1, "none": 2}
CHOICE = {"round_robin": 0, "full_groups": 1, "first_reported": 2}


@functools.lru_cache(maxsize=None)
def expected(name, hard, soft, order="count_first", choice="round_robin"):
    """the oracle's (anchors, stats) of a launch, erase on. Computed once and shared: do not change them."""
    pool, seeds = launch_seeds(name)
    return oracle_index(build().launches[name].text).search_seeds(pool, seeds, hard=hard, soft=soft, order=ORDER[order], choice=CHOICE[choice], erase=True)


# ------------------------------------------------------------------------------------------------ reads
@functools.lru_cache(maxsize=1)
def reads():
    """genome: one sequence; reads: the long reads first; long: their indices; leaves: per long read [(from, to, errors)] of its PEX
    leaves; index: the oracle's"""
    rng = _rng("reads")
    genome = rng.integers(1, 5, size=200_000).astype(np.uint8)
    out, long_ones, leaves_of = [], [], []
    for i, (at, ln) in enumerate(((20_000, 33_000), (120_000, 35_000))):
        _, leaves = O.pex_build(ln, READ_PARAMS["query_errors"], READ_PARAMS["seed_errors"])
        leaves = [(int(a), int(b) + 1, int(e)) for _, a, b, e in leaves.tolist()]
        read = genome[at:at + ln].copy()
        for a, b, e in leaves:                                     # every leaf is a seed of its own: its substitutions at its own places
            read[a:b] = _sub(read[a:b], _long_subs(b - a, e), rng)
        long_ones.append(len(out))
        leaves_of.append(leaves)
        out.append(revcomp(read) if i else read)
    for i in range(6):
        at = int(rng.integers(1000, 190_000))
        read = _sub(genome[at:at + 1200], [150 + 300 * j for j in range(i % 5)], rng)
        out.append(revcomp(read) if i % 2 else read)
    return types.SimpleNamespace(genome=[genome], reads=out, long=long_ones, leaves=leaves_of, index=O.Index([genome]))
