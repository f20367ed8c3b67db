"""A text and seeds whose hit groups sit on the switches of the anchor selection (K1b, flx_select.hip). TEST INFRASTRUCTURE ONLY.

A family is a random unit of 40 symbols and copies of it in the text, every copy followed by 30 random symbols (and led by two: the
groups of a search with insertions at the ends depend on a copy's neighbours, so they are fixed with the copy). A copy carries one
substitution (searched with one error: one group of one row and one error per copy) or two (searched with two errors: the large
counts). A copy written r times is one group of r rows. The unit itself as a copy, or one-substitution copies searched with two
errors, give groups of mixed errors, anchors of equal position and anchors that erase each other. Every count is met by asking the
CPU oracle (`Index.search_groups`) and adding or removing copies, never by asking the product.

The copies of a family are dealt to the three reference sequences against the order of the reference ids (the first copies to the last
sequence), a copy written several times may lie in two sequences, and every sequence starts with the same length of filler followed
by a copy of the first family (the unit starts at LEAD + PRE): two anchors of one seed with the same in-sequence position in two references.
"""
import functools
import types

import numpy as np

import oracle_lib as O

UNIT, PRE, SPACER, N_REFS, LEAD = 40, 2, 30, 3, 1000
FILLER = 100_000                       # random symbols between the families, over all sequences
NO_CAP = 2 ** 40

# (hard cap, soft cap, erase) of the GPU test, all count_first / round_robin
CONFIGS = [(500, 50, True), (500, 50, False), (2000, 50, True), (2000, 64, True), (2000, 65, True), (2000, 1, True), (60, 7, True)]

# name -> (groups, rows over all groups) the corpus must contain
CELLS = {
    "light_1_1": (1, 1), "light_1_5": (1, 5), "light_8_8": (8, 8), "light_8_9": (8, 9), "light_9_9": (9, 9),
    "single_1_60": (1, 60),
    "tied_16": (16, 16), "tied_17": (17, 17),
    "wave_63": (63, 63), "wave_64": (64, 64), "wave_65": (65, 65), "wave_65_multi": (65, 65 + 9),
    "wave_96": (96, 96),
    "hard_count_500": (500, 500), "hard_count_501": (501, 501), "hard_rows_500": (3, 500), "hard_rows_501": (3, 501),
    "soft_5_70": (5, 70), "soft_4_46": (4, 46),
}
# name -> groups (the rows are whatever the construction gives)
CELL_GROUPS = {"mixed_17": 17, "mixed_40": 40, "groups_512": 512, "groups_513": 513, "rerun_400": 400}


def _rand(rng, n):
    return rng.integers(1, 5, size=n).astype(np.uint8)


class _Family:
    def __init__(self, rng, name, errors, subs):
        self.rng, self.name, self.errors, self.subs = rng, name, errors, subs
        self.unit = _rand(rng, UNIT)
        self.keys = set()
        self.segments = []              # per copy: the pieces (two symbols, the copy, its spacer) it is written as

    def add(self, times=1):
        """a copy with `subs` substitutions at its own (position in 4..35, one of the three other symbols)"""
        if len(self.keys) >= (32 * 3 if self.subs == 1 else 10 ** 5):
            raise RuntimeError(f"family {self.name}: no copy left to draw")
        while True:
            key = tuple(sorted((int(self.rng.integers(4, 36)), int(self.rng.integers(1, 4))) for _ in range(self.subs)))
            if len({p for p, _ in key}) == self.subs and key not in self.keys:
                break
        self.keys.add(key)
        c = self.unit.copy()
        for p, d in key:
            c[p] = (c[p] - 1 + d) % 4 + 1
        self._write(c, times)

    def add_unit(self):
        self._write(self.unit.copy(), 1)

    def _write(self, c, times):
        self.segments.append([np.concatenate([_rand(self.rng, PRE), c, _rand(self.rng, SPACER)]) for _ in range(times)])

    def pieces(self):
        """the text of the family, one piece per written copy"""
        return [p for seg in self.segments for p in seg]

    def groups(self):
        """what the oracle finds for the unit in a text that holds only this family"""
        text = np.concatenate([_rand(self.rng, 200)] + self.pieces())
        return O.Index([text]).search_groups(self.unit, self.errors, n=NO_CAP)[0]

    def dial(self, target):
        """adds or removes single copies until the oracle reports `target` groups"""
        for _ in range(400):
            n = len(self.groups())
            if n == target:
                return self
            if n < target:
                self.add()
            else:                       # (takes out the copy added last: another one is drawn if the count falls short)
                last = max(i for i, seg in enumerate(self.segments) if len(seg) == 1)
                self.segments.pop(last)
        raise RuntimeError(f"family {self.name}: the oracle's group count does not reach {target}")


def _families(rng):
    fams = []

    def fam(name, errors=1, subs=1, copies=0, times=(), unit=False, dial=None):
        f = _Family(rng, name, errors, subs)
        for t in times:
            f.add(t)
        for _ in range(copies - len(times)):
            f.add()
        if unit:
            f.add_unit()
        if dial is not None:
            f.dial(dial)
        fams.append(f)

    fam("light_9_9", copies=9)                                   # first: its copies lead the three sequences
    fam("light_1_1", copies=1)
    fam("light_1_5", copies=1, times=(5,))
    fam("light_8_8", copies=8)
    fam("light_8_9", copies=8, times=(2,))
    fam("single_1_60", copies=1, times=(60,))
    fam("tied_16", copies=16)
    fam("tied_17", copies=17)
    fam("mixed_17", copies=8, times=(3, 2, 2), unit=True, dial=17)          # 0 and 1 errors, group lengths 1..3
    fam("mixed_40", copies=30, times=(5, 4, 3, 2, 2), unit=True, dial=40)
    fam("wave_63", copies=63)
    fam("wave_64", copies=64)
    fam("wave_65", copies=65)
    fam("wave_65_multi", copies=65, times=(4, 3, 3, 2, 2))       # 65 + 9 rows
    fam("wave_96", copies=96)
    fam("groups_512", errors=2, subs=2, copies=470, dial=512)
    fam("groups_513", errors=2, subs=2, copies=470, dial=513)
    fam("hard_count_500", errors=2, subs=2, copies=460, dial=500)
    fam("hard_count_501", errors=2, subs=2, copies=460, dial=501)
    fam("hard_rows_500", copies=3, times=(498,))
    fam("hard_rows_501", copies=3, times=(499,))
    fam("soft_5_70", copies=5, times=(40, 20, 8))
    fam("soft_4_46", copies=4, times=(40, 3, 2))                 # group lengths 1, 2, 3, 40
    fam("erase_wave64", errors=2, subs=1, copies=6)              # one-substitution copies searched with two errors: every locus is
    fam("erase_wave512", errors=2, subs=1, copies=20)            # also reached shifted by one (1 and 2 errors, equal positions)
    fam("rerun_400", errors=2, subs=2, copies=370, dial=400)     # not a seed of the corpus: the rerun test searches many copies of it
    return fams


@functools.lru_cache(maxsize=1)
def build():
    """refs: three sequences; pool, seeds [(offset, length, errors, leaf)], names: the seeds in corpus order; extra: name -> seed
    tuple of the families that are in the text but not among the seeds"""
    rng = np.random.default_rng(20240611)
    fams = _families(rng)
    refs = [[_rand(rng, LEAD)] for _ in range(N_REFS)]
    gap = FILLER // (len(fams) * N_REFS)
    for f in fams:
        pieces = f.pieces()
        n = len(pieces)
        for j, piece in enumerate(pieces):
            refs[N_REFS - 1 - (j * N_REFS) // n].append(piece)   # the first copies into the last sequence
        for r in refs:
            r.append(_rand(rng, gap))
    refs = [np.concatenate(r) for r in refs]
    pool, seeds, names, extra = [], [], [], {}

    def seed(name, seq, errors, listed=True):
        off = sum(len(p) for p in pool)
        pool.append(np.asarray(seq, dtype=np.uint8))
        if listed:
            seeds.append((off, len(seq), errors, len(seeds)))
            names.append(name)
        else:
            extra[name] = (off, len(seq), errors, 0)

    for i, f in enumerate(fams):
        seed(f.name, f.unit, f.errors, listed=f.name != "rerun_400")
        if i == 5:
            seed("nohit_a", _rand(rng, UNIT), 1)
        if i == 11:
            seed("random_a", refs[0][500:540], 1)
        if i == 17:
            seed("nohit_b", _rand(rng, 33), 2)
    seed("random_b", refs[1][700:731], 2)
    seed("random_c", refs[2][300:352], 0)
    return types.SimpleNamespace(refs=refs, pool=np.concatenate(pool), seeds=seeds, names=names, extra=extra)


@functools.lru_cache(maxsize=1)
def oracle_index():
    return O.Index(build().refs)


@functools.lru_cache(maxsize=None)
def groups(name=None):
    """the oracle's groups (lb, len, errors) of every seed of the corpus, or of one extra seed"""
    c = build()
    todo = c.seeds if name is None else [c.extra[name]]
    out = [oracle_index().search_groups(c.pool[off:off + ln], k, n=NO_CAP)[0] for off, ln, k, _ in todo]
    return out if name is None else out[0]


@functools.lru_cache(maxsize=None)
def expected(hard, soft, erase):
    """the oracle's (anchors, stats) per seed of the corpus, computed once per configuration and shared: a list of
    (anchor rows {leaf, ref, pos, errors}, stats row) in corpus order"""
    c = build()
    anchors, stats = oracle_index().search_seeds(c.pool, c.seeds, hard=hard, soft=soft, order=1, choice=0, erase=erase)
    return [(anchors[anchors[:, 0] == i][:, 1:].copy(), stats[i].copy()) for i in range(len(c.seeds))]


def assemble(per_seed, order):
    """(anchors, stats) as search_seeds returns them for the seeds per_seed[i], i in order"""
    rows, stats = [], []
    for at, i in enumerate(order):
        a, s = per_seed[i]
        rows.append(np.concatenate([np.full((len(a), 1), at, dtype=np.uint64), a], axis=1))
        stats.append(s)
    return np.concatenate(rows).reshape(-1, 5), np.array(stats, dtype=np.uint64).reshape(-1, 4)
