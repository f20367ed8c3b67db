"""Reads and anchors built against the structure of the verification rounds (flx_rounds.hip: vr2_request_kernel, vr2_apply_kernel; the
drivers climb_on_device / climb_on_host of flx_verify.cpp), for the hook that runs only the climb (flx_climb_anchors). TEST INFRASTRUCTURE ONLY.

A case is (name, cls, read, anchors, props): one read of its own and the anchors (orientation, leaf, reference, position) the hook is
handed for it - placed by construction, never by a search: a read is a copy of a locus with substitutions planted evenly at a third of
its error budget (so the true diagonal passes every node), and an anchor names a leaf and a position on or deliberately off that
diagonal. props is what the construction promises (checked with the CPU oracle by test_rounds_corpus_host.py, never on the product).
A launch is one hook call: reads in order, one parameter set. The text: five sequences of 20-50 kb, the padding behind sequence 0 is one
delimiter and behind sequence 1 four, sequence 3 ends in a run of N; sequence 4 holds the planted tandem repeats of the solo cases.

Two independent references, both over the oracle only (oracle_lib.pex_build / span / align mode 0):
  climb()    a plain per-anchor climb: from the leaf's parent upwards every node in the anchor's own window, to the first failure (dead,
             that node) or the root (at root, the root's index); identical tests memoised. Knows nothing of clusters, rounds or tiles.
  model()    the rounds as the header of flx_rounds.hip describes them, written again in Python: the size classes of the rounds, 256-anchor
             tiles, the sort by (node, window start, alone), buckets of max(8, rows / 8) columns from the node's first window, one job or an
             intersection and a union job per cluster, pass / dead / alone per anchor. It yields a launch's counters (rounds, requests,
             jobs, the jobs' bytes as the kernel accounts them, clusters of each form, anchors sent on alone); its fates must be
             climb()'s (which anchors pass does not depend on grouping). It knows no launch shape: it never cuts a union for its width.

Classes:
  dedup       every leaf of a read on one diagonal, the true one (forward and reverse complement) and a wrong one: every shared ancestor is
              requested once per anchor and run once; no window differs within a node
  pairs       two or three anchors of ONE leaf on diagonals 1-3 columns apart: they climb in lockstep, at every node a cluster of that
              many windows whose intersection still holds the alignment (one at a wrong locus: intersection and union hold none)
  solo        two anchors of one node T in one bucket, from leaves in different children of T, so that they meet at T first: one on the
              true diagonal, the other 2 e + 2 columns off it. The off one has passed the nodes below T because its child of T is a tandem
              repeat of that period in read and text. Intersection fails, union holds, members split. T in the lowest inner level (no
              repeat needed), a middle level, the root's children; the dead member as the query's first and as its last anchor. The mirror
              "every member holds alone although the intersection fails": all of T a tandem repeat, at the root's children.
              solo_late_arrival: two more anchors ask for T in the round in which the two members are tested alone, one and two columns
              right of the true diagonal - windows that are not alone directly behind one that is (the cluster walk must cut between them).
              solo_union_holds_no_member, the other mirror: T's rows carry exactly e substitutions, so a window that cuts one column off
              the alignment holds none; one member e + 2 columns left of the true diagonal, one e + 1 right of it, both leaves of a
              lowest-level T. The union holds the alignment, neither member does: alone, then both dead at T.
  boundary    anchors of one node at the end of one sequence and the start of the next, over the 1- and the 4-delimiter padding and the
              N run. Cluster code 2 (several windows that share no column) needs two windows of one node, in one round, less than
              max(8, rows / 8) columns apart in different sequences. An anchor whose leaf lies inside its sequence (what the search
              guarantees and the hook demands) has a window that reaches at least leaf rows + e columns back from the sequence's end, and
              an anchor that is alive at a node above its leaf's parent has passed a child of half the node's rows inside the sequence:
              in both cases the windows are further apart than the bucket. So the promise here is union_only_clusters == 0.
  edges       windows clipped to column 0 of the first and of a later sequence, clipped at a sequence's last column (still wide enough;
              and, a read that hangs over the end, down to fewer than rows - errors columns), a read whose last rows lie on the N run, a
              tree of one node, a leaf whose parent is the root, a read without anchors. Anchors handed in already dead or at the root do
              not arise through the hook: it starts every anchor alive at its leaf's parent.
  tiles       one query with 64, 65, 256, 257 and about 700 anchors (every leaf at a fan of diagonals, so the run of a node and identical
              windows straddle the 256 boundary: tested twice, decided alike), beside 300 queries of one anchor
  trees       six (length, errors) classes interleaved, one read of about 6000 rows (its anchors trimmed to every fourth leaf): several node
              tables and round classes, a node reached from leaves of different depth in different rounds
  tiles_exact one query of more than 256 anchors whose windows stay within two columns of each other or lie 60 columns off: its node runs and
              identical windows straddle the tile boundary as in tiles, and no union can outgrow a launch shape
Launches: dedup, pairs, solo, boundary (isolated: only their own cases), edges, tiles, tiles_exact, trees, all (every case of the main
parameters, reads shuffled), seed1 (seed errors 1, 8 %), trees_bu (bottom-up trees), direct (direct_full_verification: nothing climbs),
empty (no anchor). The product has no counter of its clusters. What it does report of a hook call: the requests (the device asks again
for an anchor it tests alone, the host does not: their difference is the anchors sent on alone), and, with kernel timing on, the
launches of the existence kernel (one per device round) and the bytes of the jobs it was given (window columns + node rows per job,
summed by vr2_request_kernel). The job bytes pin the job list: a cluster that is not formed, a pair job that is not written, a window
that is not de-duplicated or a tile that is not cut changes them. They are compared with model() on the launches marked exact.
The 32-bit window start in the sort key cannot be reached at test sizes (a text near 2^32 positions): not covered.
"""
import collections
import functools
import zlib

import numpy as np

import oracle_lib as O

Case = collections.namedtuple("Case", "name cls read anchors props")          # anchors: [(orientation, leaf, ref, pos)]
Launch = collections.namedtuple("Launch", "name cases params isolated exact")
Params = collections.namedtuple("Params", "rate seed_errors bottom_up direct")

MAIN = Params(0.05, 2, False, False)
SEED1 = Params(0.08, 1, False, False)
BOTTOM_UP = Params(0.05, 2, True, False)
DIRECT = Params(0.05, 2, False, True)
SEQ_LENS = (30003, 24000, 40001, 22002, 20005)        # 30003 % 4 == 3: one delimiter behind it; 24000 % 4 == 0: four
N_RUN = 40                                           # sequence 3 ends in this many N
SAMPLING = 4
NULL = 0xFFFFFFFF
TILE = 256
ROUND_SPAN = 150
COUNTERS = ("rounds", "requests", "jobs", "job_bytes", "pair_clusters", "union_only_clusters", "tiled_queries", "solo_decisions")


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _rand(rng, n):
    return rng.integers(1, 5, size=n).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def tree(length, k, s, bottom_up):
    """(inner, leaves) as lists of (parent, from, to, errors); parent NULL for the root"""
    inner, leaves = O.pex_build(length, k, s, bottom_up)
    fix = lambda rows: [(int(p) & NULL, int(f), int(t), int(e)) for p, f, t, e in rows.tolist()]
    return fix(inner), fix(leaves)


def errors_of(length, p):
    return int(O.lib().orc_fp_ceil(length * p.rate))


def tree_of(read, p):
    return tree(len(read), errors_of(len(read), p), p.seed_errors, p.bottom_up)


def path_of(tr, leaf):
    """the inner nodes from the leaf's parent up to the root"""
    inner, leaves = tr
    out, nd = [], leaves[leaf][0]
    while nd != NULL:
        out.append(nd)
        nd = inner[nd][0]
    return out


class Text:
    def __init__(self):
        rng = _rng("rounds corpus text")
        self.refs = [_rand(rng, n) for n in SEQ_LENS]
        self.refs[3][-N_RUN:] = 5
        self.planted = []                                 # (ref, from, to) of the tandem repeats

    def plant_tandem(self, ref, a, b, period, name):
        assert 0 <= a < b <= len(self.refs[ref]) and all(r != ref or b <= x or a >= y for r, x, y in self.planted), name
        unit = _rand(_rng("tandem " + name), period)
        self.refs[ref][a:b] = np.resize(unit, b - a)
        self.planted.append((ref, a, b))

    def finish(self):
        self.starts, at = [], 0
        for r in self.refs:
            self.starts.append(at)
            at += len(r) + (SAMPLING - len(r) % SAMPLING)
        self.glob = np.zeros(at, dtype=np.uint8)
        for s, r in zip(self.starts, self.refs):
            self.glob[s:s + len(r)] = r


def copy_read(seq, k, keep=()):
    """a copy with k // 3 substitutions spread evenly, none inside the half-open row ranges of `keep`"""
    c = np.array(seq, dtype=np.uint8)
    n = max(1, k // 3)
    for i in range(n):
        p = int((i + 0.5) * len(c) / n)
        if not any(a <= p < b for a, b in keep) and 1 <= c[p] <= 4:
            c[p] = c[p] % 4 + 1
    return c


# ------------------------------------------------------------------------------------------------ the cases
def _true(tr, locus, leaves=None, shift=0, orientation=0, ref=0):
    return [(orientation, l, ref, locus + tr[1][l][1] + shift) for l in (range(len(tr[1])) if leaves is None else leaves)]


def _solo_nodes(tr):
    """per level ("lowest", "middle", "top") a node T with two children, 2 e + 2 < max(8, rows / 8): (T, left child, right child)"""
    inner, leaves = tr
    kids = collections.defaultdict(list)
    for i, nd in enumerate(inner):
        if nd[0] != NULL:
            kids[nd[0]].append(i)
    leaf_parents = {l[0] for l in leaves}
    fits = lambda t: 2 * inner[t][3] + 2 < max(8, (inner[t][2] - inner[t][1] + 1) // 8)
    out = {}
    for t, nd in enumerate(inner):
        if nd[0] == NULL or not fits(t):
            continue
        if t in leaf_parents and len(kids[t]) == 0:
            out.setdefault("lowest", t)
        elif len(kids[t]) == 2 and inner[nd[0]][0] == NULL:
            out.setdefault("top", t)
        elif len(kids[t]) == 2 and inner[nd[0]][0] != NULL and inner[inner[nd[0]][0]][0] != NULL:
            out["middle"] = t                             # (the last that fits: the smallest such node)
    return out, kids


def _build_cases():
    T = Text()
    cases = {}
    rng = _rng("rounds corpus loci")

    def add(name, cls, read, anchors, **props):
        assert name not in cases
        cases[name] = Case(name, cls, np.asarray(read, dtype=np.uint8), sorted(anchors, key=lambda a: a[0]), props)

    def locus(ref, length):
        return int(rng.integers(4000, len(T.refs[ref]) - 4000 - length))

    # ---- solo first: it plants into sequence 4
    L = 3000
    k = errors_of(L, MAIN)
    tr = tree(L, k, MAIN.seed_errors, False)
    inner, leaves = tr
    levels, kids = _solo_nodes(tr)
    assert set(levels) == {"lowest", "middle", "top"}, levels
    first_leaf_in = lambda nd: next(l for l, lf in enumerate(leaves) if inner[nd][1] <= lf[1] and lf[2] <= inner[nd][2])
    assert all(inner[kids[t][0]][1] < inner[kids[t][1]][1] for t in kids if len(kids[t]) == 2)
    at = 300
    solo_plan = []
    for level, dead_first in (("lowest", False), ("lowest", True), ("middle", False), ("middle", True), ("top", False), ("top", True), ("top", "both")):
        t = levels[level]
        e, lo, hi = inner[t][3], inner[t][1], inner[t][2]
        sh = 2 * e + 2
        name = f"solo_{level}_" + ("both_hold" if dead_first == "both" else "dead_first" if dead_first else "dead_last")
        keep = []
        if level == "lowest":                              # the members are leaves of T: nothing below T to pass, no repeat
            ref, loc = 0, locus(0, L)
            l_lo, l_hi = [l for l, lf in enumerate(leaves) if lf[0] == t]
            off_leaf, true_leaf, shift = (l_lo, l_hi, -sh) if dead_first else (l_hi, l_lo, sh)
        else:
            ref, loc = 4, at + sh
            at += L + 2 * sh + 100
            if dead_first == "both":                       # all of T, and a period on either side
                T.plant_tandem(4, loc + lo - sh, loc + hi + 1 + sh, sh, name)
                keep.append((lo - sh, hi + 1 + sh))
                true_leaf, off_leaf, shift = first_leaf_in(kids[t][0]), first_leaf_in(kids[t][1]), sh
            else:                                          # the off member's child of T, and a period beyond it on the side it is shifted to
                c = kids[t][0] if dead_first else kids[t][1]
                c_lo, c_hi = inner[c][1], inner[c][2]
                a, b = (c_lo - sh, c_hi + 1) if dead_first else (c_lo, c_hi + 1 + sh)
                T.plant_tandem(4, loc + a, loc + b, sh, name)
                keep.append((a, b))
                off_leaf, shift = first_leaf_in(c), (-sh if dead_first else sh)
                true_leaf = first_leaf_in(kids[t][1] if dead_first else kids[t][0])
        solo_plan.append((name, ref, loc, keep, t, true_leaf, off_leaf, shift, dead_first))
    # ---- solo_late_arrival: a node T one of whose children is in T's own round class (T.rows <= 1.5 child rows: rare, this length has
    #      one). Two members from the small child split at T as above; a third anchor is tested at the large child in that same round and
    #      asks for T one round later, one column right of the true diagonal: a window that is not alone, sorted directly behind one that is.
    #      A fourth, of the same leaf one column further right, makes the cluster that a walk without that cut would form one of three
    #      windows: the bytes of an intersection and a union job equal those of two windows' own jobs, not those of three
    L2 = 2522
    k2 = errors_of(L2, MAIN)
    tr2 = tree(L2, k2, MAIN.seed_errors, False)
    inner2, leaves2 = tr2
    _, kids2 = _solo_nodes(tr2)
    rows2 = lambda n: inner2[n][2] - inner2[n][1] + 1
    t2, big, small = next((t, b, s) for t in kids2 if len(kids2[t]) == 2 and inner2[t][0] != NULL for b, s in (kids2[t], kids2[t][::-1])
                          if rows2(t) * 100 <= rows2(b) * ROUND_SPAN and 2 * inner2[t][3] + 2 < max(8, rows2(t) // 8))
    sh2 = 2 * inner2[t2][3] + 2
    loc2 = at + sh2
    left = inner2[small][1] < inner2[big][1]
    a, b = (inner2[small][1] - sh2, inner2[small][2] + 1) if left else (inner2[small][1], inner2[small][2] + 1 + sh2)
    T.plant_tandem(4, loc2 + a, loc2 + b, sh2, "solo_late_arrival")
    in_small = [l for l, lf in enumerate(leaves2) if inner2[small][1] <= lf[1] and lf[2] <= inner2[small][2]]
    in_big = [l for l, lf in enumerate(leaves2) if inner2[big][1] <= lf[1] and lf[2] <= inner2[big][2]]
    assert loc2 + L2 + sh2 < SEQ_LENS[4]
    T.finish()
    late = [(0, in_small[0], 4, loc2 + leaves2[in_small[0]][1]), (0, in_small[-1], 4, loc2 + leaves2[in_small[-1]][1] + (-sh2 if left else sh2)),
            (0, in_big[0], 4, loc2 + leaves2[in_big[0]][1] + 1), (0, in_big[0], 4, loc2 + leaves2[in_big[0]][1] + 2)]
    add("solo_late_arrival", "solo", copy_read(T.refs[4][loc2:loc2 + L2], k2, [(a, b)]), sorted(late, key=lambda x: x[1]),
        node=t2, solo_decisions=2, both_hold=False, off_leaf=in_small[-1], shift=-sh2 if left else sh2, late=in_big[0],
        pair_clusters=len(path_of(tr2, in_big[0])))      # the two members at T; the two late ones at every node of their path below the root, above T with the member that passed
    for name, ref, loc, keep, t, true_leaf, off_leaf, shift, dead_first in solo_plan:
        read = copy_read(T.refs[ref][loc:loc + L], k, keep)
        anchors = [(0, true_leaf, ref, loc + leaves[true_leaf][1]), (0, off_leaf, ref, loc + leaves[off_leaf][1] + shift)]
        anchors.sort(key=lambda x: x[1])
        add(name, "solo", read, anchors, node=t, solo_decisions=2, both_hold=dead_first == "both", off_leaf=off_leaf, shift=shift, pair_clusters=1)

    # ---- solo_union_holds_no_member: a lowest-level T (its members are its two leaves: nothing below to pass) whose rows carry exactly e
    #      substitutions, all inside: the alignment uses the node's whole budget, so a window that cuts one column off it holds none. One
    #      member e + 2 columns left of the true diagonal (its window ends one column short), one e + 1 right of it (its window starts one
    #      column late): 2 e + 3 apart, in one bucket; the union holds the alignment, the intersection and both members do not
    L3 = 1000
    k3 = errors_of(L3, MAIN)
    tr3 = tree(L3, k3, MAIN.seed_errors, False)
    inner3, leaves3 = tr3
    t3, (l_lo3, l_hi3) = next((t, ls) for t in range(len(inner3)) for ls in [[l for l, lf in enumerate(leaves3) if lf[0] == t]]
                              if len(ls) == 2 and inner3[t][0] != NULL and 2 * inner3[t][3] + 3 < max(8, (inner3[t][2] - inner3[t][1] + 1) // 8))
    e3, lo3, hi3 = inner3[t3][3], inner3[t3][1], inner3[t3][2]
    loc3 = locus(1, L3)
    read3 = copy_read(T.refs[1][loc3:loc3 + L3], k3, [(lo3, hi3 + 1)])
    for i in range(e3):
        p = lo3 + int((i + 0.5) * (hi3 - lo3 + 1) / e3)
        read3[p] = read3[p] % 4 + 1
    add("solo_union_holds_no_member", "solo", read3, [(0, l_lo3, 1, loc3 + leaves3[l_lo3][1] - (e3 + 2)), (0, l_hi3, 1, loc3 + leaves3[l_hi3][1] + e3 + 1)],
        node=t3, solo_decisions=2, both_hold=False, none_holds=True, off_leaf=l_lo3, shift=2 * e3 + 3, pair_clusters=1)

    # ---- dedup
    L = 1000
    k = errors_of(L, MAIN)
    tr = tree(L, k, MAIN.seed_errors, False)
    loc = locus(0, L)
    add("dedup_true", "dedup", copy_read(T.refs[0][loc:loc + L], k), _true(tr, loc), pair_clusters=0, all_pass=True)
    loc = locus(1, L)
    add("dedup_true_rc", "dedup", O.revcomp(copy_read(T.refs[1][loc:loc + L], k)), _true(tr, loc, orientation=1, ref=1), pair_clusters=0, all_pass=True)
    loc, wrong = locus(2, L), locus(0, L)
    add("dedup_wrong", "dedup", copy_read(T.refs[2][loc:loc + L], k), _true(tr, wrong), pair_clusters=0, all_dead=True)

    # ---- pairs: anchors of one leaf, so that they climb in lockstep
    for name, L, leaf_at, shifts, ref in (("pairs_two", 800, 0.3, (0, 1), 0), ("pairs_three", 800, 0.7, (-1, 0, 2), 2), ("pairs_short", 300, 0.5, (0, 3), 1),
                                          ("pairs_spread", 2000, 0.5, (-2, 1), 3)):
        k = errors_of(L, MAIN)
        tr = tree(L, k, MAIN.seed_errors, False)
        leaf = int(leaf_at * len(tr[1]))
        loc = locus(ref, L)
        add(name, "pairs", copy_read(T.refs[ref][loc:loc + L], k), [a for s in shifts for a in _true(tr, loc, [leaf], s, ref=ref)],
            pair_clusters=len(path_of(tr, leaf)) - 1, windows=len(shifts), all_pass=True)
    L = 800
    k = errors_of(L, MAIN)
    tr = tree(L, k, MAIN.seed_errors, False)
    loc, wrong = locus(1, L), locus(3, L)
    add("pairs_wrong", "pairs", copy_read(T.refs[1][loc:loc + L], k), [a for s in (0, 2) for a in _true(tr, wrong, [3], s, ref=3)],
        pair_clusters=1, windows=2, all_dead=True)

    # ---- boundary: the end of one sequence and the start of the next, one node
    L = 3000
    k = errors_of(L, MAIN)
    tr = tree(L, k, MAIN.seed_errors, False)
    inner, leaves = tr
    top = next(i for i, nd in enumerate(inner) if nd[0] != NULL and inner[nd[0]][0] == NULL and nd[1] == 0)       # the root's first child
    in_top = [l for l, lf in enumerate(leaves) if lf[2] <= inner[top][2]]
    for name, ra in (("boundary_pad1", 0), ("boundary_pad4", 1), ("boundary_n_run", 3)):
        rb = ra + 1
        end_len = inner[top][2] + 1                       # the first child of the root fits exactly in front of the end of sequence ra
        la = len(T.refs[ra])
        read = copy_read(np.concatenate([T.refs[ra][la - end_len:], T.refs[rb][:L - end_len]]), k)
        # at the end of ra: the read's first rows on their true diagonal, and the same leaves further right, so that the leaf still lies inside
        anchors = _true(tr, la - end_len, in_top[:3], ref=ra)
        for l in in_top[:2]:
            anchors.append((0, l, ra, la - (leaves[l][2] - leaves[l][1] + 1)))
        # at the start of rb: leaves of the same nodes at the first columns (windows clipped to column 0), and the rows behind end_len on theirs
        anchors += [(0, l, rb, p) for l in in_top[:3] for p in (0, 5)]
        anchors += [(0, l, rb, leaves[l][1] - end_len) for l in range(len(leaves)) if leaves[l][1] >= end_len][:3]
        add(name, "boundary", read, sorted(anchors, key=lambda a: (a[1], a[2], a[3])), union_only_clusters=0, refs=(ra, rb))

    # ---- edges
    L = 1000
    k = errors_of(L, MAIN)
    tr = tree(L, k, MAIN.seed_errors, False)
    add("edge_col0_first", "edges", copy_read(T.refs[0][:L], k), _true(tr, 0), clipped="start", all_pass=True)
    add("edge_col0_later", "edges", copy_read(T.refs[2][:L], k), _true(tr, 0, ref=2), clipped="start", all_pass=True)
    la = len(T.refs[1])
    add("edge_end_fits", "edges", copy_read(T.refs[1][la - L:], k), _true(tr, la - L, ref=1), clipped="end", all_pass=True)
    la, hang = len(T.refs[2]), 300
    inside = [l for l, lf in enumerate(tr[1]) if lf[2] < L - hang]
    add("edge_end_short", "edges", np.concatenate([copy_read(T.refs[2][la - (L - hang):], k), _rand(rng, hang)]), _true(tr, la - (L - hang), inside, ref=2),
        clipped="end_short")
    la = len(T.refs[3])
    inside = [l for l, lf in enumerate(tr[1]) if lf[2] < L - N_RUN]
    add("edge_n_run", "edges", np.concatenate([copy_read(T.refs[3][la - L:la - N_RUN], k), _rand(rng, N_RUN)]), _true(tr, la - L, inside, ref=3), clipped="end")
    loc = locus(0, 30)
    assert len(tree(30, errors_of(30, MAIN), 2, False)[0]) == 0
    add("edge_one_node", "edges", T.refs[0][loc:loc + 30].copy(), [(0, 0, 0, loc), (1, 0, 0, loc)], one_node=True)
    L2 = next(n for n in range(40, 200) if len(tree(n, errors_of(n, MAIN), 2, False)[0]) == 1)
    loc = locus(1, L2)
    add("edge_parent_is_root", "edges", T.refs[1][loc:loc + L2].copy(), _true(tree(L2, errors_of(L2, MAIN), 2, False), loc, ref=1), parent_is_root=True)
    add("edge_no_anchor", "edges", _rand(rng, 500), [], no_anchor=True)

    # ---- tiles: every leaf of a query at a fan of diagonals
    L = 1000
    k = errors_of(L, MAIN)
    tr = tree(L, k, MAIN.seed_errors, False)
    fan = -(-704 // len(tr[1]))
    for n in (64, 65, 256, 257, 700):
        ref = n % 4
        loc = locus(ref, L)
        anchors = [a for l in range(len(tr[1])) for s in range(-(fan // 2), fan - fan // 2) for a in _true(tr, loc, [l], s, ref=ref)]
        add(f"tiles_{n}", "tiles", copy_read(T.refs[ref][loc:loc + L], k), anchors[:n], n_anchors=n)
    # one query of more than 256 anchors whose windows stay within two columns of each other (each leaf on the true diagonal, two columns
    # right of it and 60 off, six times over): no union is wider than a launch shape holds, so the device's job list is the model's
    ref, loc = 2, locus(2, L)
    anchors = [a for l in range(len(tr[1])) for _ in range(6) for s in (0, 2, 60) for a in _true(tr, loc, [l], s, ref=ref)]
    add("tiles_exact_query", "tiles_exact", copy_read(T.refs[ref][loc:loc + L], k), anchors, n_anchors=len(anchors))
    L = 300
    k = errors_of(L, MAIN)
    tr = tree(L, k, MAIN.seed_errors, False)
    for i in range(300):
        ref = i % 4
        loc = locus(ref, L)
        leaf = i % len(tr[1])
        add(f"tiles_single_{i}", "tiles", copy_read(T.refs[ref][loc:loc + L], k), _true(tr, loc, [leaf], (0, 0, 1, 40)[i % 4], orientation=0, ref=ref), n_anchors=1)

    # ---- trees: six classes interleaved, on both orientations, true and a few columns off
    def tree_cases(prefix, cls, p, lengths):
        for i, L in enumerate(lengths):
            k = errors_of(L, p)
            tr = tree(L, k, p.seed_errors, p.bottom_up)
            ref = i % 4
            loc = locus(ref, L)
            o = i % 2
            seq = copy_read(T.refs[ref][loc:loc + L], k)
            picks = range(0, len(tr[1]), 4 if L > 5000 else 1)
            anchors = [a for l in picks for s in ((0, 2, 60) if l % 3 == 0 else (0,)) for a in _true(tr, loc, [l], s, o, ref)]
            add(f"{prefix}_{i}_{L}", cls, O.revcomp(seq) if o else seq, anchors, length=L)

    tree_cases("trees", "trees", MAIN, (300, 6000, 450, 1700, 300, 2999, 450, 1000, 1700, 800, 2999, 1000))
    tree_cases("trees_bu", "trees_bu", BOTTOM_UP, (300, 3000, 450, 1700, 300, 800, 450, 1000, 1700, 3000))
    tree_cases("seed1", "seed1", SEED1, (300, 1000, 2000, 500, 300, 1000))
    # seed errors 1: a lockstep pair as well
    L = 600
    k = errors_of(L, SEED1)
    tr = tree(L, k, 1, False)
    loc = locus(0, L)
    add("seed1_pair", "seed1", copy_read(T.refs[0][loc:loc + L], k), [a for s in (0, 1) for a in _true(tr, loc, [2], s)], windows=2)
    return T, cases


Corpus = collections.namedtuple("Corpus", "text refs cases launches")


@functools.lru_cache(maxsize=None)
def build():
    T, cases = _build_cases()
    by_cls = collections.defaultdict(list)
    for c in cases.values():
        by_cls[c.cls].append(c.name)
    main = [n for n, c in cases.items() if c.cls not in ("trees_bu", "seed1")]
    order = _rng("all").permutation(len(main)).tolist()
    launches = {}
    # exact: the launches on which the device is expected to cut no union for its width, so that its job list is the model's: windows of
    # a node at most three columns apart or a bucket away, and the solo clusters' 2 e + 2 (the launch shape of a round holds 4 e + 1
    # diagonals and, flx_device.hip shape_width_cap, a good deal more). Not tiles and all: their fans of diagonals are cut here and there.
    # Where the expectation is wrong the GPU test's job bytes differ from the model's and say so
    for name, names, p, iso, exact in (
            ("dedup", by_cls["dedup"], MAIN, True, True), ("pairs", by_cls["pairs"], MAIN, True, True), ("solo", by_cls["solo"], MAIN, True, True),
            ("boundary", by_cls["boundary"], MAIN, True, True), ("edges", by_cls["edges"], MAIN, False, True), ("tiles", by_cls["tiles"], MAIN, False, False),
            ("tiles_exact", by_cls["tiles_exact"] + by_cls["dedup"], MAIN, False, True), ("trees", by_cls["trees"], MAIN, False, True),
            ("all", [main[i] for i in order], MAIN, False, False), ("seed1", by_cls["seed1"], SEED1, False, True),
            ("trees_bu", by_cls["trees_bu"], BOTTOM_UP, False, True), ("direct", by_cls["pairs"] + by_cls["dedup"], DIRECT, False, True),
            ("empty", by_cls["dedup"], MAIN, False, True)):
        launches[name] = Launch(name, tuple(names), p, iso, exact)
    return Corpus(T, T.refs, cases, launches)


def launch_reads(launch):
    c = build()
    return [c.cases[n].read for n in c.launches[launch].cases]


def launch_anchors(launch):
    """rows (read, orientation, leaf, reference, position) in (read, orientation) order, as the hook wants them"""
    c = build()
    if launch == "empty":
        return []
    return [(r, o, l, ref, pos) for r, n in enumerate(c.launches[launch].cases) for o, l, ref, pos in c.cases[n].anchors]


# ------------------------------------------------------------------------------------------------ existence tests on the oracle, memoised
_tests = {}


def oriented(case, o):
    return O.revcomp(case.read) if o else case.read


def exists(case, o, nd, gstart, n):
    """is there an alignment of the node's rows with at most its errors in text[gstart, gstart + n) (global, padded text)"""
    key = (case.name, o, nd[1], nd[2], nd[3], gstart, n)
    if key not in _tests:
        c = build()
        _tests[key] = O.align(c.text.glob[gstart:gstart + n], oriented(case, o)[nd[1]:nd[2] + 1], nd[3], mode=0) is not None
    return _tests[key]


# ------------------------------------------------------------------------------------------------ reference 1: the plain climb
@functools.lru_cache(maxsize=None)
def climb(launch):
    """per anchor of the launch: (status 0 dead / 1 at root, node), and the number of tests over all anchors (not memoised)"""
    c = build()
    L = c.launches[launch]
    out, n_tests = [], 0
    for r, o, l, ref, pos in launch_anchors(launch):
        case = c.cases[L.cases[r]]
        inner, leaves = tree_of(case.read, L.params)
        nd = leaves[l][0]
        if L.params.direct or nd == NULL:
            out.append((1, NULL))
            continue
        status = 1
        while inner[nd][0] != NULL:
            off, length, _ = O.span(pos, inner[nd][1], inner[nd][2], inner[nd][3], leaves[l][1], len(c.refs[ref]), 0.0)
            n_tests += 1
            if not exists(case, o, inner[nd], c.text.starts[ref] + off, length):
                status = 0
                break
            nd = inner[nd][0]
        out.append((status, nd))
    return out, n_tests


# ------------------------------------------------------------------------------------------------ reference 2: the rounds
def window(c, inner_nd, leaf_from, ref, pos):
    """(global start, length) of the anchor's window of the node: verification.cpp:157-184 without extension"""
    start = max(0, pos - (leaf_from - inner_nd[1]) - inner_nd[3])
    return c.text.starts[ref] + start, min(inner_nd[2] - inner_nd[1] + 1 + 2 * inner_nd[3] + 1, len(c.refs[ref]) - start)


@functools.lru_cache(maxsize=None)
def model(launch):
    """the rounds of the launch: (fates per anchor, counters, groups); groups: per (round, read, orientation, tile, node) the list of
    (window start, length, alone, anchor) in sorted order - what the host test checks the promises on"""
    c = build()
    L = c.launches[launch]
    A = launch_anchors(launch)
    trees = [tree_of(c.cases[n].read, L.params) for n in L.cases]
    ctr = dict.fromkeys(COUNTERS, 0)
    node, state = [NULL] * len(A), ["root"] * len(A)          # climbing / alone / dead / root
    q_first = {}
    for i, (r, o, l, ref, pos) in enumerate(A):
        q_first.setdefault((r, o), i)
        inner, leaves = trees[r]
        if L.params.direct or leaves[l][0] == NULL:
            continue
        node[i] = leaves[l][0]
        if inner[node[i]][0] != NULL:
            state[i] = "climbing"
    rows = lambda i: trees[A[i][0]][0][node[i]][2] - trees[A[i][0]][0][node[i]][1] + 1
    groups = {}
    while True:
        live = [i for i in range(len(A)) if state[i] in ("climbing", "alone")]
        if not live:
            break
        limit = min(rows(i) for i in live) * ROUND_SPAN // 100
        rnd = ctr["rounds"]
        ctr["rounds"] += 1
        tiles = collections.defaultdict(list)
        for i in live:
            if rows(i) <= limit:
                r, o = A[i][0], A[i][1]
                tiles[(r, o, (i - q_first[(r, o)]) // TILE)].append(i)
        per_query = collections.Counter((r, o) for r, o, _ in tiles)
        ctr["tiled_queries"] += sum(1 for v in per_query.values() if v > 1)
        decided = {}
        for (r, o, tile), members in sorted(tiles.items()):
            case = c.cases[L.cases[r]]
            inner, leaves = trees[r]
            req = []
            for i in members:
                st, ln = window(c, inner[node[i]], leaves[A[i][2]][1], A[i][3], A[i][4])
                req.append((node[i], st, 1 if state[i] == "alone" else 0, ln, i))
            req.sort(key=lambda x: x[:3])
            ctr["requests"] += len(req)
            for nd in sorted({x[0] for x in req}):
                run = [x for x in req if x[0] == nd]
                groups[(rnd, r, o, tile, nd)] = [(st, ln, alone, i) for _, st, alone, ln, i in run]
                m, e = inner[nd][2] - inner[nd][1] + 1, inner[nd][3]
                d, first = max(8, m // 8), run[0][1]
                clusters, prev = [], None
                for _, st, alone, ln, i in run:
                    key = (st, alone)
                    if prev is not None and key == prev[0]:
                        clusters[-1][-1][2].append(i)
                        continue
                    bucket = (st - first) // d
                    cur = clusters[-1] if clusters else None
                    apart = cur is None or alone or prev[2] or bucket != prev[1]
                    if apart:
                        clusters.append([])
                    clusters[-1].append((st, ln, [i]))
                    prev = (key, bucket, alone)
                for cl in clusters:
                    lo_start, hi_start = min(w[0] for w in cl), max(w[0] for w in cl)
                    lo_end, hi_end = min(w[0] + w[1] for w in cl), max(w[0] + w[1] for w in cl)
                    # (the bytes the kernel accounts per job: its window's columns and the node's rows)
                    if len(cl) == 1:
                        ctr["jobs"] += 1
                        ctr["job_bytes"] += hi_end - lo_start + m
                        verdict = "pass" if exists(case, o, inner[nd], lo_start, hi_end - lo_start) else "dead"
                    else:
                        both = lo_end > hi_start
                        ctr["jobs"] += 2 if both else 1
                        ctr["job_bytes"] += hi_end - lo_start + m + (lo_end - hi_start + m if both else 0)
                        ctr["pair_clusters" if both else "union_only_clusters"] += 1
                        if both and exists(case, o, inner[nd], hi_start, lo_end - hi_start):
                            verdict = "pass"
                        else:
                            verdict = "alone" if exists(case, o, inner[nd], lo_start, hi_end - lo_start) else "dead"
                    for w in cl:
                        for i in w[2]:
                            decided[i] = verdict
        for i, verdict in decided.items():
            inner = trees[A[i][0]][0]
            if verdict == "pass":
                node[i] = inner[node[i]][0]
                state[i] = "root" if inner[node[i]][0] == NULL else "climbing"
            elif verdict == "dead":
                state[i] = "dead"
            else:
                state[i] = "alone"
                ctr["solo_decisions"] += 1
    return [(1 if s == "root" else 0, n) for s, n in zip(state, node)], ctr, groups


def promised(launch):
    """the counters an isolated launch promises from its construction alone (the cases' props): name -> value"""
    c = build()
    L = c.launches[launch]
    cs = [c.cases[n] for n in L.cases]
    fates, n_tests = climb(launch)
    if launch == "dedup":
        return dict(pair_clusters=0, union_only_clusters=0, solo_decisions=0, requests=n_tests)
    if launch == "pairs":
        return dict(pair_clusters=sum(x.props["pair_clusters"] for x in cs), jobs=2 * sum(x.props["pair_clusters"] for x in cs), solo_decisions=0,
                    union_only_clusters=0, requests=n_tests)
    if launch == "solo":
        solos = sum(x.props["solo_decisions"] for x in cs)
        return dict(solo_decisions=solos, pair_clusters=sum(x.props["pair_clusters"] for x in cs), union_only_clusters=0, requests=n_tests + solos)
    if launch == "boundary":
        return dict(union_only_clusters=0)
    return {}
