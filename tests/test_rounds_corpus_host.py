"""The promises of rounds_corpus.py, proved on the CPU oracle: what the GPU test of the verification rounds relies on without checking.
No case may be rejected or skipped by the builder: a case that does not keep its promise fails here. Runs anywhere."""
import collections

import numpy as np
import pytest

import oracle_lib as O
import rounds_corpus as RC


@pytest.fixture(scope="module")
def corpus():
    return RC.build()


def _groups_of(launch, read):
    """the model's groups of one read of the launch: [(round, node, [(start, length, alone, anchor)])]"""
    return [(k[0], k[4], v) for k, v in sorted(RC.model(launch)[2].items()) if k[1] == read]


def test_text_is_what_the_docstring_says(corpus):
    T = corpus.text
    assert [len(r) for r in corpus.refs] == list(RC.SEQ_LENS) and all(20_000 <= n <= 50_000 for n in RC.SEQ_LENS)
    assert T.starts[1] - (T.starts[0] + RC.SEQ_LENS[0]) == 1 and T.starts[2] - (T.starts[1] + RC.SEQ_LENS[1]) == 4
    assert (corpus.refs[3][-RC.N_RUN:] == 5).all() and corpus.refs[3][-RC.N_RUN - 1] != 5
    assert all((T.glob[s + n:s + n + 1] == 0).all() for s, n in zip(T.starts, RC.SEQ_LENS))
    lens = sorted(len(c.read) for c in corpus.cases.values())
    assert lens[0] == 30 and 5900 <= lens[-1] <= 6100 and sum(300 <= n <= 3000 for n in lens) >= len(lens) - 3


@pytest.mark.parametrize("launch", list(RC.build().launches))
def test_anchors_are_what_the_hook_accepts(corpus, launch):
    """(read, orientation) order, leaves inside their trees, every leaf inside its sequence less its errors"""
    L = corpus.launches[launch]
    A = RC.launch_anchors(launch)
    assert [(a[0], a[1]) for a in A] == sorted((a[0], a[1]) for a in A)
    for r, o, l, ref, pos in A:
        _, leaves = RC.tree_of(corpus.cases[L.cases[r]].read, L.params)
        assert l < len(leaves) and ref < len(corpus.refs)
        assert 0 <= pos < len(corpus.refs[ref]) and pos + leaves[l][2] - leaves[l][1] + 1 <= len(corpus.refs[ref]) + leaves[l][3], (launch, L.cases[r])


@pytest.mark.parametrize("launch", list(RC.build().launches))
def test_fates_do_not_depend_on_grouping(corpus, launch):
    """the rounds written again in Python decide every anchor as the plain climb does, and the launch holds dead and at-root anchors"""
    fates, n_tests = RC.climb(launch)
    m_fates, ctr, _ = RC.model(launch)
    assert m_fates == fates
    if launch == "empty":
        assert fates == []
    elif launch == "direct":
        assert all(f == (1, RC.NULL) for f in fates) and ctr["rounds"] == 0
    else:
        assert {f[0] for f in fates} == {0, 1}, launch
        assert ctr["requests"] == n_tests + ctr["solo_decisions"]
    if launch == "all":
        assert len(fates) >= 2000


@pytest.mark.parametrize("launch", [n for n, l in RC.build().launches.items() if l.isolated])
def test_promised_counts_are_what_the_construction_yields(corpus, launch):
    promised, ctr = RC.promised(launch), RC.model(launch)[1]
    assert promised
    for name, value in promised.items():
        assert ctr[name] == value, (launch, name, ctr)


def test_dedup_jobs_are_the_distinct_tests(corpus):
    """one job per distinct (round, node, window); the same (node, window) is never asked for in two rounds here, so that is the
    number of distinct (node, window) pairs of the plain climb"""
    L = corpus.launches["dedup"]
    _, ctr, groups = RC.model("dedup")
    distinct = {(k[1], k[2], k[4], st) for k, v in groups.items() for st, _, _, _ in v}
    assert ctr["jobs"] == len(distinct) == len({(k[0],) + d for k, v in groups.items() for d in [(k[1], k[2], k[4], st) for st, _, _, _ in v]})
    for n in L.cases:
        c = corpus.cases[n]
        fates = [f for f, a in zip(RC.climb("dedup")[0], RC.launch_anchors("dedup")) if L.cases[a[0]] == n]
        assert all(f[0] == (1 if c.props.get("all_pass") else 0) for f in fates), n
    assert ctr["requests"] > 3 * ctr["jobs"]


def test_pairs_climb_in_lockstep(corpus):
    L = corpus.launches["pairs"]
    for r, n in enumerate(L.cases):
        c = corpus.cases[n]
        groups = _groups_of("pairs", r)
        assert len(groups) == c.props["pair_clusters"], n
        for _, nd, wins in groups:
            starts = sorted({w[0] for w in wins})
            inner = RC.tree_of(c.read, L.params)[0]
            assert len(starts) == c.props["windows"] == len(wins) and 1 <= starts[-1] - starts[0] <= 3 < max(8, (inner[nd][2] - inner[nd][1] + 1) // 8)
            lo_end = min(w[0] + w[1] for w in wins)
            assert RC.exists(c, 0, inner[nd], starts[-1], lo_end - starts[-1]) == bool(c.props.get("all_pass")), (n, nd)      # the intersection
            if c.props.get("all_dead"):
                assert not RC.exists(c, 0, inner[nd], starts[0], max(w[0] + w[1] for w in wins) - starts[0])                 # and the union


def test_solo_cases_split_at_their_node(corpus):
    """per case: the two members meet at T in one round and one bucket, the intersection of their windows holds no alignment, the union
    does; then the member on the true diagonal passes and the other dies at T (both_hold: both pass). Levels and orders as promised."""
    L = corpus.launches["solo"]
    fates = RC.climb("solo")[0]
    A = RC.launch_anchors("solo")
    seen = collections.Counter()
    for r, n in enumerate(L.cases):
        c = corpus.cases[n]
        inner, leaves = RC.tree_of(c.read, L.params)
        t = c.props["node"]
        at_t = [(rnd, wins) for rnd, nd, wins in _groups_of("solo", r) if nd == t]
        assert len(at_t) == 2 and at_t[1][0] == at_t[0][0] + 1, n                  # together, then alone in the next round
        wins = at_t[0][1]
        assert len(wins) == 2 and [w[2] for w in wins] == [0, 0]
        if "late" in c.props:            # the late anchor's window: not alone, directly behind one that is, further right, in its bucket
            again = at_t[1][1]
            at = next(j for j, w in enumerate(again) if not w[2])
            d = max(8, (inner[t][2] - inner[t][1] + 1) // 8)
            assert sorted(w[2] for w in again) == [0, 0, 1, 1] and at > 0 and again[at - 1][2] == 1 and A[again[at][3]][2] == c.props["late"]
            assert again[at][0] > again[at - 1][0] and (again[at][0] - again[0][0]) // d == (again[at - 1][0] - again[0][0]) // d
        else:
            assert [w[2] for w in at_t[1][1]] == [1, 1]
        (s0, n0, _, _), (s1, n1, _, _) = wins
        m, e = inner[t][2] - inner[t][1] + 1, inner[t][3]
        assert 0 < s1 - s0 == abs(c.props["shift"]) == 2 * e + (3 if c.props.get("none_holds") else 2) < max(8, m // 8)
        assert not RC.exists(c, 0, inner[t], s1, min(s0 + n0, s1 + n1) - s1), n
        assert RC.exists(c, 0, inner[t], s0, max(s0 + n0, s1 + n1) - s0), n
        mine = [(a, f) for a, f in zip(A, fates) if a[0] == r]
        if c.props.get("none_holds"):              # neither member's own window holds the alignment: both die at T
            assert not RC.exists(c, 0, inner[t], s0, n0) and not RC.exists(c, 0, inner[t], s1, n1) and [f for _, f in mine] == [(0, t)] * 2, n
            assert all(leaves[a[2]][0] == t for a, _ in mine)
            seen[("none", "")] += 1
            continue
        for a, f in mine:
            if a[2] == c.props["off_leaf"] and not c.props["both_hold"]:
                assert f == (0, t), n
            else:
                assert f[0] == 1 and inner[f[1]][0] == RC.NULL, n
        level = "lowest" if all(lf[0] == t for lf in (leaves[a[2]] for a, _ in mine)) else "top" if inner[inner[t][0]][0] == RC.NULL else "middle"
        dead_at = [i for i, (a, f) in enumerate(mine) if f[0] == 0]
        seen[("late", "") if "late" in c.props else (level, "both" if c.props["both_hold"] else "first" if dead_at == [0] else "last")] += 1
    assert seen == {(lv, o): 1 for lv in ("lowest", "middle", "top") for o in ("first", "last")} | {("top", "both"): 1, ("late", ""): 1, ("none", ""): 1}


def test_boundary_windows_lie_on_both_sides_and_never_in_one_bucket(corpus):
    L = corpus.launches["boundary"]
    T = corpus.text
    for r, n in enumerate(L.cases):
        c = corpus.cases[n]
        ra, rb = c.props["refs"]
        inner = RC.tree_of(c.read, L.params)[0]
        end_a, start_b = T.starts[ra] + len(corpus.refs[ra]), T.starts[rb]
        both = clipped = 0
        for rnd, nd, wins in _groups_of("boundary", r):
            in_a, in_b = [w for w in wins if w[0] < end_a], [w for w in wins if w[0] >= start_b]
            assert all(w[0] + w[1] <= end_a for w in in_a) and len(in_a) + len(in_b) == len(wins)
            if in_a and in_b:
                both += 1
                d = max(8, (inner[nd][2] - inner[nd][1] + 1) // 8)
                assert min(w[0] for w in in_b) - max(w[0] for w in in_a) >= d, (n, nd)
                clipped += any(w[0] + w[1] == end_a for w in in_a) and any(w[0] == start_b for w in in_b)  # clipped at the end, clipped to column 0
        assert both >= 2 and clipped >= 1, n
    assert RC.model("boundary")[1]["union_only_clusters"] == 0


def test_clipped_cases_are_clipped(corpus):
    L = corpus.launches["edges"]
    T = corpus.text
    fates = RC.climb("edges")[0]
    A = RC.launch_anchors("edges")
    for r, n in enumerate(L.cases):
        c = corpus.cases[n]
        inner, leaves = RC.tree_of(c.read, L.params)
        mine = [(a, f) for a, f in zip(A, fates) if a[0] == r]
        wins = [(nd, w) for _, nd, ws in _groups_of("edges", r) for w in ws]
        full = lambda nd: inner[nd][2] - inner[nd][1] + 1 + 2 * inner[nd][3] + 1
        if c.props.get("clipped") == "start":
            ref = mine[0][0][3]
            # (the first leaf at position 0: the window of every node above it would start e columns in front of the sequence)
            assert any(a[2] == 0 and a[4] == 0 for a, _ in mine) and any(w[0] == T.starts[ref] for nd, w in wins) and all(f[0] == 1 for _, f in mine), n
        if c.props.get("clipped") in ("end", "end_short"):
            ref = mine[0][0][3]
            end = T.starts[ref] + len(corpus.refs[ref])
            assert any(w[0] + w[1] == end and w[1] < full(nd) for nd, w in wins), n
        if c.props.get("clipped") == "end_short":
            assert any(w[1] < inner[nd][2] - inner[nd][1] + 1 - inner[nd][3] for nd, w in wins) and any(f[0] == 0 for _, f in mine), n
        if c.props.get("one_node"):
            assert len(inner) == 0 and [f for _, f in mine] == [(1, RC.NULL)] * 2 and {a[1] for a, _ in mine} == {0, 1}
        if c.props.get("parent_is_root"):
            assert len(inner) == 1 and all(f == (1, 0) for _, f in mine) and mine
        if c.props.get("no_anchor"):
            assert not mine
    assert {c.props.get("clipped") for c in (corpus.cases[n] for n in L.cases)} >= {"start", "end", "end_short"}
    assert any(f[0] == 0 for (a, f) in zip(A, fates) if L.cases[a[0]] == "edge_n_run")                      # the rows on the N run cost too much somewhere


def test_tiles_cut_runs_and_identical_windows(corpus):
    L = corpus.launches["tiles"]
    A = RC.launch_anchors("tiles")
    _, ctr, groups = RC.model("tiles")
    per_read = collections.Counter(a[0] for a in A)
    assert sorted(per_read.values())[-5:] == [64, 65, 256, 257, 700] and sum(1 for v in per_read.values() if v == 1) == 300
    # the first round: the queries of 257 and 700 anchors have requests in more than one tile, those of up to 256 never
    first = collections.defaultdict(set)
    for (rnd, r, o, tile, nd) in groups:
        if rnd == 0:
            first[r].add(tile)
    assert sorted(per_read[r] for r, tiles in first.items() if len(tiles) > 1) == [257, 700]
    assert ctr["tiled_queries"] >= 2
    # a node whose run is cut by the tile boundary, with one window on both sides of it
    cut = 0
    for (rnd, r, o, tile, nd), wins in groups.items():
        other = groups.get((rnd, r, o, tile + 1, nd))
        if other and {w[0] for w in wins} & {w[0] for w in other}:
            cut += 1
    assert cut >= 2
    assert ctr["solo_decisions"] > 0 and ctr["pair_clusters"] > 0


def test_trees_hold_several_tables_and_rounds(corpus):
    for launch, n_classes in (("trees", 6), ("trees_bu", 6), ("seed1", 4)):
        L = corpus.launches[launch]
        classes = {(len(corpus.cases[n].read), RC.errors_of(len(corpus.cases[n].read), L.params)) for n in L.cases}
        assert len(classes) >= n_classes
        _, ctr, groups = RC.model(launch)
        # a node reached from leaves of different depth in different rounds
        rounds_of_node = collections.defaultdict(set)
        for (rnd, r, o, tile, nd) in groups:
            rounds_of_node[(r, o, nd)].add(rnd)
        assert launch != "trees" or any(len(v) > 1 for v in rounds_of_node.values())
        assert {a[1] for a in RC.launch_anchors(launch)} == {0, 1}
    assert corpus.launches["trees_bu"].params.bottom_up and corpus.launches["seed1"].params.seed_errors == 1


def test_all_holds_every_main_case_and_at_least_the_isolated_counts(corpus):
    L = corpus.launches["all"]
    for iso in ("dedup", "pairs", "solo", "boundary", "edges", "tiles", "trees"):
        assert set(corpus.launches[iso].cases) <= set(L.cases)
    ctr = RC.model("all")[1]
    for name in ("pair_clusters", "solo_decisions", "requests", "jobs"):
        assert ctr[name] >= sum(RC.model(iso)[1][name] for iso in ("dedup", "pairs", "solo", "boundary")), name
    assert list(L.cases) != sorted(L.cases)


def test_hook_is_exported_and_refuses_without_a_context():
    import ctypes as C
    from floxer_amd import capi
    assert C.sizeof(capi.ClimbAnchor) == 24 and C.sizeof(capi.ClimbOptions) == 16
    n = C.c_uint64(7)
    assert capi.lib().flx_climb_anchors(None, None, None, None, 0, None, None, None, C.byref(n)) != 0


def test_tiles_exact_cuts_a_run_and_keeps_its_windows_close(corpus):
    """one query of more than 256 anchors: requests in two tiles in one round, a node's run and one window on both sides of the boundary
    (tested twice), and no two windows of a node between 3 columns and a bucket apart"""
    c = corpus.cases["tiles_exact_query"]
    assert len(c.anchors) > RC.TILE
    _, ctr, groups = RC.model("tiles_exact")
    assert ctr["tiled_queries"] > 0 and ctr["pair_clusters"] > 0
    inner = RC.tree_of(c.read, RC.MAIN)[0]
    cut = 0
    for (rnd, r, o, tile, nd), wins in groups.items():
        other = groups.get((rnd, r, o, tile + 1, nd))
        cut += bool(other and {w[0] for w in wins} & {w[0] for w in other})
        starts = sorted({w[0] for w in wins})
        d = max(8, (inner[nd][2] - inner[nd][1] + 1) // 8) if corpus.launches["tiles_exact"].cases[r] == c.name else None
        if d:
            assert all(b - a <= 3 or (b - starts[0]) // d != (a - starts[0]) // d for a, b in zip(starts, starts[1:])), (nd, starts)
    assert cut >= 1
