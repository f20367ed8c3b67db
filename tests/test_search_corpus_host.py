"""The promises of search_corpus.py, checked on the CPU oracle: the guard against a corpus that silently stops reaching the boundaries of
the seeding kernels it was built for. No GPU."""
import collections

import numpy as np

import search_corpus as SC

CLASSES = ("lengths", "shift", "edges", "runs", "symbols", "filler", "heavy", "cap")


def _groups_by_case():
    """case index -> (groups, walk counters) of the oracle, over the three launches"""
    c = SC.build()
    out = {}
    for launch in c.launches:
        for i, g in zip(c.launches[launch], SC.groups(launch)):
            out[i] = g
    return out


def test_the_corpus_keeps_its_size_and_names():
    c = SC.build()
    names = [x.name for x in c.cases]
    assert len(set(names)) == len(names)
    count = collections.Counter(x.cls for x in c.cases)
    assert set(count) == set(CLASSES) and all(count[cls] > 0 for cls in CLASSES)
    assert len(c.refs) == 3 and 250_000 <= sum(len(r) for r in c.refs) <= SC.TEXT_LIMIT
    assert all(not np.any(r == 0) for r in c.refs)
    for launch, members in c.launches.items():
        assert 0 < len(members) <= 2500, launch
        assert len(set(members)) == len(members), launch
    assert {i for m in c.launches.values() for i in m} == set(range(len(c.cases)))          # every case is searched somewhere
    # the walk with keys: at most three errors, at most 0x3FFF symbols, inside the pool
    for (off, ln, k, _), x in zip(c.seeds, c.cases):
        assert k == x.k <= 3 and ln == len(x.seed) <= 0x3FFF and c.pool[off:off + ln].tolist() == x.seed.tolist(), x.name
    # building it again gives the same corpus (a second copy: the shared one stays)
    again = SC._build()
    assert [r.tolist() for r in again.refs] == [r.tolist() for r in c.refs] and again.pool.tolist() == c.pool.tolist() and again.seeds == c.seeds


def test_both_window_sizes_get_their_launch():
    c = SC.build()
    assert not SC.is_long_launch("short") and SC.is_long_launch("long") and not SC.is_long_launch("heavy")
    for launch in ("short", "long"):
        lens = {len(c.cases[i].seed) for i in c.launches[launch] if c.cases[i].cls == "lengths"}
        assert lens == set(SC.LENGTHS)
        # on either side of both windows, so in either launch some seeds have a window and some read memory
        assert {SC.WIN_SHORT - 1, SC.WIN_SHORT, SC.WIN_SHORT + 1, SC.WIN_LONG - 1, SC.WIN_LONG, SC.WIN_LONG + 1} <= lens
        for cls in ("lengths", "shift", "edges", "runs", "symbols"):
            assert any(c.cases[i].cls == cls for i in c.launches[launch]), (launch, cls)
        for k in range(4):
            for ln in SC.LENGTHS:
                subs = {len(c.cases[i].props["subs"]) for i in c.launches[launch] if c.cases[i].cls == "lengths" and c.cases[i].k == k and len(c.cases[i].seed) == ln}
                assert subs == set(range(k + 1)), (ln, k)


def test_every_planted_seed_is_found_where_it_was_planted():
    c = SC.build()
    idx = SC.oracle_index()
    by_case = _groups_by_case()
    planted = 0
    for i, x in enumerate(c.cases):
        if "locus" not in x.props:
            continue
        ref, pos, errors = x.props["locus"]
        g, _ = by_case[i]
        assert any(int(e) == errors and idx.locate(row) == (ref, pos) for lb, ln, e in g for row in range(int(lb), int(lb + ln))), (x.name, x.props)
        planted += 1
    assert planted > 1500
    # every case of the window classes but the two units that are not in the text makes the promise
    assert [x.name for x in c.cases if x.cls in ("lengths", "shift", "edges", "symbols", "runs") and "locus" not in x.props] == \
           ["runs_40_unit", "runs_40_unit_k2", "runs_120_unit"]
    for x in c.cases:
        if "copies" in x.props:
            g, _ = by_case[c.cases.index(x)]
            assert sum(int(ln) for _, ln, e in g if int(e) >= 1) >= x.props["copies"] and not any(int(e) == 0 for _, _, e in g), x.name


def test_the_edges_are_the_edges_of_the_text():
    c = SC.build()
    loci = {x.name: x.props["locus"] for x in c.cases if x.cls == "edges"}
    n0, n1, n2 = (len(r) for r in c.refs)
    assert {loci[f"edges_start{p}_exact"][:2] for p in (0, 1, 3, 4, 5, 7)} == {(0, p) for p in (0, 1, 3, 4, 5, 7)}
    assert loci["edges_start0_first"] == (0, 1, 1) and loci["edges_start0_last"] == (0, 0, 1)
    assert {loci[f"edges_end{d}_exact"][1] + SC.EDGE_LEN for d in (1, 2, 5)} == {n2, n2 - 1, n2 - 4}
    assert loci["edges_behind_delimiter_exact"] == (1, 0, 0)
    assert loci["edges_in_front_of_delimiter_exact"] == (0, n0 - SC.EDGE_LEN, 0) and loci["edges_in_front_of_delimiter2_exact"] == (1, n1 - SC.EDGE_LEN, 0)
    assert sorted(x.props["pool_offset_mod8"] for x in c.cases if x.cls == "shift") == sorted(list(range(8)) * 2)
    for x, (off, _, _, _) in zip(c.cases, c.seeds):
        if x.cls == "shift":
            assert off % 8 == x.props["pool_offset_mod8"]
    # runs: every position of the short unit, every residue mod 8 from both ends of the long one and around its middle
    at = collections.defaultdict(list)
    for x in c.cases:
        if "sub_at" in x.props:
            at[len(x.seed)].append(x.props["sub_at"])
    assert at[SC.UNIT_SHORT] == list(range(SC.UNIT_SHORT))
    assert {p % 8 for p in at[SC.UNIT_LONG] if p < 8} == set(range(8)) == {(SC.UNIT_LONG - 1 - p) % 8 for p in at[SC.UNIT_LONG] if p >= SC.UNIT_LONG - 8}
    assert sorted(x.props["subs"][1] - x.props["subs"][0] for x in c.cases if x.name.startswith("runs_40_apart")) == [7, 8, 9]


def test_one_row_starts_are_promised_for_most_planted_seeds():
    """the number the GPU test holds the counter of queued subtrees against: it must be worth asserting"""
    c = SC.build()
    for launch in ("short", "long"):
        members = [c.cases[i] for i in c.launches[launch]]
        assert all(0 <= x.props["one_row_starts"] <= len(SC.FIRST_PARTS[x.k]) for x in members)
        assert sum(x.props["one_row_starts"] >= 1 for x in members) >= 0.6 * len(members), launch
        # parts of 15 symbols or more (4^15 is far above the text's length): such a seed of the lengths class has at least one part without
        # a substitution, and a search starts on it
        assert all(x.props["one_row_starts"] >= 1 for x in members if x.cls == "lengths" and len(x.seed) >= 63 and x.k <= 2)
    assert SC.first_parts(98, 3) == [(0, 20), (40, 60), (60, 79), (79, 98)] and SC.first_parts(36, 1) == [(0, 18), (18, 36)] and SC.first_parts(24, 0) == [(0, 24)]


def test_cap_counts_are_exact_and_spread_over_groups():
    c = SC.build()
    by_case = _groups_by_case()
    targets = SC.cap_targets()
    assert sorted(targets.values()) == [60, 61, 120, 500, 501, 1000]
    seen = 0
    for i, x in enumerate(c.cases):
        if x.cls != "cap":
            continue
        g, _ = by_case[i]
        assert x.props["rows"] == targets[x.name] == int(g[:, 1].sum()), x.name
        assert len(g) == x.props["rows"] and len(set(g[:, 0].tolist())) == len(g), x.name          # one row per group, every group another row
        seen += 1
    assert seen == len(targets)
    # what that means for the selection: at the cap the seed is kept, one row over it the seed is excluded
    for hard, soft in SC.CONFIGS:
        _, stats = SC.expected("heavy", hard, soft)
        fully_excluded = {c.cases[i].name: int(stats[at, 3]) for at, i in enumerate(c.launches["heavy"]) if c.cases[i].cls == "cap"}
        for name, rows in targets.items():
            assert fully_excluded[name] == (rows > hard), (hard, name)


def test_heavy_seeds_are_heavy_and_come_last():
    c = SC.build()
    by_case = _groups_by_case()
    members = [c.cases[i] for i in c.launches["heavy"]]
    assert len(members) >= 1100 and all(x.k == 3 for x in members)
    heavy = [x for x in members if x.cls == "heavy"]
    assert len(heavy) == SC.N_HEAVY_FAMILY + SC.N_HEAVY_TANDEM == 64
    # the launch order (flx_seeding.cpp: more errors first, then shorter seeds first): the heavy seeds are the longest of one class of errors
    assert min(len(x.seed) for x in heavy) > max(len(x.seed) for x in members if x.cls != "heavy")
    light_steps = sorted(int(by_case[i][1][0]) for i in c.launches["heavy"] if c.cases[i].cls == "filler")
    rows = []
    for i in c.launches["heavy"]:
        x = c.cases[i]
        g, ctr = by_case[i]
        if "steps" in x.props:
            assert int(ctr[0]) >= x.props["steps"], (x.name, ctr)
            assert int(ctr[0]) >= 3 * light_steps[len(light_steps) // 2]
            rows.append(int(g[:, 1].sum()))
        if "rows_over" in x.props:
            assert int(g[:, 1].sum()) > x.props["rows_over"], x.name
    # seeds of the family on either side of the larger hard cap, all of them above the smaller
    assert sum(r <= 500 for r in rows) >= 10 and sum(r > 500 for r in rows) >= 10 and min(rows) > 60
