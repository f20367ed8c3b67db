"""The promises of ordered_corpus.py, checked on the CPU oracle: the guard against a corpus that silently stops reaching the queue, slot,
cap and length boundaries of the ordered walk it was built for. No GPU."""
import collections

import numpy as np

import oracle_lib as O
import ordered_corpus as OC
import search_corpus as SC

CLASSES = ("queue", "slots", "cap", "tiny", "length")


def _rows_at(idx, g):
    """(reference, position, errors) of every row of the groups"""
    return {idx.locate(row) + (int(e),) for lb, ln, e in g for row in range(int(lb), int(lb + ln))}


def test_the_corpus_keeps_its_names_and_builds_the_same_twice():
    c = OC.build()
    names = [x.name for x in c.cases]
    assert len(set(names)) == len(names)
    assert set(x.cls for x in c.cases) == set(CLASSES) == set(L.cls for L in c.launches.values())
    assert len(c.refs) == 2 and 100_000 <= sum(len(r) for r in c.refs) <= 300_000
    assert all(not np.any(r == 0) for r in c.refs)
    assert sorted(c.launches) == sorted(OC.LAUNCHES) and len(set(OC.LAUNCHES)) == len(OC.LAUNCHES)
    for name, L in c.launches.items():
        assert name == L.name and L.cls == name.split("_")[0] and 0 < len(L.members) <= 600 and len(L.caps) >= 1
    searched = {i for L in c.launches.values() if L.text == "own" for i in L.members}
    assert searched <= set(range(len(c.cases))) and {i for i, x in enumerate(c.cases) if x.cls in ("cap", "tiny", "length")} <= searched
    for (off, ln, k, _), x in zip(c.seeds, c.cases):
        assert k == x.k <= 3 and ln == len(x.seed) and c.pool[off:off + ln].tolist() == x.seed.tolist(), x.name
    again = OC._build()
    assert [r.tolist() for r in again.refs] == [r.tolist() for r in c.refs] and again.pool.tolist() == c.pool.tolist() and again.seeds == c.seeds
    assert {n: (L.members, L.caps) for n, L in again.launches.items()} == {n: (L.members, L.caps) for n, L in c.launches.items()}
    # the constants restated here are the kernel's
    assert (OC.GRAB, OC.SEEDS_PER_WAVE, OC.HIT_GRAB, OC.KEYED_MAX) == (64, 256, 64, 16383)


def test_queue_launches_have_the_listed_seed_counts():
    c = OC.build()
    assert OC.QUEUE_COUNTS == (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
    waves = lambda n: (n + OC.SEEDS_PER_WAVE - 1) // OC.SEEDS_PER_WAVE
    for n in OC.QUEUE_COUNTS:
        members = OC.launch_cases(f"queue_{n}")
        assert len(members) == n and all(x.k == 0 and 24 <= len(x.seed) <= 40 for x in members)
        # each occurs once, where it was cut
        for x, (g, _) in zip(members, OC.groups(f"queue_{n}")):
            assert g.tolist() == [[g[0, 0], 1, 0]] and c.index.locate(int(g[0, 0])) == x.props["locus"][:2], x.name
    assert [waves(n) for n in (1, 256, 257, 513)] == [1, 1, 2, 3]
    assert {len(OC.launch_cases(n)) % OC.GRAB for n in OC.QUEUE_TAILS} == {1, 63}
    assert all(len(OC.launch_cases(n)) > 2 * OC.GRAB for n in OC.QUEUE_TAILS)
    mixed = OC.launch_cases("queue_mixed")
    assert 190 <= len(mixed) <= 210 and len(mixed) <= OC.SEEDS_PER_WAVE
    assert {len(x.seed) for x in mixed if x.k == 0} == set(range(24, 41))
    heavy = [i for i, x in enumerate(mixed) if x.k == 2]
    assert 4 <= len(heavy) <= 10 and sum(x.k == 0 for x in mixed) == len(mixed) - len(heavy)
    assert min(heavy) < OC.GRAB < max(heavy)                      # (in the caller's order: among the others)
    idx = c.index
    for x, (g, _) in zip(mixed, OC.groups("queue_mixed")):
        ref, pos, errors = x.props["locus"]
        assert (ref, pos, errors) in _rows_at(idx, g), x.name


def test_slots_launches_have_the_listed_hit_totals():
    c = OC.build()
    assert OC.SLOT_TOTALS == (1, 63, 64, 65, 127, 128, 129)
    for total in OC.SLOT_TOTALS:
        name = f"slots_{total}"
        res = OC.groups(name)
        assert len(res) <= OC.SEEDS_PER_WAVE                          # one wave
        assert sum(len(g) for g, _ in res) == total, name
        if total >= 63:
            assert sum(len(g) > 1 for g, _ in res) >= 10, name        # seeds of several hits among seeds of one
    # the ballot launch: two seeds, 40 copies each; the first has two groups or more, so two ballots of 40 follow each other
    ballot = OC.launch_cases("slots_ballot")
    assert len(ballot) == 2 * OC.BALLOT and OC.HIT_GRAB // 2 < OC.BALLOT < OC.HIT_GRAB
    first, second = ballot[:OC.BALLOT], ballot[OC.BALLOT:]
    assert len({x.name for x in first}) == 1 == len({x.name for x in second}) and first[0].k == 1 and second[0].k == 0
    assert len(OC.groups("slots_ballot")[0][0]) >= 2
    # ordinals beyond the byte of the error count
    counts = [len(g) for g, _ in OC.groups("slots_heavy")]
    assert any(255 < n <= 1000 for n in counts) and any(n > 1000 for n in counts)
    assert sum(n > 500 for n in counts) >= 10                        # (reached under the hard cap of 500, too: max_hits 501)


def test_cap_families_have_a_group_of_r_rows_and_the_caps_cut_inside_it():
    c = OC.build()
    idx = c.index
    members = OC.launch_cases("cap")
    assert [(x.name, x.props["R"], x.k) for x in members] == list(OC.CAP_FAMILIES)
    assert sorted({x.props["R"] for x in members if x.k == 1}) == [2, 7, 64]
    full = OC.groups("cap")
    for at, x in enumerate(members):
        R = x.props["R"]
        assert x.props["caps"] == sorted({1, R - 1, R, R + 1} - {0}) and set(x.props["caps"]) <= set(c.launches["cap"].caps)
        g = full[at][0].tolist()
        # the first group: the R exact copies
        assert g[0][1:] == [R, 0] and len(g) > 1, x.name
        assert {idx.locate(row) for row in range(g[0][0], g[0][0] + R)} == set(x.props["copies"])
        # the variant is reported, by a later group
        variant = x.props["variant"] + (1,)
        assert any(variant in _rows_at(idx, [grp]) for grp in g[1:]), x.name
        for cap in c.launches["cap"].caps[:-1]:
            capped = OC.groups("cap", cap)[at][0].tolist()
            if cap <= R:
                # the capped emission is the first group alone, cut to the cap: every later group, the variant's among them, is lost
                assert capped == [[g[0][0], cap, 0]], (x.name, cap)
                assert variant not in _rows_at(idx, capped)
            else:
                # the first group whole; the emission differs from the uncapped one in its last group's length only
                assert capped[0] == g[0] and capped[:-1] == g[:len(capped) - 1], (x.name, cap)
                assert capped[-1][0] == g[len(capped) - 1][0] and capped[-1][2] == g[len(capped) - 1][2] and capped[-1][1] <= g[len(capped) - 1][1]
                assert sum(n for _, n, _ in capped) == min(cap, sum(n for _, n, _ in g))


def test_early_abort_cases_lose_what_a_later_search_reports():
    """the variant copy has its substitution in the part(s) that the first search walks without an error: no path of the first search
    reaches it, so the group that reports it comes from a later search, and a cap met by the first search's first group loses it"""
    c = OC.build()
    idx = c.index
    seen = set()
    for at, x in enumerate(OC.launch_cases("cap")):
        sub_at = OC._cap_variant_at(x.k)
        exact_parts = OC.long_parts(len(x.seed), x.k)[:1 if x.k < 2 else 2]
        assert exact_parts[0][0] <= sub_at < exact_parts[-1][1]
        ref, pos = x.props["variant"]
        planted = c.refs[ref][pos:pos + len(x.seed)]
        assert np.flatnonzero(planted != x.seed).tolist() == [sub_at]
        R = x.props["R"]
        capped = OC.groups("cap", R)[at][0].tolist()
        uncapped = OC.groups("cap")[at][0].tolist()
        assert len(capped) == 1 and sum(n for _, n, _ in capped) == R and len(uncapped) > 1
        assert (ref, pos, 1) in _rows_at(idx, uncapped) and (ref, pos, 1) not in _rows_at(idx, capped)
        seen.add(x.k)
    assert seen == {1, 3}


def test_tiny_seeds_cover_every_length_and_error_count():
    c = OC.build()
    idx = c.index
    members = {x.name: (x, g) for x, (g, _) in zip(OC.launch_cases("tiny"), OC.groups("tiny"))}
    tiny = members[f"tiny_{OC.TINY_MAX}_k0"][0].seed
    for ln in range(1, OC.TINY_MAX + 1):
        for k in range(4):
            x, g = members[f"tiny_{ln}_k{k}"]
            assert x.seed.tolist() == tiny[:ln].tolist() and x.k == k
            # a seed shorter than its scheme's parts has no search and no hit; every other is found where it stands
            assert (x.props["searches"] == 0) == (ln < SC.PARTS[k])
            if x.props["searches"] == 0:
                assert len(g) == 0
            else:
                assert x.props["locus"] in _rows_at(idx, g[:1]) if k == 0 else len(g) >= 1
    # all four letters follow every proper prefix
    for j in range(1, OC.TINY_MAX):
        for letter in range(1, 5):
            g, _ = idx.search_groups(np.concatenate([tiny[:j], [letter]]), 0)
            assert len(g) == 1 and g[0, 1] >= 1, (j, letter)
    # the homopolymer seeds lie inside a longer run: with k errors the run's rows and those around its ends
    for ln in (12, 20):
        for k in range(4):
            x, g = members[f"tiny_homopolymer_{ln}_k{k}"]
            ref, pos, run = x.props["run"]
            assert c.refs[ref][pos:pos + run].tolist() == [1] * run and c.refs[ref][pos - 1] != 1 and c.refs[ref][pos + run] != 1
            assert run > 2 * ln and sum(int(n) for _, n, e in g if int(e) == 0) == run - ln + 1
    assert any(np.any(x.seed == 5) for x, _ in members.values()) and any(np.any(x.seed == 0) for x, _ in members.values())
    assert len(members["tiny_n_k0"][1]) == 1 and len(members["tiny_delimiter_first_k0"][1]) == 1 == len(members["tiny_delimiter_last_k0"][1])


def test_the_absent_8mer_is_absent():
    c = OC.build()
    assert len(OC.ABSENT) == 8 and set(OC.ABSENT.tolist()) <= {1, 2, 3, 4}
    g, _ = c.index.search_groups(OC.ABSENT, 0)
    assert len(g) == 0
    word = OC.ABSENT.tobytes()
    assert all(word not in r.tobytes() for r in c.refs)
    absent = [x for x in OC.launch_cases("tiny") if x.props.get("absent")]
    assert len(absent) == 8 and all(x.seed[:8].tolist() == OC.ABSENT.tolist() for x in absent)
    assert {x.k for x in absent} == {0, 1, 2, 3}


def test_long_seeds_are_found_where_planted_within_the_extension_limit():
    c = OC.build()
    idx = c.index
    assert OC.LONG_LENGTHS == (16383, 16384, 16999) and max(OC.LONG_LENGTHS) <= 17000 and OC.EXT_LIMIT == 60_000
    combos = collections.Counter()
    worst = 0
    for name in ("length", "length_keyed", "length_spare"):
        L = c.launches[name]
        for cap in L.caps:
            for x, (g, ctr) in zip(OC.launch_cases(name), OC.groups(name, cap)):
                ref, pos, s = x.props["locus"]
                assert len(x.props["subs"]) == s <= x.k and len(x.seed) in OC.LONG_LENGTHS
                assert np.flatnonzero(c.refs[ref][pos:pos + len(x.seed)] != x.seed).tolist() == sorted(x.props["subs"])
                found = _rows_at(idx, g)
                if s == x.k:
                    assert found == {(ref, pos, s)}, (x.name, cap)             # its planted errors use the whole budget: that alignment alone
                else:
                    assert len(g) == 1 and cap == 1                          # one row: the first the walk reports, at the locus, with
                    assert {(r, p) for r, p, _ in found} == {(ref, pos)} and all(s <= e <= x.k for _, _, e in found), x.name      # spare errors used or not
                extensions = int(ctr[0] + ctr[1])
                assert extensions <= OC.EXT_LIMIT, (x.name, cap, extensions)
                worst = max(worst, extensions)
                combos[(len(x.seed), x.k, s)] += 1
    print(f"long seeds: {len(combos)} (length, errors, substitutions) combinations, at most {worst} oracle extensions for one seed under the caps it is searched with")
    assert set(combos) == {(ln, k, s) for ln in OC.LONG_LENGTHS for k in range(4) for s in range(k + 1)}
    # the launches: only the seeds longer than the keyed walk's limit turn a launch
    assert {len(x.seed) for x in OC.launch_cases("length_keyed")} == {OC.KEYED_MAX}
    assert max(len(x.seed) for x in OC.launch_cases("length")) > OC.KEYED_MAX and max(len(x.seed) for x in OC.launch_cases("length_spare")) > OC.KEYED_MAX
    assert all(len(x.props["subs"]) == x.k for x in OC.launch_cases("length") + OC.launch_cases("length_keyed"))


def test_read_leaves_are_longer_than_the_keyed_walk_takes():
    R = OC.reads()
    assert len(R.genome) == 1 and 150_000 <= len(R.genome[0]) <= 250_000
    assert 2 <= len(R.long) <= 3 and len(R.reads) - len(R.long) >= 4
    for i, leaves in zip(R.long, R.leaves):
        ln = len(R.reads[i])
        assert 33_000 <= ln <= 35_000
        _, lv = O.pex_build(ln, OC.READ_PARAMS["query_errors"], OC.READ_PARAMS["seed_errors"])
        assert [(int(a), int(b) + 1, int(e)) for _, a, b, e in lv.tolist()] == leaves and len(leaves) == 2
        assert all(b - a > OC.KEYED_MAX and e == OC.READ_PARAMS["seed_errors"] for a, b, e in leaves)
        assert sum(e for _, _, e in leaves) <= OC.READ_PARAMS["query_errors"]
    assert all(len(r) == 1200 for i, r in enumerate(R.reads) if i not in R.long)
    # every leaf of a long read within the extension limit, as a seed of the oracle under the default cap, in either orientation
    for i, leaves in zip(R.long, R.leaves):
        for read in (R.reads[i], OC.revcomp(R.reads[i])):
            for a, b, e in leaves:
                _, ctr = R.index.search_groups(read[a:b], e, n=501)
                print(f"read {i} leaf [{a}, {b}): {int(ctr[0] + ctr[1])} oracle extensions")
                assert int(ctr[0] + ctr[1]) <= OC.EXT_LIMIT, (i, a, b, ctr)
    exp = R.index.run(R.reads, O.params(**OC.READ_PARAMS))
    mapped = {r[0] for r in exp.records() if not r[1] & 4}
    assert set(R.long) <= mapped and len(mapped) == len(R.reads) and not exp.skipped.any()
