"""The stride corpus (tests/stride_corpus.py) is what it claims: the period is odd and its cases distinct, every state that could leak
from one job of a wave into the next is held by a named case, the periodic expansion gives distinct alignment requests, the plain
Python references agree with the library's host rules on the cases, and the periodic expansion of the expected values is what the
references give on the expanded input. No GPU."""
import numpy as np

import floxer_amd as F
import coverage_ref
import cs_ref
import errprof_ref
import leftalign_ref as LA
import oracle_lib as O
import paf_ref
import pileup_ref
import sort_ref
import stride_corpus as SC
import sv_ref
from stride_corpus import DEL, EQ, INS, X
from test_extend_host import rule as extend_rule, rule_full_matrix
from test_md_host import md_from_cigar, reference_from_md
from test_tails_host import rule as tails_rule

CASES = SC.path_cases()
BY_NAME = {c.name: c for c in CASES}
CAPS = SC.caps()
P = len(CASES)
SV_MIN = 3


def test_the_caps_are_what_the_launches_use():
    assert set(CAPS) == set(F.GRID_CAP_NAMES) and all(v > 0 and v & (v - 1) == 0 for v in CAPS.values())      # powers of two: coprime with an odd period
    assert CAPS["errprof_add"] < CAPS["coverage_add"] and CAPS["sort_census"] < CAPS["sort_strided"] == CAPS["sv_strided"]
    assert SC.n_jobs(CAPS["cs_build"], P) == 2 * CAPS["cs_build"] + P and sum(SC.multiplicity(SC.n_jobs(CAPS["cs_build"], P), P)) == 2 * CAPS["cs_build"] + P


def test_periods_are_odd_and_their_cases_distinct():
    assert P % 2 == 1 and len({c.key() for c in CASES}) == P and len(BY_NAME) == P
    sv = SC.sv_cases(CASES, SV_MIN)
    assert len(sv) % 2 == 1 and len(sv) >= 5
    al = SC.align_cases()
    assert len(al) % 2 == 1 and len({(w.tobytes(), q.tobytes(), k) for _, w, q, k in al}) == len(al)
    ex = SC.extend_cases()
    assert len(ex) % 2 == 1 and len({(q.tobytes(), t.tobytes(), d, tuple(sorted(kw.items()))) for _, q, t, d, kw in ex}) == len(ex)
    for period in (P, len(sv), len(al), len(ex)):                        # every case is followed by another one, and every case follows one
        for cap in set(CAPS.values()) | {4 * v for v in CAPS.values()}:
            assert sorted(SC.follower(a, cap, period) for a in range(period)) == list(range(period)) and all(SC.follower(a, cap, period) != a for a in range(period))


def test_every_path_case_is_true_and_holds_its_state():
    for c in CASES:
        cols, rows, nm = LA.replay(c.path, c.ref, c.qry, c.begin)        # '=' over equal letters, X over unequal ones
        assert rows == len(c.qry) and cols == c.columns() and LA.normal_form(c.path)
    assert len(BY_NAME["one_word"].path) == 1
    assert len(BY_NAME["words_64"].path) == 64 and 65 <= len(BY_NAME["words_96"].path) <= 130
    # carries that are not zero at the job's end
    assert BY_NAME["words_64"].path[-1][0] == INS and BY_NAME["words_96"].path[-1][0] == DEL and BY_NAME["ins_last"].path[-1][0] == INS      # left-align's prev_op and x
    assert BY_NAME["open_match_run"].path[-1] == (EQ, 30) and BY_NAME["long_words"].path[-1][0] == EQ      # md's pending
    assert BY_NAME["ins_last"].trail and BY_NAME["long_words"].trail and BY_NAME["long_words"].lead and BY_NAME["words_64"].lead      # sv's pending and trail
    assert BY_NAME["x_first"].path[0][0] == X and BY_NAME["x_first"].begin == 0
    long_ops = {op for op, ln in BY_NAME["long_words"].path if ln >= 64}
    assert long_ops == {EQ, X, DEL, INS}                                 # the whole-wave paths of md_build, cs_build and errprof_add
    # left-align: the word-by-word branch, and directly behind it in some wave the all-at-once branch
    assert [c.name for c in CASES if SC.merges(c)] == ["merge"]
    merge_at = [c.name for c in CASES].index("merge")
    for cap in (CAPS["cigar_left_align"],):
        behind = CASES[SC.follower(merge_at, cap, P)]
        assert not SC.merges(behind) and any(op in (INS, DEL) for op, _ in behind.path), behind.name
    moved = [c.name for c in CASES if LA.left_align(c.path, c.ref, c.qry, c.begin) != c.path]
    assert "shift" in moved and "merge" in moved and "one_word" not in moved
    for c in CASES:
        LA.check_properties(c.path, c.ref, c.qry, c.begin, LA.left_align(c.path, c.ref, c.qry, c.begin))


def test_the_world_holds_forward_and_reverse_records_of_every_case():
    w = SC.World(CASES)
    assert {int(f) for f in w.rec["flag"]} == set(SC.FLAGS) and len(w.lengths) == 2
    for c, case in enumerate(CASES):
        r = w.rec[c]
        ws = w.words[int(r["coff"]): int(r["coff"]) + int(r["clen"])]
        assert [int(x) for x in ws] == case.record_words() and pileup_ref.query_length(ws) == len(w.reads[c])
        at = int(coverage_ref.starts_of(w.lengths)[int(r["ref"])]) + int(r["pos"])
        assert (w.concat[at: at + case.columns()] == case.ref[case.begin: case.begin + case.columns()]).all()
        seq = pileup_ref.oriented(w.reads[c], r["flag"])
        assert (seq[case.lead: case.lead + len(case.qry)] == case.qry).all()
    rec = w.records(2 * P + 3)
    assert (rec[P: 2 * P] == w.rec).all() and (rec[2 * P:] == w.rec[:3]).all()
    sv = SC.sv_cases(CASES, SV_MIN)
    assert all(any(op in (INS, DEL) and ln >= SV_MIN for op, ln in c.path) for c in sv) and any(c.lead and c.trail for c in sv) and any(c.trail and not c.lead for c in sv)


def test_align_cases_on_the_oracle():
    """what K5's own words look like: one word, exactly 64, 65 to 130, a long word, an open '=' run, gaps that left-align moves and merges"""
    res = {}
    for name, w, q, k in SC.align_cases():
        r = O.align(w, q, k)
        assert r is not None, name
        path = LA.parse(r[2])
        LA.replay(path, w, q, r[1])
        res[name] = (path, LA.left_align(path, w, q, r[1]), SC.merges(SC.PathCase(name, path, w, q, r[1])))
    assert len(res["perfect"][0]) == 1 and len(res["subs_and_last"][0]) == 64 and res["subs_and_last"][0][-1][0] == X
    assert 65 <= len(res["subs_dense"][0]) <= 130 and 65 <= len(res["ragged_right"][0]) <= 130
    assert (X, 70) in res["x_run_70"][0] and res["perfect"][0][-1][0] == EQ
    assert res["del_in_a_run"][1] != res["del_in_a_run"][0] and not res["del_in_a_run"][2]      # moved, all at once
    assert res["ragged_right"][2] and any(op == INS for op, _ in res["ins_and_subs"][0])        # merged: word by word
    names = [c[0] for c in SC.align_cases()]
    cap = CAPS["cigar_left_align"]
    assert any(res[n][2] and not res[names[SC.follower(a, cap, len(names))]][2] for a, n in enumerate(names))


def test_the_periodic_expansion_gives_distinct_alignment_requests():
    al = SC.align_cases()
    n = SC.n_jobs(CAPS["md_build"], len(al))
    ref_pool, q_pool, jobs = SC.tile_align_jobs(al, n)
    assert len(jobs) == n and len({(j[0], j[2], j[1], j[3], j[4]) for j in jobs}) == n      # what dedup_requests compares
    for i in (0, len(al), n - 1):
        ro, rl, qo, ql, k, mode = jobs[i]
        name, w, q, kk = al[i % len(al)]
        assert (ref_pool[ro: ro + rl] == w).all() and (q_pool[qo: qo + ql] == q).all() and k == kk and mode == F.MODE_WITH_CIGAR
    assert jobs[0][0] == 0 and jobs[len(al)][0] == sum(len(c[1]) for c in al) and max(j[0] + j[1] for j in jobs) <= len(ref_pool)


def test_extend_cases_hold_every_stop_and_wide_behind_narrow():
    ex = SC.extend_cases()
    want = []
    for name, q, t, direction, kw in ex:
        il, jl = kw.get("row_limit", len(q)), kw.get("ref_limit", len(t))
        got = extend_rule(q[:il], t[:jl], kw.get("w", 0) or 4, kw.get("x", 0) or 100, kw.get("dm", 0) or 1024)
        if len(q) <= 120:
            assert got[:3] == rule_full_matrix(q[:il], t[:jl], kw.get("w", 0) or 4, kw.get("x", 0) or 100, kw.get("dm", 0) or 1024), name
        want.append(got)
    by = {name: w for (name, *_), w in zip(ex, want)}
    assert by["no error, the rows run out +"] == (40, 40, 0, 2) and by["no rows at all"][:3] == (0, 0, 0)      # stops at d = 0
    assert by["runs to its d_max +"][2:] == (6, 3) and by["stopped by the x-drop +"][3] == 1 and by["stopped by the x-drop +"][0] == 30
    assert by["wide: twenty errors up to the last row +"] == (260, 260, 20, 2) and by["the row limit cuts the rows -"][0] == 64 and by["the row limit cuts the rows -"][3] == 2
    assert {d for _, _, _, d, _ in ex} == {1, -1}
    # a wide final wavefront followed in the same wave by a narrow one, and the reverse
    cap, p = CAPS["ed_extend"], len(ex)
    wide = [w[2] >= 20 for w in want]
    narrow = [w[2] <= 2 for w in want]
    assert any(wide[a] and narrow[SC.follower(a, cap, p)] for a in range(p)) and any(narrow[a] and wide[SC.follower(a, cap, p)] for a in range(p))


# ------------------------------------------------------------------------------------------------ references against the host rules
def test_references_agree_with_the_host_rules_on_the_path_cases():
    ref_pool, q_pool, words, jobs = SC.pack_paths(CASES)
    got = F.left_align(ref_pool, q_pool, words, jobs)
    for c, g in zip(CASES, got):
        assert LA.path_of(g) == LA.left_align(c.path, c.ref, c.qry, c.begin), c.name
    for long in (False, True):
        got = F.cs_string(ref_pool, q_pool, words, jobs, long=long)
        for c, g in zip(CASES, got):
            assert g == cs_ref.cs_from_cigar(c.ref, c.begin, c.qry, c.words(), long), c.name
    tj = SC.tail_jobs(CASES)
    got = F.cigar_tails(words, tj)
    want = [tails_rule(c.words(), j[2] or 4, j[3] or 100, j[4] or 100) for c, j in zip(CASES, tj)]
    assert got.tolist() == want and sum(any(x[:4]) for x in want) >= 2 and sum(any(x[4:]) for x in want) >= 3 and sum(not any(x) for x in want) >= 2
    for c in CASES:                                                      # the md rule and its inverse
        md = md_from_cigar(c.ref, c.begin, c.words())
        assert reference_from_md(cs_ref.letters(c.qry), [int(x) for x in c.words()], md) == cs_ref.letters(c.ref[c.begin: c.begin + c.columns()]), c.name


def test_references_agree_with_the_host_rules_on_the_records_and_sum_over_the_period():
    w = SC.World(CASES)
    n = P + 4                                                            # one full period plus a remainder
    mult = SC.multiplicity(n, P)
    assert mult == [2] * 4 + [1] * (P - 4)
    rec = w.records(n)
    one = [w.rec[c: c + 1] for c in range(P)]
    # coverage
    o = coverage_ref.options(count_deletions=True)
    per = [coverage_ref.depth(w.lengths, r, w.words, o).astype(np.int64) for r in one]
    for r, d in zip(one, per):
        assert (F.coverage_host(w.lengths, r, w.words, coverage_ref.c_options(o)) == d).all()
    assert (sum(m * d for m, d in zip(mult, per)) == coverage_ref.depth(w.lengths, rec, w.words, o)).all()
    # pileup
    o = pileup_ref.options()
    per = [pileup_ref.counts(w.lengths, r, w.words, w.reads, o).astype(np.int64) for r in one]
    for r, d in zip(one, per):
        assert (F.pileup_host(w.lengths, r, w.words, w.reads, pileup_ref.c_options(o)) == d).all()
    assert (sum(m * d for m, d in zip(mult, per)) == pileup_ref.counts(w.lengths, rec, w.words, w.reads, o)).all()
    assert all(per_c[pileup_ref.A: pileup_ref.T + 1].sum() > 0 for per_c, c in zip(per, CASES) if any(op == X for op, _ in c.path))
    # errprof
    o = errprof_ref.options()
    per = [errprof_ref.table(w.concat, w.lengths, r, w.words, w.reads, o) for r in one]
    for r, t in zip(one, per):
        assert not errprof_ref.same(F.errprof_host(w.concat, w.lengths, r, w.words, w.reads, errprof_ref.c_options(o)), t)
    total = errprof_ref.empty()
    for m, t in zip(mult, per):
        total = errprof_ref.plus(total, errprof_ref.times(t, m))
    assert not errprof_ref.same(total, errprof_ref.table(w.concat, w.lengths, rec, w.words, w.reads, o))
    assert int(total["TOTALS"][0]) == n and int(total["POS_CLIP"].sum()) > 0
    # the sort keys, the PAF summaries
    ordinals = np.arange(n, dtype=np.uint64) + 5
    assert F.sort_host(2, rec, w.words, ordinals).tobytes() == sort_ref.entries(rec, w.words, ordinals).tobytes()
    assert F.paf_summarize_host(rec, w.words, w.read_lengths, w.lengths).tobytes() == paf_ref.summarize(rec, w.words, w.read_lengths, w.lengths).tobytes()


def test_sv_reference_host_rule_and_period():
    sv = SC.sv_cases(CASES, SV_MIN)
    w = SC.World(sv)
    o = sv_ref.options(min_length=SV_MIN, max_distance=2, min_support=1)
    p = len(sv)
    n = p + 2
    rec = w.records(n)
    per = [sv_ref.signatures(w.rec[c: c + 1], w.words, w.read_lengths, o) for c in range(p)]
    assert all(per) and all(s[0] in (sv_ref.DEL, sv_ref.INS) for sigs in per for s in sigs)
    want = sorted(s for m, sigs in zip(SC.multiplicity(n, p), per) for s in sigs * m)
    assert want == sv_ref.signatures(rec, w.words, w.read_lengths, o)    # neighbours have different reads: no junctions
    assert sv_ref.signature_tuples(F.sv_host(w.lengths, rec, w.words, w.read_lengths, sv_ref.c_options(o))) == want


def test_the_big_sv_input_has_every_kind_of_cluster_where_it_is_wanted():
    cap = CAPS["sv_strided"]
    n = cap * 256 + 300
    distinct, rec, words, read_lengths = SC.sv_big_records(n)
    o = sv_ref.options(**SC.SV_BIG)
    assert 2000 <= len(rec) <= 2100 and int(rec["clen"].max()) >= 4096
    first = np.concatenate([[0], np.cumsum([c for _, _, c in distinct])])[:-1]
    keys, sizes = [], []                                                 # (pos_a, q) of every distinct signature and its copies, then the clusters of the distinct ones
    sigs = []
    for (pos, ws, copies), at in zip(distinct, first):
        s = sv_ref.signatures(rec[at: at + 1], words, read_lengths, o)
        assert s == sorted(s) and len(s) == sum(1 for x in ws if x & 15 == DEL)
        keys += [(x, copies) for x in s]
        sigs += s
    assert sum(c for _, c in keys) == n and [k for k, _ in keys] == sorted(k for k, _ in keys)
    cl = sv_ref.clusters(sigs, o)                                        # the clusters of one copy of each: members times copies is the support
    positions = np.array([k[5] for k, _ in keys])                        # (ascending: one class, the key order is the position's)
    copies_before = np.concatenate([[0], np.cumsum([c for _, c in keys])])
    support, start, at = [], [], 0
    for c in cl:
        a, b = np.searchsorted(positions, c[6], side="left"), np.searchsorted(positions, c[7], side="right")
        assert b - a == c[3] and int(copies_before[a]) == at             # its members are neighbours in key order, the clusters come in that order
        support.append(int(copies_before[b] - copies_before[a]))
        start.append(at)
        at += support[-1]
    assert at == n and 1 in support and 2 in support and any(2 < s < 64 for s in support) and any(s > 64 for s in support)
    edge = cap * 256
    straddle = [i for i, (a, s) in enumerate(zip(start, support)) if a < edge < a + s]
    assert len(straddle) == 1 and start[straddle[0]] + support[straddle[0]] >= edge + 128      # the second round's first two waves hold it alone
    ends_in = (start[straddle[0]] + support[straddle[0]] - edge) // 64
    assert sum(1 for a in start if edge + 64 * ends_in <= a < edge + 64 * (ends_in + 1)) >= 2    # and a later wave holds several clusters
