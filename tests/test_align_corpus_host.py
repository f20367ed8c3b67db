"""The alignment corpus (align_corpus.py) on the CPU: the oracle's two algorithms agree on it, every case has the path its construction
promises, and flx_align_shapes reports the launch shapes the GPU tests rely on. Runs anywhere: flx_align_shapes is host arithmetic."""
import collections

import pytest

import floxer_amd as F
import align_corpus as AC
from test_oracle_pins import _cigar_check


def _all_corpora():
    yield "whole", AC.whole()
    for W, R in AC.SHAPES[2:]:                      # (the corpora of (1, 2) and (2, 2) are part of the whole one)
        yield f"{W},{R}", AC.corpus(W, R)


ALL = list(_all_corpora())


@pytest.mark.parametrize("which", [name for name, _ in ALL])
def test_oracle_algorithms_agree_on_the_corpus(which):
    """the bit-vector algorithm (what the kernels are compared with elsewhere) against the matrix DP that defines the semantics, on multi-word
    structured input"""
    for c in dict(ALL)[which]:
        for mode in (0, 1, 2):
            assert AC.expected(c, mode, algo=0) == AC.expected(c, mode, algo=1), (c.name, mode)


@pytest.mark.parametrize("which", [name for name, _ in ALL])
def test_cases_have_the_paths_they_were_built_for(which):
    cases = dict(ALL)[which]
    n_found = n_none = 0
    for c in cases:
        res = AC.expected(c, 2, algo=0)
        if "twin_of" in c.props:
            assert res is None, c.name
            n_none += 1
            continue
        assert res is not None, c.name
        n_found += 1
        nm, begin, cigar = res
        assert nm <= c.k
        _cigar_check(c.ref, c.query, res)
        runs = AC.cigar_runs(cigar)
        for key in ("planted", "planted2"):
            if key in c.props:
                kind, length = c.props[key]
                of_kind = [n for n, op in runs if op == kind]
                if c.props.get("substitutions"):    # (a substitution next to the run lets a column or row of it move at equal cost)
                    assert sum(of_kind) >= length and max(of_kind, default=0) >= length // 2, (c.name, key, cigar[:200])
                else:
                    assert max(of_kind, default=0) >= length, (c.name, key, cigar[:200])
        if c.props.get("begin0"):
            assert begin == 0, c.name
        if c.props.get("end_n"):
            assert begin + sum(n for n, op in runs if op in "=XD") == len(c.ref), c.name
        if "ends_within" in c.props:              # band edges: NM <= k keeps the path this close to both ends of the window
            assert begin <= c.props["ends_within"] and begin + sum(n for n, op in runs if op in "=XD") >= len(c.ref) - c.props["ends_within"], c.name
        if "runs" in c.props:
            assert nm == c.k and len(runs) == 2 * nm + 1 == c.props["runs"], (c.name, len(runs), nm)
    # the share of "no alignment" expectations is exactly the twins' share
    twins = sum(1 for c in cases if "twin_of" in c.props)
    assert (n_found, n_none) == (len(cases) - twins, twins) and twins > 0
    by_name = {c.name: c for c in cases}
    for c in cases:
        if "twin_of" in c.props:
            assert c.k == AC.nm_of(by_name[c.props["twin_of"]]) - 1


def test_the_corpus_holds_what_the_kernels_windows_are_built_around():
    cases = AC.whole()
    cls = collections.Counter(c.cls for c in cases)
    assert set(cls) == {"gap", "band", "ties", "runs", "thresholds"}
    planted = {c.props["planted"] for c in cases if c.cls == "gap"}
    assert {("D", L) for L in AC.D_RUNS} | {("I", L) for L in AC.I_RUNS} <= planted
    assert max(c.props["runs"] for c in cases if c.cls == "runs") >= 200
    assert any(len(c.ref) == 0 for c in cases)
    assert any(len(c.ref) + c.k == len(c.query) - 1 for c in cases)
    assert any(c.k == 2 * len(c.query) for c in cases) and any(c.k == len(c.query) for c in cases)
    assert {1, 63, 64, 65} <= {len(c.query) for c in cases}
    assert all((len(c.ref) + 1) * (len(c.query) + 1) <= AC.MAX_CELLS and len(c.query) <= 5000 for _, cs in ALL for c in cs)


# what a forced corpus leaves out, and why. D1100: k = L + 2 makes the band 3L + 4 = 3304 diagonals wide and the flanks ask for more than
# 2200 rows: more than two groups at W <= 13, whose ring would wait (3304 - 64W) / 16 block-steps where a launch has slots for 127. Only
# (25, 2) holds it, in a ring that waits; the default-shape tests run it in every placement. Band edges of k >= 64W at W = 25, and the k
# deletions of k = 64W + 1 at W = 13, need 2k + 16 rows: beyond the cell cap with their columns, or a band wider than the queue.
_D1100 = ["gap_D1100_" + p for p in AC.D_PLACES]
EXPECTED_DROPPED = {
    (1, 2): _D1100, (2, 2): _D1100,
    (3, 2): ["gap_D1100_first", "gap_D1100_last"], (4, 2): ["gap_D1100_first", "gap_D1100_last"], (5, 2): ["gap_D1100_first", "gap_D1100_last"],
    (6, 2): ["gap_D1100_first", "gap_D1100_last"], (8, 2): ["gap_D1100_first", "gap_D1100_last"],
    (13, 2): ["band_dels_k833_l0r0", "gap_D1100_group"],
    (25, 2): [f"band_{kind}_k{k}_l0r0" for k in (1600, 1601) for kind in ("lead_ins", "trail_ins", "dels")],
}


@pytest.mark.parametrize("shape", AC.SHAPES, ids=lambda s: f"{s[0]},{s[1]}")
def test_nothing_is_left_out_of_a_corpus_unseen(shape):
    assert sorted(AC.dropped(*shape)) == sorted(EXPECTED_DROPPED[shape])
    if shape[0] <= 2:
        assert AC.dropped(*shape, forced=False) == ()
        planted = {(c.props["planted"], c.name.split("_")[2]) for c in AC.corpus(*shape, forced=False) if c.cls == "gap" and "planted2" not in c.props and not c.props["substitutions"]}
        assert planted == {(("D", L), p) for L in AC.D_RUNS for p in AC.D_PLACES} | {(("I", L), p) for L in AC.I_RUNS for p in AC.I_PLACES}
    cases = AC.corpus(*shape)
    assert {c.props["planted"] for c in cases if c.cls == "gap"} >= {("D", L) for L in AC.D_RUNS if L < 1100 or shape == (25, 2)} | {("I", L) for L in AC.I_RUNS}
    assert {c.name.split("_")[2] for c in cases if c.cls == "gap"} >= set(AC.D_PLACES)


def test_a_run_longer_than_the_traceback_cache_goes_through_a_waiting_ring():
    c = next(c for c in AC.corpus(25, 2) if c.props.get("planted") == ("D", 1100))
    assert AC.ring_delay(len(c.ref), len(c.query), c.k, 25, 2) > 0


# ------------------------------------------------------------------------------------------------ flx_align_shapes
def test_ring_schedule_transcription_matches_the_library(monkeypatch):
    """queue reported by the library == slots for the transcription's delay, for every job of every forced corpus"""
    monkeypatch.setenv("FLX_ALIGN_FEW_WAVES", "0")
    for W, R in AC.SHAPES:
        monkeypatch.setenv("FLX_FORCE_SHAPE", f"{W},{R}")
        _, _, jobs, what = AC.batch(AC.corpus(W, R))
        for (c, mode), (w, r, queue) in zip(what, F.align_shapes(jobs)):
            delay = AC.ring_delay(len(c.ref), len(c.query), c.k, W, R)
            slots = 0 if delay == 0 else max(32, 1 << (delay).bit_length())
            assert queue == slots, (W, R, c.name, mode, delay, queue)


@pytest.mark.parametrize("shape", AC.SHAPES, ids=lambda s: f"{s[0]},{s[1]}")
def test_forced_shape_holds_and_a_third_of_the_jobs_wait(monkeypatch, shape):
    W, R = shape
    cases = AC.corpus(W, R)
    _, _, jobs, what = AC.batch(cases)
    monkeypatch.setenv("FLX_FORCE_SHAPE", f"{W},{R}")
    monkeypatch.setenv("FLX_ALIGN_FEW_WAVES", "0")
    shapes = F.align_shapes(jobs)
    assert all((w, r) == (W, R) for w, r, _ in shapes)
    assert all(q <= AC.RING_QUEUE_MAX for _, _, q in shapes)
    for (c, mode), (_, _, queue) in zip(what, shapes):
        assert (queue == 0) == (AC.ring_delay(len(c.ref), len(c.query), c.k, W, R) == 0), (c.name, mode)
    for mode in (0, 1, 2):
        waiting = sum(1 for (c, md), s in zip(what, shapes) if md == mode and s[2] > 0)
        assert 3 * waiting >= len(cases), (mode, waiting, len(cases))
    # without FLX_ALIGN_FEW_WAVES a batch this small takes the common-shape branch, whose ring never waits whatever shape is forced: what
    # test_align_batch_on_rings_that_wait ran before it set the switch
    monkeypatch.delenv("FLX_ALIGN_FEW_WAVES")
    few = F.align_shapes(jobs)
    assert all(q == 0 for _, _, q in few)
    assert len({(w, r) for w, r, _ in few[0::3]}) == 1              # one shape per call and mode


def test_align_shapes_default_shapes_hold_every_job(monkeypatch):
    """no shape forced: per job and common shapes; none asks for more hand-over slots than a launch has, identical jobs get one shape"""
    _, _, jobs, _ = AC.batch(AC.whole())
    for few in ("0", None):
        if few is None:
            monkeypatch.delenv("FLX_ALIGN_FEW_WAVES")
        else:
            monkeypatch.setenv("FLX_ALIGN_FEW_WAVES", few)
        shapes = F.align_shapes(jobs + jobs[:30])
        assert all(w in AC.WORDS_PER_LANE and r in (1, 2, 4, 8, 16, 32, 64) and q <= AC.RING_QUEUE_MAX for w, r, q in shapes)
        assert shapes[len(jobs):] == shapes[:30]
        if few == "0":
            assert any(q > 0 for _, _, q in shapes)
    assert F.align_shapes([]) == []
    with pytest.raises(F.FloxerError):
        F.align_shapes([(0, 10, 0, 0, 1, 2)])
