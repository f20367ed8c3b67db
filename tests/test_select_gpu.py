"""The device's anchor selection (K1b, flx_select.hip) on the corpus of select_corpus.py, whose seeds sit on every switch of the
selection (test_select_host.py proves that on the CPU), and the rerun path of the search (hit buffer outgrown, subtree buffer outgrown, launch repeated).
Bit-exact against the CPU oracle. Needs an MI355X (-m gpu)."""
import functools

import numpy as np
import pytest

import floxer_amd as F
import oracle_lib as O
import select_corpus as SC

pytestmark = pytest.mark.gpu


def goes_to_host(cnt, rows, hard, soft):
    """restated from the description of seed_rows_kernel, not imported: a seed under the hard cap (by groups and by rows) goes to the
    host with more than 512 groups or with more than 64 rows to keep"""
    if cnt == 0 or cnt > hard or rows > hard:
        return False
    return cnt > 512 or min(rows, soft) > 64


@pytest.fixture(scope="module")
def corpus_ctx():
    c = SC.build()
    ctx = F.context(F.fmindex(c.refs))
    yield c, ctx
    ctx.close()


def _run(ctx, cfg, c, order, single):
    """the seeds `order` of the corpus in one call, or every seed in a call of its own; (anchors, stats, seeds selected on the host)"""
    sr = F.searcher(ctx, cfg)
    ctx.path_counters(reset=True)
    if not single:
        a, s = sr.search_seeds(c.pool, [c.seeds[i] for i in order])
    else:
        parts = [sr.search_seeds(c.pool, [c.seeds[i]]) for i in order]
        for at, (pa, _) in enumerate(parts):
            pa[:, 0] = at
        a = np.concatenate([pa for pa, _ in parts]).reshape(-1, 5)
        s = np.concatenate([ps for _, ps in parts]).reshape(-1, 4)
    return a, s, ctx.path_counters()["seeds_selected_on_host"]


@pytest.mark.parametrize("hard,soft,erase", SC.CONFIGS)
def test_selection_matches_oracle_on_the_boundary_corpus(corpus_ctx, monkeypatch, hard, soft, erase):
    c, ctx = corpus_ctx
    cfg = F.search_config(hard, soft, "count_first", "round_robin", erase)
    per_seed = SC.expected(hard, soft, erase)
    n = len(c.seeds)
    to_host = sum(goes_to_host(len(g), int(g[:, 1].sum()), hard, soft) for g in SC.groups())
    orders = [("corpus", list(range(n)), False), ("shuffled", np.random.default_rng(7).permutation(n).tolist(), False),
              ("single", list(range(n)), True)]
    for label, order, single in orders:
        exp_a, exp_s = SC.assemble(per_seed, order)
        got_a, got_s, on_host = _run(ctx, cfg, c, order, single)
        print(f"hard {hard} soft {soft} erase {erase} {label}: anchors {len(got_a)}, selected on the host {on_host} (rule: {to_host})")
        assert got_s.tolist() == exp_s.tolist(), label
        assert got_a.tolist() == exp_a.tolist(), label
        assert on_host == to_host, label
        monkeypatch.setenv("FLX_HOST_SELECT", "1")
        host_a, host_s, all_on_host = _run(ctx, cfg, c, order, single)
        monkeypatch.delenv("FLX_HOST_SELECT")
        assert all_on_host == n
        assert host_s.tolist() == got_s.tolist() and host_a.tolist() == got_a.tolist(), label


RERUN_N, RERUN_HARD, RERUN_SOFT = 1000, 500, 50


@functools.lru_cache(maxsize=1)
def _rerun_case():
    """RERUN_N copies of the seed of the family rerun_400 (G groups of one row each) and what the oracle selects for them, computed
    once for the two rerun tests"""
    c = SC.build()
    g = SC.groups("rerun_400")
    N, G = RERUN_N, len(g)
    assert G == 400 and int(g[:, 1].sum()) == G
    # flx_seeding.cpp:182-183: hit_cap = max(6 n, 1.25 * hits_per_seed * n) + 4096 * 64, hits_per_seed = 0 on a fresh lane
    first_hit_cap = 6 * N + 4096 * 64
    # flx_seeding.cpp:176: item_cap = max(8 n, 1.25 * items_per_seed * n) + 4096 * 64, items_per_seed = 0 on a fresh lane. A hit of
    # one row was a node of one row with at least two symbols to go before (the substitutions lie in 4..35 of 40 symbols), and such a
    # node is queued as a subtree (flx_fm_core.hpp:521): at least G queued subtrees per seed
    first_item_cap = 8 * N + 4096 * 64
    assert N * G > first_hit_cap and N * G > first_item_cap
    off, ln, k, _ = c.extra["rerun_400"]
    seeds = [(off, ln, k, i) for i in range(N)]
    search = functools.partial(SC.oracle_index().search_seeds, c.pool, hard=RERUN_HARD, soft=RERUN_SOFT, order=1, choice=0, erase=True)
    one_a, one_s = search([seeds[0]])
    assert int(one_s[0, 1]) == RERUN_SOFT and int(one_s[0, 3]) == 0
    exp_a, exp_s = search(seeds)
    assert len(exp_a) == N * len(one_a)
    return c, seeds, exp_a.tolist(), exp_s.tolist()


def _two_calls(expected_reruns):
    """the case on a fresh context (the lane's estimates at their start values), twice: (reruns of the first call) asserted, anchors and
    statistics against the oracle, and no rerun in the second call, which starts from the adapted estimates"""
    c, seeds, exp_a, exp_s = _rerun_case()
    ctx = F.context(F.fmindex(c.refs))
    try:
        sr = F.searcher(ctx, F.search_config(RERUN_HARD, RERUN_SOFT, "count_first", "round_robin", True))
        ctx.path_counters(reset=True)
        got_a, got_s = sr.search_seeds(c.pool, seeds)
        reruns = ctx.path_counters()["search_reruns"]
        print(f"first call: search reruns {reruns} (expected {expected_reruns}), anchors {len(got_a)}")
        assert 1 <= reruns <= 3
        assert reruns == expected_reruns
        assert got_s.tolist() == exp_s
        assert got_a.tolist() == exp_a
        ctx.path_counters(reset=True)
        again_a, again_s = sr.search_seeds(c.pool, seeds)
        reruns = ctx.path_counters()["search_reruns"]
        print(f"second call: search reruns {reruns}")
        assert reruns == 0
        assert again_s.tolist() == exp_s and again_a.tolist() == exp_a
    finally:
        ctx.close()


def test_search_rerun_when_the_hit_buffer_is_outgrown(monkeypatch):
    """Without the text walk (FLX_FM_NO_TEXT=1, read per call: no subtree is queued, counters[16] stays 0 and the items fit by
    construction) the N * G hits outgrow the first hit buffer and nothing else: one rerun, in the `counters[0] > hit_cap` branch
    (flx_seeding.cpp:272). The `sel_cap` branch (:273) is not reached: sel_cap >= hit_cap and a seed keeps at most `soft` < G rows."""
    monkeypatch.setenv("FLX_FM_NO_TEXT", "1")
    _two_calls(expected_reruns=1)


def test_search_rerun_when_the_subtree_buffer_is_outgrown_too():
    """The same input with the text walk: the first pass queues at least N * G one-row subtrees, more than the first subtree buffer
    holds, and takes the `!items_fit` branch (flx_seeding.cpp:271), which leaves hit_cap as it was; the second pass outgrows the hit
    buffer as above; the third fits. hit_cap grows only in its own branch, so the second rerun can only be the subtree buffer's."""
    _two_calls(expected_reruns=2)
