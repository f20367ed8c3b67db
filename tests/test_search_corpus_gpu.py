"""The seeding kernels (K1, flx_search.hip) on the corpus of search_corpus.py: the LDS windows of the text walk at their length, offset and
text-edge boundaries, and the work sharing of the filter walk (lane to lane, wave to wave, the shared row count of a seed, walks abandoned
over the hard cap), which the context's search counters show at work. test_search_corpus_host.py proves the corpus's promises on the CPU.
Bit-exact against the CPU oracle. Needs an MI355X (-m gpu)."""
import pytest

import floxer_amd as F
import search_corpus as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus_ctx():
    c = SC.build()
    ctx = F.context(F.fmindex(c.refs))
    yield c, ctx
    ctx.close()


def _set(monkeypatch, env):
    for name, value in env.items():
        monkeypatch.setenv(name, value)


# ------------------------------------------------------------------------------------------------ 1. raw groups
RAW_MODES = [{}, {"FLX_FM_NO_WINDOWS": "1"}, {"FLX_FM_NO_TEXT": "1"}, {"FLX_FM_NO_FILTER": "1"}]


@pytest.mark.parametrize("launch", ["short", "long"])
@pytest.mark.parametrize("mode", RAW_MODES, ids=lambda m: "-".join(m) or "default")
def test_raw_groups_match_oracle(corpus_ctx, monkeypatch, launch, mode):
    """every group of every seed in the oracle's order (no cap: the walk finds the groups in another order than the oracle, so a cap would
    cut another group short), with the windows, without them, without the text walk, without the filter. With the text walk the launch
    queues a subtree at least for every search the corpus promises to start on a part that occurs once (props["one_row_starts"])."""
    c, ctx = corpus_ctx
    pool, seeds = SC.launch_seeds(launch)
    exp = [g.tolist() for g, _ in SC.groups(launch)]
    promised = sum(c.cases[i].props["one_row_starts"] for i in c.launches[launch])
    monkeypatch.setenv("FLX_FM_KEYED_RAW", "1")
    _set(monkeypatch, mode)
    ctx.path_counters(reset=True)
    got = F.searcher(ctx).search_groups(pool, seeds, max_hits=2 ** 31)
    sc = ctx.search_counters()
    print(f"{launch} {mode or 'default'}: groups {len(got)}, search counters {sc}, promised one-row starts {promised}")
    by_seed = [[] for _ in seeds]
    for i, lb, ln, e in got.tolist():
        by_seed[i].append([lb, ln, e])
    for at, i in enumerate(c.launches[launch]):
        assert by_seed[at] == exp[at], (mode, c.cases[i].name, seeds[at])
    assert sc["launches"] >= 1
    if "FLX_FM_NO_TEXT" in mode:
        assert sc["subtrees_queued"] == 0
    else:
        assert promised > 0 and sc["subtrees_queued"] >= promised


# ------------------------------------------------------------------------------------------------ 2. search_seeds, default order and choice
@pytest.mark.parametrize("mode", [{}, {"FLX_FM_TEXT_MIN": "1"}], ids=lambda m: "-".join(m) or "default")
def test_search_seeds_match_oracle_on_the_whole_corpus(corpus_ctx, monkeypatch, mode):
    c, ctx = corpus_ctx
    _set(monkeypatch, mode)
    sr = F.searcher(ctx, F.search_config(500, 50, "count_first", "round_robin", True))
    for launch in c.launches:
        pool, seeds = SC.launch_seeds(launch)
        exp_a, exp_s = SC.expected(launch, 500, 50)
        ctx.path_counters(reset=True)
        got_a, got_s = sr.search_seeds(pool, seeds)
        print(f"{launch} {mode or 'default'}: anchors {len(got_a)}, search counters {ctx.search_counters()}")
        assert got_s.tolist() == exp_s.tolist(), launch
        assert got_a.tolist() == exp_a.tolist(), launch


# ------------------------------------------------------------------------------------------------ 3. sharing
SHARING_MODES = {
    "steal_after_1": {"FLX_FM_STEAL_AFTER": "1"},
    "default": {"FLX_FM_STEAL_AFTER": "64"},
    "no_mailboxes": {"FLX_FM_STEAL_AFTER": "1", "FLX_FM_NO_MAILBOXES": "1"},
    "cap_look_1": {"FLX_FM_STEAL_AFTER": "1", "FLX_FM_CAP_LOOK": "1"},
    "steal_min_0": {"FLX_FM_STEAL_MIN": "0"},
}


def _sharing_run(ctx, hard, soft):
    pool, seeds = SC.launch_seeds("heavy")
    ctx.path_counters(reset=True)
    got_a, got_s = F.searcher(ctx, F.search_config(hard, soft, "count_first", "round_robin", True)).search_seeds(pool, seeds)
    return got_a.tolist(), got_s.tolist(), ctx.search_counters(), ctx.path_counters()["search_reruns"]


@pytest.mark.parametrize("hard,soft", SC.CONFIGS)
@pytest.mark.parametrize("mode", list(SHARING_MODES))
def test_shared_walks_match_oracle(corpus_ctx, monkeypatch, mode, hard, soft):
    """the heavy launch (cap seeds, light seeds, the heavy seeds last) with the sharing forced early, at its default, without mailboxes, with a look
    at the seed's row count in every iteration, and compiled out: anchors and statistics are the oracle's whoever walked what, and the counters
    show that the path under test was taken. Which lane or wave takes a subtree depends on scheduling, so the counts are asserted against zero only."""
    c, ctx = corpus_ctx
    _set(monkeypatch, SHARING_MODES[mode])
    exp_a, exp_s = SC.expected("heavy", hard, soft)
    got_a, got_s, sc, reruns = _sharing_run(ctx, hard, soft)
    print(f"heavy launch, hard {hard} soft {soft}, {mode}: lane hand-overs {sc['lane_handovers']}, wave hand-overs {sc['wave_handovers']}, "
          f"walks abandoned {sc['walks_abandoned']}, subtrees queued {sc['subtrees_queued']}, launches {sc['launches']} (reruns {reruns})")
    assert got_s == exp_s.tolist()
    assert got_a == exp_a.tolist()
    assert sc["launches"] == 1 + reruns
    if mode in ("steal_after_1", "no_mailboxes", "cap_look_1"):
        assert sc["lane_handovers"] > 0
    if mode == "steal_after_1":
        assert sc["wave_handovers"] > 0
    if mode == "no_mailboxes":
        assert sc["wave_handovers"] == 0
    if mode == "cap_look_1":
        assert sc["walks_abandoned"] > 0
    if mode == "steal_min_0":
        assert sc["lane_handovers"] == 0 and sc["wave_handovers"] == 0 and sc["walks_abandoned"] == 0


# ------------------------------------------------------------------------------------------------ 4. scheduling independence
def test_shared_walks_do_not_depend_on_scheduling(corpus_ctx, monkeypatch):
    """three launches in one process hand other subtrees to other lanes and waves and return the same; none fails (a subtree handed between
    waves that was not taken fails the call)"""
    _, ctx = corpus_ctx
    monkeypatch.setenv("FLX_FM_STEAL_AFTER", "1")
    hard, soft = 500, 50
    exp_a, exp_s = SC.expected("heavy", hard, soft)
    runs = [_sharing_run(ctx, hard, soft) for _ in range(3)]
    for got_a, got_s, sc, _ in runs:
        print(f"heavy launch, steal after 1: lane hand-overs {sc['lane_handovers']}, wave hand-overs {sc['wave_handovers']}, walks abandoned {sc['walks_abandoned']}")
        assert got_s == runs[0][1] and got_a == runs[0][0]
    assert runs[0][1] == exp_s.tolist() and runs[0][0] == exp_a.tolist()
