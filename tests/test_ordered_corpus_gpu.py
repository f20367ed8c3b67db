"""The ordered FM-index walk (K1', fm_search_ordered_kernel of flx_search_ordered.hip) on the corpus of ordered_corpus.py: its seed queue at
the sizes of a grab and of a wave, its hit-slot ranges at their size, the cap on a seed's rows inside a group, tiny seeds, seeds longer
than the walk with keys takes, and behind it both consumers of its hits - the host's grouping and the device selection's scatter by
ordinal. test_ordered_corpus_host.py proves the corpus's promises on the CPU. Bit-exact against the CPU oracle. Needs an MI355X (-m gpu)."""
import numpy as np
import pytest

import floxer_amd as F
import oracle_lib as O
import ordered_corpus as OC
import search_corpus as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts():
    """text name -> context"""
    ctxs = {text: F.context(F.fmindex(OC.text_refs(text))) for text in ("own", "search")}
    yield ctxs
    for ctx in ctxs.values():
        ctx.close()


@pytest.fixture(scope="module")
def reads_ctx():
    R = OC.reads()
    ctx = F.context(F.fmindex(R.genome))
    yield R, ctx
    ctx.close()


def _ctx_of(contexts, launch):
    return contexts[OC.build().launches[launch].text]


def _by_seed(got, n):
    out = [[] for _ in range(n)]
    for i, lb, ln, e in got.tolist():
        out[i].append([lb, ln, e])
    return out


def _search_seeds(ctx, launch, cfg):
    """(anchors, stats, search counters) of one call"""
    pool, seeds = OC.launch_seeds(launch)
    ctx.path_counters(reset=True)
    a, s = F.searcher(ctx, cfg).search_seeds(pool, seeds)
    return a.tolist(), s.tolist(), ctx.search_counters()


# ------------------------------------------------------------------------------------------------ 1. raw emission
RAW_LAUNCHES = list(OC.LAUNCHES) + ["sc_short", "sc_long", "sc_heavy"]


@pytest.mark.parametrize("launch", RAW_LAUNCHES)
def test_raw_emission_matches_oracle(contexts, monkeypatch, launch):
    """the raw hook without FLX_FM_KEYED_RAW is the ordered walk and the host's grouping of its slots: every seed's groups in the order
    and with the truncation of the oracle's search_n, under every cap of the launch"""
    monkeypatch.delenv("FLX_FM_KEYED_RAW", raising=False)
    if launch.startswith("sc_"):
        ctx, caps = contexts["search"], OC.CAPS
        pool, seeds = SC.launch_seeds(launch[3:])
        names = [SC.build().cases[i].name for i in SC.build().launches[launch[3:]]]
        oidx = SC.oracle_index()
        expect = lambda cap: [oidx.search_groups(pool[off:off + ln], k, n=cap)[0] for off, ln, k, _ in seeds]
    else:
        ctx, caps = _ctx_of(contexts, launch), OC.build().launches[launch].caps
        pool, seeds = OC.launch_seeds(launch)
        names = [x.name for x in OC.launch_cases(launch)]
        expect = lambda cap: [g for g, _ in OC.groups(launch, cap)]
    for cap in caps:
        exp = [g.tolist() for g in expect(cap)]
        ctx.path_counters(reset=True)
        got = _by_seed(F.searcher(ctx).search_groups(pool, seeds, max_hits=cap), len(seeds))
        sc = ctx.search_counters()
        print(f"{launch} max_hits {cap}: seeds {len(seeds)}, groups {sum(len(g) for g in got)}, search counters {sc}")
        for at, name in enumerate(names):
            assert got[at] == exp[at], (launch, cap, name)
        assert sc["launches"] >= 1 and sc["subtrees_queued"] == 0


# ------------------------------------------------------------------------------------------------ 2. device selection behind the ordered walk
DEVICE_LAUNCHES = OC.launches_of("slots", "cap")


@pytest.mark.parametrize("hard,soft", OC.CONFIGS)
def test_device_selection_behind_the_ordered_walk_on_the_search_corpus(contexts, monkeypatch, hard, soft):
    """FLX_FM_ORDERED=1 puts the ordered walk in front of the device selection: its hits carry their ordinal above the error count and
    hit_scatter_kernel places them by it. The default walk queues a subtree for every one-row start the search corpus promises; the
    ordered walk queues none."""
    ctx = contexts["search"]
    monkeypatch.setenv("FLX_FM_ORDERED", "1")
    c = SC.build()
    cfg = F.search_config(hard, soft, "count_first", "round_robin", True)
    for launch in c.launches:
        pool, seeds = SC.launch_seeds(launch)
        exp_a, exp_s = SC.expected(launch, hard, soft)
        ctx.path_counters(reset=True)
        before = ctx.search_counters()["launches"]
        got_a, got_s = F.searcher(ctx, cfg).search_seeds(pool, seeds)
        sc = ctx.search_counters()
        print(f"{launch} hard {hard} soft {soft}, ordered: anchors {len(got_a)}, search counters {sc}, path counters seeds_selected_on_host {ctx.path_counters()['seeds_selected_on_host']}")
        assert got_s.tolist() == exp_s.tolist(), launch
        assert got_a.tolist() == exp_a.tolist(), launch
        assert sc["subtrees_queued"] == 0 and sc["launches"] > before
        if launch != "heavy":
            assert sum(c.cases[i].props["one_row_starts"] for i in c.launches[launch]) > 0


@pytest.mark.parametrize("hard,soft", OC.CONFIGS + [(2000, 50)])
@pytest.mark.parametrize("launch", DEVICE_LAUNCHES)
def test_device_selection_behind_the_ordered_walk(contexts, monkeypatch, launch, hard, soft):
    """the slots and cap launches through the ordered walk and the device selection (hard cap 2000: more than 1000 hits of a seed are
    scattered by their ordinals, and a seed of more than 512 groups goes on to the host in the order the scatter left)"""
    ctx = _ctx_of(contexts, launch)
    monkeypatch.setenv("FLX_FM_ORDERED", "1")
    exp_a, exp_s = OC.expected(launch, hard, soft)
    before = ctx.search_counters()["launches"]
    got_a, got_s, sc = _search_seeds(ctx, launch, F.search_config(hard, soft, "count_first", "round_robin", True))
    print(f"{launch} hard {hard} soft {soft}, ordered: anchors {len(got_a)}, search counters {sc}")
    assert got_s == exp_s.tolist()
    assert got_a == exp_a.tolist()
    assert sc["subtrees_queued"] == 0 and sc["launches"] >= 1


# ------------------------------------------------------------------------------------------------ 3. host selection behind the ordered walk
HOST_CONFIGS = [("count_first", "first_reported", 500, 1), ("count_first", "first_reported", 500, 3), ("count_first", "first_reported", 500, 50),
                ("count_first", "full_groups", 500, 50), ("count_first", "full_groups", 60, 7), ("errors_first", "round_robin", 500, 50),
                ("errors_first", "round_robin", 60, 7), ("none", "round_robin", 500, 50), ("none", "full_groups", 5, 3)]


@pytest.mark.parametrize("order,choice,hard,soft", HOST_CONFIGS, ids=lambda v: str(v))
def test_host_selection_behind_the_ordered_walk(contexts, monkeypatch, order, choice, hard, soft):
    """first_reported is the ordered walk by itself (its cap on a seed's rows is the soft cap); the other orders and choices are selected
    on the host and get the ordered walk from FLX_FM_ORDERED=1"""
    if choice != "first_reported":
        monkeypatch.setenv("FLX_FM_ORDERED", "1")
    for launch in DEVICE_LAUNCHES:
        ctx = _ctx_of(contexts, launch)
        exp_a, exp_s = OC.expected(launch, hard, soft, order, choice)
        got_a, got_s, sc = _search_seeds(ctx, launch, F.search_config(hard, soft, order, choice, True))
        print(f"{launch} {order} {choice} hard {hard} soft {soft}: anchors {len(got_a)}, search counters {sc}")
        assert got_s == exp_s.tolist(), launch
        assert got_a == exp_a.tolist(), launch
        assert sc["subtrees_queued"] == 0 and sc["launches"] >= 1


# ------------------------------------------------------------------------------------------------ 4. length
def test_long_seeds_turn_the_launch_to_the_ordered_walk(contexts, monkeypatch):
    """no variable set, the default configuration: a seed of more than 16383 symbols makes the launch the ordered walk's, seeds of
    16383 stay with the walk with keys (which queues their one-row subtrees); first_reported with a soft cap of 1 for the seeds with
    spare errors"""
    for name in ("FLX_FM_ORDERED", "FLX_FM_KEYED_RAW", "FLX_HOST_SELECT"):
        monkeypatch.delenv(name, raising=False)
    ctx = contexts["own"]
    for launch, cfg, ordered in (("length", (500, 50, "count_first", "round_robin"), True), ("length_keyed", (500, 50, "count_first", "round_robin"), False),
                                 ("length_spare", (500, 1, "count_first", "first_reported"), True)):
        exp_a, exp_s = OC.expected(launch, *cfg)
        got_a, got_s, sc = _search_seeds(ctx, launch, F.search_config(*cfg, True))
        print(f"{launch}: anchors {len(got_a)}, search counters {sc}, cursor extensions {ctx.path_counters()['cursor_extensions']}")
        assert got_s == exp_s.tolist(), launch
        assert got_a == exp_a.tolist(), launch
        assert len(got_a) == len(OC.launch_cases(launch))              # every long seed has its one anchor
        assert sc["launches"] >= 1 and (sc["subtrees_queued"] == 0) == ordered, launch


# ------------------------------------------------------------------------------------------------ 5. whole path
def _records(run):
    return run.records(), np.asarray(run.skipped).tolist()


def test_long_reads_through_the_aligner(reads_ctx, monkeypatch):
    """reads whose leaves are longer than the walk with keys takes: the chunk's search asks for the host's seed list and runs the
    ordered walk behind it, in front of the device selection"""
    R, ctx = reads_ctx
    for name in ("FLX_FM_ORDERED", "FLX_CHUNK_READS"):
        monkeypatch.delenv(name, raising=False)
    exp = R.index.run(R.reads, O.params(**OC.READ_PARAMS))
    expected = (exp.records(), exp.skipped.tolist())
    al = F.aligner(ctx, F.params(**OC.READ_PARAMS))
    ctx.path_counters(reset=True)
    got = al.align_reads(R.reads)
    sc = ctx.search_counters()
    print(f"long reads: {len(got.records())} records, search counters {sc}, path counters {ctx.path_counters()}")
    assert _records(got) == expected
    assert sc["subtrees_queued"] == 0 and sc["launches"] >= 1           # one chunk, and the ordered walk took it
    mapped = {r[0] for r in got.records() if not r[1] & 4}
    assert set(R.long) <= mapped
    rr = F.resident_reads(ctx, R.reads)
    assert _records(al.align_reads(rr)) == expected
    monkeypatch.setenv("FLX_CHUNK_READS", "3")
    assert _records(al.align_reads(rr)) == expected
    assert _records(al.align_reads(R.reads)) == expected
    monkeypatch.delenv("FLX_CHUNK_READS")
    rr.close()


def test_ordinary_reads_through_the_aligner_behind_the_ordered_walk(reads_ctx, monkeypatch):
    """the ordinary reads alone: FLX_FM_ORDERED=1 sends their chunk through the host's seed list and the ordered walk; first_reported
    and errors_first take the host selection"""
    R, ctx = reads_ctx
    monkeypatch.delenv("FLX_CHUNK_READS", raising=False)
    reads = [r for i, r in enumerate(R.reads) if i not in R.long]
    exp = R.index.run(reads, O.params(**OC.READ_PARAMS))
    expected = (exp.records(), exp.skipped.tolist())
    al = F.aligner(ctx, F.params(**OC.READ_PARAMS))
    ctx.path_counters(reset=True)
    assert _records(al.align_reads(reads)) == expected
    assert ctx.search_counters()["subtrees_queued"] > 0                 # (the default walk)
    monkeypatch.setenv("FLX_FM_ORDERED", "1")
    ctx.path_counters(reset=True)
    assert _records(al.align_reads(reads)) == expected
    sc = ctx.search_counters()
    print(f"ordinary reads, ordered: search counters {sc}")
    assert sc["subtrees_queued"] == 0 and sc["launches"] >= 1
    monkeypatch.delenv("FLX_FM_ORDERED")
    for kw, okw in ((dict(anchor_choice_strategy="first_reported"), dict(choice="first_reported")),
                    (dict(anchor_group_order="errors_first"), dict(group_order="errors_first"))):
        exp = R.index.run(reads, O.params(**OC.READ_PARAMS, **okw))
        got = F.aligner(ctx, F.params(**OC.READ_PARAMS, **kw)).align_reads(reads)
        assert _records(got) == (exp.records(), exp.skipped.tolist()), kw


# ------------------------------------------------------------------------------------------------ 6. scheduling independence
def test_the_mixed_queue_does_not_depend_on_scheduling(contexts, monkeypatch):
    """three launches in one process give lanes other seeds at other times and return the same"""
    monkeypatch.delenv("FLX_FM_KEYED_RAW", raising=False)
    ctx = contexts["own"]
    pool, seeds = OC.launch_seeds("queue_mixed")
    exp = [g.tolist() for g, _ in OC.groups("queue_mixed")]
    runs = [F.searcher(ctx).search_groups(pool, seeds, max_hits=2 ** 31).tolist() for _ in range(3)]
    assert runs[1] == runs[0] and runs[2] == runs[0]
    assert _by_seed(np.asarray(runs[0], dtype=np.uint64).reshape(-1, 4), len(seeds)) == exp
    monkeypatch.setenv("FLX_FM_ORDERED", "1")
    cfg = F.search_config(500, 50, "count_first", "round_robin", True)
    sel = [_search_seeds(ctx, "queue_mixed", cfg)[:2] for _ in range(3)]
    assert sel[1] == sel[0] and sel[2] == sel[0]
    exp_a, exp_s = OC.expected("queue_mixed", 500, 50)
    assert sel[0] == (exp_a.tolist(), exp_s.tolist())
