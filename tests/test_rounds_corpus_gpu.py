"""The verification rounds (flx_rounds.hip: vr2_request_kernel, vr2_apply_kernel, ed_exists_block on the rounds' job lists; the drivers
climb_on_device and climb_on_host) on the corpus of rounds_corpus.py, through the hook that runs only the climb (flx_climb_anchors):
every anchor's fate and node against a plain per-anchor climb over the CPU oracle, both drivers, the drivers' request counts against
the oracle's tests and the solo decisions the cases promise, and the device rounds' launches and job bytes (the kernel accounting of
ed_align_exists) against the rounds written again in Python. test_rounds_corpus_host.py proves the corpus's promises on the CPU.
Needs an MI355X (-m gpu)."""
import numpy as np
import pytest

import floxer_amd as F
import oracle_lib as O
import rounds_corpus as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus_ctx():
    c = RC.build()
    ctx = F.context(F.fmindex(c.refs))
    yield c, ctx
    ctx.close()


def _params(p):
    return F.params(error_probability=p.rate, seed_errors=p.seed_errors, bottom_up_pex_tree=p.bottom_up, direct_full_verification=p.direct)


def _climb(ctx, launch, host_rounds):
    """(fates, requests, launches of the existence kernel, bytes of its jobs) of one hook call"""
    L = RC.build().launches[launch]
    reads = F.resident_reads(ctx, RC.launch_reads(launch))
    ctx.enable_kernel_timing(True)
    try:
        ctx.reset_kernel_stats()
        status, node, requests = F.climb_anchors(ctx, _params(L.params), reads, RC.launch_anchors(launch), host_rounds=host_rounds)
        exists = ctx.kernel_stats().get("ed_align_exists", dict(launches=0, algorithmic_bytes=0))
    finally:
        ctx.enable_kernel_timing(False)
        reads.close()
    return list(zip(status.tolist(), node.tolist())), requests, int(exists["launches"]), int(exists["algorithmic_bytes"])


def _first_difference(launch, got, exp):
    c = RC.build()
    L = c.launches[launch]
    for a, g, e in zip(RC.launch_anchors(launch), got, exp):
        if g != e:
            return f"{L.cases[a[0]]}: anchor (orientation, leaf, reference, position) {a[1:]} got (status, node) {g}, expected {e}"
    return None


@pytest.mark.parametrize("launch", list(RC.build().launches))
def test_fates_and_requests(corpus_ctx, launch):
    """out_status / out_node of every anchor equal the plain climb's on both drivers (so the drivers equal each other). The host rounds
    request every test of the plain climb once; the device rounds request an anchor again when they test it alone, so on the isolated
    launches the difference is exactly the solo decisions the cases promise (none, or every member of the solo clusters). The device
    rounds launch the existence kernel once per round, and vr2_request_kernel sums the bytes of the jobs it writes (window columns + node
    rows): on the launches marked exact both equal the model's, which pins the job list - de-duplication, the clusters' one or two jobs,
    the members asked again alone, the windows tested twice across a tile boundary"""
    c, ctx = corpus_ctx
    L = c.launches[launch]
    exp, n_tests = RC.climb(launch)
    model = RC.model(launch)[1]
    dev, dev_requests, dev_rounds, dev_bytes = _climb(ctx, launch, False)
    host, host_requests, _, host_bytes = _climb(ctx, launch, True)
    print(f"{launch}: anchors {len(exp)}, at root {sum(f[0] for f in exp)}, oracle tests {n_tests}, requests device {dev_requests} host {host_requests}, "
          f"device rounds {dev_rounds} job bytes {dev_bytes} (host rounds' jobs {host_bytes}), model {model}")
    assert _first_difference(launch, dev, exp) is None
    assert _first_difference(launch, host, exp) is None
    assert dev == host
    assert host_requests == n_tests and dev_requests >= n_tests
    if L.isolated:
        assert dev_requests - host_requests == RC.promised(launch).get("solo_decisions", 0), launch
    if L.exact:
        assert (dev_requests, dev_rounds, dev_bytes) == (model["requests"], model["rounds"], model["job_bytes"]), launch
    if launch == "tiles_exact":
        assert model["tiled_queries"] > 0
    if launch == "all":
        assert dev_requests - host_requests >= RC.promised("solo")["solo_decisions"]


def test_invalid_anchors_are_refused(corpus_ctx):
    """before any launch: anchors out of (read, orientation) order, a leaf outside the tree, a reference outside the index, a position whose
    leaf does not lie inside the sequence, an unknown driver"""
    c, ctx = corpus_ctx
    L = c.launches["pairs"]
    p = _params(L.params)
    reads = F.resident_reads(ctx, RC.launch_reads("pairs"))
    good = RC.launch_anchors("pairs")
    n_leaves = len(RC.tree_of(c.cases[L.cases[0]].read, L.params)[1])
    r, o, l, ref, pos = good[0]
    bad = {
        "read order": [good[-1]] + good[:-1],
        "orientation order": [(r, 1, l, ref, pos), (r, 0, l, ref, pos)],
        "leaf": [(r, o, n_leaves, ref, pos)],
        "reference": [(r, o, l, len(c.refs), pos)],
        "position past the end": [(r, o, l, ref, len(c.refs[ref]))],
        "leaf over the end": [(r, o, l, ref, len(c.refs[ref]) - 5)],
        "read": [(len(L.cases), o, l, ref, pos)],
        "orientation": [(r, 2, l, ref, pos)],
    }
    try:
        for what, anchors in bad.items():
            with pytest.raises(F.FloxerError):
                F.climb_anchors(ctx, p, reads, anchors)
            print("refused:", what)
        with pytest.raises(F.FloxerError):
            F.climb_anchors(ctx, p, reads, good, host_rounds=2)
        status, node, _ = F.climb_anchors(ctx, p, reads, good)          # and the context still works
        assert list(zip(status.tolist(), node.tolist())) == RC.climb("pairs")[0]
    finally:
        reads.close()


def test_whole_runs_on_the_pairs_and_solo_reads(corpus_ctx):
    """align_reads on the reads of the pairs and solo cases, their anchors found by the real search: the oracle's records on both drivers
    (a statistics object on the context selects the host rounds); the device requests more inner tests than the host where it tests
    anchors alone"""
    c, ctx = corpus_ctx
    reads = RC.launch_reads("pairs") + RC.launch_reads("solo")
    exp = O.Index(c.refs).run(reads, O.params(error_probability=RC.MAIN.rate, seed_errors=RC.MAIN.seed_errors)).records()
    p = _params(RC.MAIN)
    ctx.path_counters(reset=True)
    got = F.aligner(ctx, p).align_reads(reads).records()
    dev_requests = ctx.path_counters()["inner_tests_requested"]
    assert got == exp
    host_ctx = F.context(ctx.index)
    stats = F.statistics("simulated").attach(host_ctx)
    try:
        got_host = F.aligner(host_ctx, p).align_reads(reads).records()
        host_requests = host_ctx.path_counters()["inner_tests_requested"]
        assert got_host == exp
        assert stats.num_queries == len(reads)
    finally:
        host_ctx.close()
    print(f"whole run: inner tests requested device {dev_requests} host {host_requests}")
    # (which anchors the search hands to the rounds is not constructed here - it selects among many hits in the tandem repeats - so no
    # count is promised; the lowest-level solo clusters need only their two seeds found, and any one undecided cluster makes this strict)
    assert dev_requests > host_requests
