"""Every capped launch run past its grid, job after job (tests/stride_corpus.py; the corpus is checked by test_stride_corpus_host.py).
Behind its cap (floxer_amd.grid_caps()) a wave or a thread takes its next job in a loop; here every such loop takes a second and a
third turn on cases that leave its carries, LDS and flags in another state than the next case expects. One wave per job: 2 cap + P
jobs in one call of the kernel's own door; one wave per record: 2 (4 cap) + P counted records in one add_records call; one thread
per key: the sorter and the sv object past 256 cap elements. Every comparison is exact. Each test asserts, from the kernel accounting or
from the object's own counts, that one launch held more work than its grid, and prints its wall time.

cigar_realign is absent: RealignPass::cut gives a launch at most 4096 jobs, below its grid cap, so its job loop takes no second turn
through any door (test_realign_gpu.py covers the cut). sv_junctions past its grid needs over four million records in split groups
and carries nothing between turns."""
import time
from collections import Counter

import numpy as np
import pytest

import floxer_amd as F
import coverage_ref
import cs_ref
import errprof_ref
import leftalign_ref as LA
import oracle_lib as O
import pileup_ref
import sort_ref
import stride_corpus as SC
import sv_ref
from test_extend_gpu import Jobs
from test_md_host import md_from_cigar
from test_tails_host import rule as tails_rule

gpu = pytest.mark.gpu
CAPS = SC.caps()
CASES = SC.path_cases()
P = len(CASES)
SV_MIN = 3


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.perf_counter()
    yield
    print(f"\n[stride corpus] {request.node.name}: {time.perf_counter() - t0:.2f} s wall")


@pytest.fixture(scope="module")
def ctx():
    c = F.context(F.fmindex([np.random.default_rng(5).integers(1, 5, size=6000, dtype=np.uint8)]))
    c.enable_kernel_timing(True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world():
    return SC.World(CASES)


def probes(n, cap):
    """an index below the cap, the cap, one behind it, the third turn's first, the last"""
    return (cap - 1, cap, cap + 1, 2 * cap, n - 1)


def check_periodic(got, want, n, cap, same=lambda g, w: g == w):
    """got[i] is want[i mod P] for every i, and explicitly around the grid's edge"""
    p = len(want)
    assert len(got) == n and n > 2 * cap
    bad = [i for i in range(n) if not same(got[i], want[i % p])]
    assert not bad, (len(bad), bad[:5], [got[i] for i in bad[:2]], [want[i % p] for i in bad[:2]])
    for i in probes(n, cap):
        assert same(got[i], want[i % p]), i


def one_launch(ctx, kernel, units=None):
    """the call made exactly one launch of the kernel (else the arena or a host cut split it and the test proved nothing)"""
    st = ctx.kernel_stats()[kernel]
    assert st["launches"] == 1, (kernel, st)
    if units is not None:
        assert st["work_units"] == units, (kernel, st)


# ------------------------------------------------------------------------------------------------ one wave per job
@gpu
@pytest.mark.parametrize("long", [False, True])
def test_cs_build_past_its_grid(ctx, long):
    cap = CAPS["cs_build"]
    n = SC.n_jobs(cap, P)
    ref_pool, q_pool, words, jobs = SC.pack_paths(CASES)
    want = [cs_ref.cs_from_cigar(c.ref, c.begin, c.qry, c.words(), long) for c in CASES]
    ctx.reset_kernel_stats()
    got = F.cs_batch(ctx, q_pool, words, SC.cycle(jobs, n), long=long, reference_pool=ref_pool)
    one_launch(ctx, "cs_build")
    check_periodic(got, want, n, cap)


@gpu
def test_cigar_left_align_past_its_grid(ctx):
    cap = CAPS["cigar_left_align"]
    n = SC.n_jobs(cap, P)
    ref_pool, q_pool, words, jobs = SC.pack_paths(CASES)
    want = [LA.words_of(LA.left_align(c.path, c.ref, c.qry, c.begin)).tobytes() for c in CASES]
    ctx.reset_kernel_stats()
    got = F.left_align_batch(ctx, q_pool, words, SC.cycle(jobs, n), reference_pool=ref_pool)
    one_launch(ctx, "cigar_left_align")
    check_periodic([g.tobytes() for g in got], want, n, cap)


@gpu
def test_cigar_tails_past_its_grid(ctx):
    cap = CAPS["cigar_tails"]
    n = SC.n_jobs(cap, P)
    _, _, words, _ = SC.pack_paths(CASES)
    tj = SC.tail_jobs(CASES)
    want = np.array([tails_rule(c.words(), j[2] or 4, j[3] or 100, j[4] or 100) for c, j in zip(CASES, tj)], dtype=np.int64)
    ctx.reset_kernel_stats()
    got = F.cigar_tails_batch(ctx, words, SC.cycle(tj, n))
    one_launch(ctx, "cigar_tails", units=n)
    assert got.shape == (n, 8) and n > 2 * cap
    bad = np.nonzero((got != np.tile(want, (n // P + 1, 1))[:n]).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:2]].tolist())
    for i in probes(n, cap):
        assert got[i].tolist() == want[i % P].tolist(), i


@gpu
def test_ed_extend_past_its_grid(ctx):
    cap = CAPS["ed_extend"]
    cases = SC.extend_cases()
    p = len(cases)
    n = SC.n_jobs(cap, p)
    J = Jobs()
    for name, q, t, direction, kw in cases:
        J.add(name, q, t, direction, **kw)                               # (the expected numbers: the rule of test_extend_host.py)
    want = np.array(J.want, dtype=np.int64)
    ctx.reset_kernel_stats()
    got = F.extend_batch(ctx, np.concatenate(J.q), SC.cycle(J.jobs, n), reference_pool=np.concatenate(J.t))
    one_launch(ctx, "ed_extend")
    assert got.shape == (n, 4) and n > 2 * cap
    bad = np.nonzero((got != np.tile(want, (n // p + 1, 1))[:n]).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:2]].tolist(), [J.names[i % p] for i in bad[:2]])
    for i in probes(n, cap):
        assert got[i].tolist() == want[i % p].tolist(), (i, J.names[i % p])


def oracle_paths(cases):
    """(nm, begin, path) of every align case from the oracle"""
    out = []
    for name, w, q, k in cases:
        nm, begin, cigar = O.align(w, q, k)[:3]
        out.append((nm, begin, LA.parse(cigar)))
    return out


@gpu
def test_md_build_past_its_grid(ctx):
    cap = CAPS["md_build"]
    cases = SC.align_cases()
    n = SC.n_jobs(cap, len(cases))
    ref_pool, q_pool, jobs = SC.tile_align_jobs(cases, n)
    want = [(nm, begin, LA.show(path), md_from_cigar(w, begin, LA.words_of(path))) for (nm, begin, path), (_, w, q, k) in zip(oracle_paths(cases), cases)]
    ctx.reset_kernel_stats()
    got = F.align_batch(ctx, q_pool, jobs, reference_pool=ref_pool, md=True)
    one_launch(ctx, "md_build", units=n)
    one_launch(ctx, "ed_traceback")
    check_periodic(got, want, n, cap)


@gpu
def test_left_align_md_and_cs_behind_the_traceback_past_their_grids(ctx):
    """cigar_left_align rewrites the DevTraceOuts that md_build and cs_build then read, all three past their grids in one call"""
    cap = max(CAPS["cigar_left_align"], CAPS["md_build"], CAPS["cs_build"])
    cases = SC.align_cases()
    n = SC.n_jobs(cap, len(cases))
    ref_pool, q_pool, jobs = SC.tile_align_jobs(cases, n)
    want = []
    for (nm, begin, path), (_, w, q, k) in zip(oracle_paths(cases), cases):
        moved = LA.left_align(path, w, q, begin)
        words = LA.words_of(moved)
        want.append((nm, begin, LA.show(moved), md_from_cigar(w, begin, words), cs_ref.cs_from_cigar(w, begin, q, words, False)))
    ctx.reset_kernel_stats()
    got = F.align_batch_cs(ctx, q_pool, jobs, F.cs_options(long=False), reference_pool=ref_pool, md=True, gaps=F.gap_options())
    for kernel in ("cigar_left_align", "cs_build"):
        one_launch(ctx, kernel)
    one_launch(ctx, "md_build", units=n)
    check_periodic([(g[0], g[1], g[2], g[3], g[5]) for g in got], want, n, cap)


# ------------------------------------------------------------------------------------------------ one wave per record
def summed(per_case, n, period):
    """the expected table of an additive object: multiplicity times the reference's table of each case, in exact integers"""
    return sum(m * np.asarray(t, dtype=np.int64) for m, t in zip(SC.multiplicity(n, period), per_case))


@gpu
def test_coverage_add_past_its_grid(world):
    cap = CAPS["coverage_add"]
    n = SC.n_jobs(cap, P, 4)
    o = coverage_ref.options(count_deletions=True)
    want = summed([coverage_ref.depth(world.lengths, world.rec[c: c + 1], world.words, o) for c in range(P)], n, P)
    cov = F.coverage(lengths=world.lengths, options=coverage_ref.c_options(o))
    cov.add_records(world.records(n), world.words)                       # one call: one launch over n jobs, every record counts
    cov.finish()
    got = np.concatenate([cov.depth(r, 0, world.lengths[r]) for r in range(2)])
    win = cov.windows(0)
    cov.close()
    assert n > 2 * 4 * cap and int(win["depth_sum"].sum()) == int(want.sum()) == sum(m * sum(ln for op, ln in c.path if op != SC.INS) for m, c in zip(SC.multiplicity(n, P), CASES))
    assert (got.astype(np.int64) == want).all(), np.nonzero(got != want)[0][:10]


@gpu
def test_pileup_add_past_its_grid(world):
    cap = CAPS["pileup_add"]
    n = SC.n_jobs(cap, P, 4)
    o = pileup_ref.options()
    want = summed([pileup_ref.counts(world.lengths, world.rec[c: c + 1], world.words, world.reads, o) for c in range(P)], n, P)
    pile = F.pileup(lengths=world.lengths, options=pileup_ref.c_options(o))
    pile.add_records(world.records(n), world.words, world.reads)
    pile.finish()
    got = np.concatenate([pile.counts(r, 0, world.lengths[r]) for r in range(2)], axis=1)
    pile.close()
    assert n > 2 * 4 * cap and int(got[pileup_ref.DEPTH].sum()) == sum(m * sum(ln for op, ln in c.path if op in (SC.EQ, SC.X)) for m, c in zip(SC.multiplicity(n, P), CASES))
    assert (got.astype(np.int64) == want).all(), np.argwhere(got != want)[:10]


@gpu
def test_errprof_add_past_its_grid(world):
    cap = CAPS["errprof_add"]                                            # the small one
    n = SC.n_jobs(cap, P, 4)
    o = errprof_ref.options()
    want = errprof_ref.empty()
    for m, c in zip(SC.multiplicity(n, P), range(P)):
        want = errprof_ref.plus(want, errprof_ref.times(errprof_ref.table(world.concat, world.lengths, world.rec[c: c + 1], world.words, world.reads, o), m))
    for flush in (0, 300):                                               # a wave's sums flushed at the end only, and between the records of its turns
        prof = F.errprof(text=world.text, options=errprof_ref.c_options(o, flush_threshold=flush))
        prof.add_records(world.records(n), world.words, world.reads)
        got = prof.table()
        prof.close()
        assert n > 2 * 4 * cap and int(got["TOTALS"][0]) == n            # every record of the one launch was walked
        assert not errprof_ref.same(got, want), (flush, errprof_ref.same(got, want)[:10])


@gpu
def test_sv_extract_past_its_grid():
    cap = CAPS["sv_extract"]
    cases = SC.sv_cases(CASES, SV_MIN)
    p = len(cases)
    w = SC.World(cases)
    n = SC.n_jobs(cap, p, 4)
    o = sv_ref.options(min_length=SV_MIN, max_distance=2, min_support=1)
    count = Counter()
    for m, c in zip(SC.multiplicity(n, p), range(p)):
        sigs = sv_ref.signatures(w.rec[c: c + 1], w.words, w.read_lengths, o)
        assert sigs                                                      # every record carries a qualifying word
        for s in sigs:
            count[s] += m
    uniq = sorted(count)
    obj = F.sv(lengths=w.lengths, options=sv_ref.c_options(o))
    obj.add_records(w.records(n), w.words, w.read_lengths)
    obj.finish()
    got, got_clusters = obj.signatures(), obj.clusters()
    obj.close()
    assert n > 2 * 4 * cap and len(got) == sum(count.values()) >= n      # at least one signature from every record of the one launch
    assert got.tobytes() == np.repeat(sv_ref.signature_array(uniq), [count[s] for s in uniq]).tobytes()
    want_clusters = sv_ref.cluster_array(sv_ref.clusters([s for s in uniq for _ in range(count[s])], o))
    assert got_clusters.tobytes() == want_clusters.tobytes()


def check_sorter(rec, words, n, first_ordinal=7):
    ordinals = np.arange(n, dtype=np.uint64) + first_ordinal
    sorter = F.record_sorter(2)
    order = sorter.add_records(rec, words, first_ordinal)                # one call: one sort_keys_add launch over n records
    assert len(sorter) == n
    sorter.finish()
    got = sorter.entries()
    sorter.close()
    want = sort_ref.entries(rec, words, ordinals)                        # (equal keys in ordinal order: the tie-break is part of the key)
    assert got.tobytes() == want.tobytes(), np.nonzero(got != want)[0][:10]
    assert (order == sort_ref.order(rec, ordinals)).all()
    return got


@gpu
def test_sort_keys_add_past_its_grid(world):
    cap = CAPS["sort_keys_add"]
    n = SC.n_jobs(cap, P, 4)
    got = check_sorter(world.records(n), world.words, n)
    assert n > 2 * 4 * cap and len(np.unique(got[["ref", "pos", "flag"]])) == P      # many equal keys


# ------------------------------------------------------------------------------------------------ one thread per key
@gpu
@pytest.mark.parametrize("which", ["one_more", "two_turns_and_300"])
def test_sort_census_past_its_grid(world, which):
    cap = CAPS["sort_census"]
    n = cap * 256 + 1 if which == "one_more" else 2 * cap * 256 + 300
    check_sorter(world.records(n), world.words, n)


@gpu
def test_sort_iota_and_entries_past_their_grids(world):
    n = CAPS["sort_strided"] * 256 + 300
    got = check_sorter(world.records(n), world.words, n)
    assert len(got) == n > CAPS["sort_strided"] * 256


@gpu
def test_sv_finish_past_its_grids():
    """sv_coarse_flags, sv_regroup, sv_fine_flags, sv_cluster_heads, sv_cluster_bounds and sv_signatures over 256 cap + 300 signatures (the
    sort's sort_iota and sort_entries under them): clusters of 1, 2, 7, 40, 2000 and 2148 members, the last one across element 256 cap, so
    that the second round's first waves hold one cluster and a later one several (the two branches of sv_cluster_bounds)"""
    edge = CAPS["sv_strided"] * 256
    n = edge + 300
    distinct, rec, words, read_lengths = SC.sv_big_records(n)
    o = sv_ref.options(**SC.SV_BIG)
    first = np.concatenate([[0], np.cumsum([c for _, _, c in distinct])])[:-1]
    count = Counter()
    for (pos, ws, copies), at in zip(distinct, first):
        for s in sv_ref.signatures(rec[at: at + 1], words, read_lengths, o):
            count[s] += copies
    uniq = sorted(count)
    obj = F.sv(lengths=SC.SV_BIG_LENGTHS, options=sv_ref.c_options(o))
    obj.add_records(rec, words, read_lengths)
    obj.finish()
    got, got_clusters = obj.signatures(), obj.clusters()
    obj.close()
    assert len(got) == n == sum(count.values()) and n > edge
    assert got.tobytes() == np.repeat(sv_ref.signature_array(uniq), [count[s] for s in uniq]).tobytes()
    want = sv_ref.clusters([s for s in uniq for _ in range(count[s])], o)
    assert {1, 2, 7, 40, 2000} <= {c[3] for c in want} and max(c[3] for c in want) == n - (2000 + 40 + 7) * 2048 - 200
    assert got_clusters.tobytes() == sv_ref.cluster_array(want).tobytes()
