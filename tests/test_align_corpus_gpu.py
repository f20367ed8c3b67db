"""The DP and traceback kernels (ed_exists_block, ed_trace_block, ed_traceback_wave; MD: md_build) on the adversarial corpus of
align_corpus.py, bit-exact against the oracle's matrix DP (algo=0): default shapes, per-job shapes, one forced waiting shape per words-per-lane
value, MD strings, and jobs at the edges of their pools. Needs an MI355X (-m gpu)."""
import collections

import numpy as np
import pytest

import floxer_amd as F
import align_corpus as AC
from test_md_host import md_from_cigar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    idx = F.fmindex([np.random.default_rng(5).integers(1, 5, size=2000).astype(np.uint8)])
    c = F.context(idx)
    yield c
    c.close()


def _check(ctx, cases, label, modes=(0, 1, 2), tail=0):
    rpool, qpool, jobs, what = AC.batch(cases, modes, tail)
    got = F.align_batch(ctx, qpool, jobs, reference_pool=rpool)
    wrong = [(label, c.name, mode, g, AC.expected(c, mode)) for (c, mode), g in zip(what, got) if g != AC.expected(c, mode)]
    assert not wrong, (len(wrong), [(l, n, md, str(g)[:120], str(e)[:120]) for l, n, md, g, e in wrong[:8]])
    return jobs, what


def _report(label, cases, shapes):
    cls = collections.Counter(c.cls for c in cases)
    used = collections.Counter((w, r) for w, r, _ in shapes)
    print(f"[align corpus] {label}: cases {len(cases)} {dict(sorted(cls.items()))} jobs {len(shapes)} waiting {sum(1 for s in shapes if s[2] > 0)} "
          f"shapes {dict(sorted(used.items()))}")


@pytest.mark.parametrize("few_waves", [None, "0"], ids=["common_shape", "per_job_shapes"])
def test_whole_corpus_on_default_shapes(ctx, monkeypatch, few_waves):
    """the whole corpus in one call per mode: the common shape of a small batch, then (FLX_ALIGN_FEW_WAVES=0) the shapes per job, rings that
    wait among them"""
    if few_waves is not None:
        monkeypatch.setenv("FLX_ALIGN_FEW_WAVES", few_waves)
    cases = AC.whole()
    for mode in (0, 1, 2):
        jobs, _ = _check(ctx, cases, f"default mode {mode}", modes=(mode,))
        shapes = F.align_shapes(jobs)
        _report(f"default shapes ({'per job' if few_waves else 'common'}), mode {mode}", cases, shapes)
        assert (few_waves is not None) == any(q > 0 for _, _, q in shapes)


@pytest.mark.parametrize("shape", AC.SHAPES, ids=lambda s: f"{s[0]},{s[1]}")
def test_forced_waiting_shape(ctx, monkeypatch, shape):
    """one shape per words-per-lane value the kernels are instantiated for, forced on the corpus built for it: the hand-over queue in LDS
    (K3/K4) and the delayed slots of the trace (K5), all three modes"""
    W, R = shape
    monkeypatch.setenv("FLX_FORCE_SHAPE", f"{W},{R}")
    monkeypatch.setenv("FLX_ALIGN_FEW_WAVES", "0")
    cases = AC.corpus(W, R)
    for mode in (0, 1, 2):
        rpool, qpool, jobs, what = AC.batch(cases, (mode,))
        shapes = F.align_shapes(jobs)
        assert all((w, r) == (W, R) for w, r, _ in shapes)
        assert 3 * sum(1 for s in shapes if s[2] > 0) >= len(jobs)
        if mode == 2:
            _report(f"forced {W},{R}", cases, shapes)
        _check(ctx, cases, f"forced {W},{R} mode {mode}", modes=(mode,))


def test_md_strings_of_structured_paths(ctx, monkeypatch):
    """md_build on long deletion runs, ties and paths of 2 NM + 1 runs, in the shapes per job"""
    monkeypatch.setenv("FLX_ALIGN_FEW_WAVES", "0")
    cases = [c for c in AC.whole() if c.cls in ("gap", "ties", "runs")]
    rpool, qpool, jobs, what = AC.batch(cases, (2,))
    got = F.align_batch(ctx, qpool, jobs, reference_pool=rpool, md=True)
    for (c, _), g in zip(what, got):
        exp = AC.expected(c, 2)
        assert g is not None and g[:3] == exp, (c.name, str(g)[:120], str(exp)[:120])
        words = [(int(n) << 4) | "MIDNSHP=X".index(op) for n, op in AC.cigar_runs(exp[2])]
        assert g[3] == md_from_cigar(c.ref, exp[1], words), c.name


def test_jobs_at_the_edges_of_their_pools(ctx, monkeypatch):
    """a job whose query starts the query pool (the equality masks of its padded first word begin in front of the pool) and one whose window
    ends at the reference pool's last byte, each of a gap-run and a band-edge case, in a common shape and in per-job shapes"""
    by_name = {c.name: c for c in AC.whole()}
    picks = [by_name[n] for n in ("w1_gap_D129_group", "w1_band_lead_ins_k17_l0r0", "w2_gap_I65_word", "w2_band_trail_ins_k129_l0r0", "w1_gap_I513_colbegin")]
    for few in (None, "0"):
        if few:
            monkeypatch.setenv("FLX_ALIGN_FEW_WAVES", few)
        for i, first in enumerate(picks):
            last = picks[(i + 1) % len(picks)]
            _check(ctx, [first] + [p for p in picks if p is not first and p is not last] + [last], f"pool edges {first.name} .. {last.name}", tail=0)
