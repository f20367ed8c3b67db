"""Output options on the GPU path (flx_output_options: duplicate alignments dropped, alignments per read capped). The expected records
are the oracle's uncapped records passed through a plain-Python restatement of the rule (tests/test_output_options_host.py), not the
product's own. Needs an MI355X (-m gpu)."""
import os
import subprocess
from collections import defaultdict

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import simulate as S
import oracle_lib as O
from test_output_options_host import restate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_SETS = [(True, 0), (False, 1), (False, 3), (True, 1), (True, 3)]


def restated(records, drop, cap):
    """records: [(read, flag, ref, pos, nm, cigar string)] (oracle or product, uncapped); CIGAR strings compare like their words"""
    keep = restate(records, drop, cap)
    return [r for r, k in zip(records, keep) if k]


def distinct_per_read(records):
    d = defaultdict(set)
    for r in records:
        if not r[1] & 4:
            d[r[0]].add((r[2], r[1] & 16, r[3], r[4], r[5]))
    return d


@pytest.fixture(scope="module")
def uniform():
    genome = S.make_genome(1_000_000, 3, seed=71)
    idx = F.fmindex(genome)
    ctx = F.context(idx)
    yield genome, idx, ctx, O.Index(genome)
    ctx.close()


@pytest.mark.parametrize("kw,okw", [(dict(), dict()), (dict(interval_optimization=True), dict(interval_opt=True)),
                                     (dict(without_cigar=True), dict(without_cigar=True)), (dict(seed_errors=3), dict(seed_errors=3))])
def test_options_give_the_restated_oracle_records(uniform, kw, okw):
    genome, idx, ctx, oidx = uniform
    for length, rate, n in [(8000, 0.08, 16), (5000, 0.05, 16)]:
        reads = S.make_reads(genome, n, length, rate, seed=length + n)[0] + [np.zeros(0, np.uint8), np.array([1, 2, 3], np.uint8)]
        exp = oidx.run(reads, O.params(error_probability=rate, **okw), threads=8)
        p = F.params(error_probability=rate, **kw)
        plain = F.aligner(ctx, p).align_reads(reads)
        assert plain.records() == exp.records()
        assert F.aligner(ctx, p, F.output_options()).align_reads(reads).records() == exp.records()       # zeroed options: floxer's output
        for drop, cap in OPTION_SETS:
            got = F.aligner(ctx, p, F.output_options(drop, cap)).align_reads(reads)
            assert got.skipped.tolist() == exp.skipped.tolist()
            assert got.records() == restated(exp.records(), drop, cap), (length, rate, drop, cap)
            # the run's CIGAR pool holds the kept records' words only, and no record points outside it
            used = np.zeros(len(got.cigars), dtype=bool)
            for r in got.rows:
                assert r[5] + r[6] <= len(got.cigars)
                used[r[5]: r[5] + r[6]] = True
            assert used.all()
        if not kw:
            assert len(exp.records()) > 3 * n           # copies of each alignment: the options have something to drop


def _repeat_rich_text():
    """make_genome_fast's repeat-rich text with five diverged copies (0.4 .. 2 % mismatches) of one 4-kb segment: a read of the segment
    has six loci with six edit distances"""
    rng = np.random.default_rng(90)
    _, chroms = S.make_genome_fast(1_000_000, 2, seed=77, repeat_rich=True)
    chroms = [c.copy() for c in chroms]
    seg = chroms[0][200_000:204_000].copy()
    for i, div in enumerate([0.004, 0.008, 0.012, 0.016, 0.02]):
        c = seg.copy()
        pos = rng.choice(len(c), size=int(div * len(c)), replace=False)
        c[pos] = (c[pos] % 4) + 1
        at = 400_000 + 120_000 * i
        chroms[i % 2][at:at + len(c)] = c
    reads = S.make_reads([seg], 30, 2000, 0.03, seed=91)[0] + S.make_reads(chroms, 30, 2000, 0.05, seed=92)[0]
    return chroms, reads


def test_cap_selects_among_distinct_alignments_on_repeat_rich_text():
    chroms, reads = _repeat_rich_text()
    idx = F.fmindex(chroms)
    ctx = F.context(idx)
    oidx = O.Index(chroms, imported=(idx.suffix_array_u32(), idx.bwt(False), idx.bwt(True)))
    for kw, okw in [(dict(), dict()), (dict(interval_optimization=True), dict(interval_opt=True))]:
        exp = oidx.run(reads, O.params(error_probability=0.05, **okw), threads=8)
        d = distinct_per_read(exp.records())
        # not vacuous: reads with more distinct alignments than the cap, of several edit distances
        assert sum(1 for v in d.values() if len(v) > 3 and len({x[3] for x in v}) >= 2) >= 10
        p = F.params(error_probability=0.05, **kw)
        for drop, cap in OPTION_SETS:
            got = F.aligner(ctx, p, F.output_options(drop, cap)).align_reads(reads)
            assert got.records() == restated(exp.records(), drop, cap), (kw, drop, cap)
        # with both options, a read with six loci keeps its three best, one record each
        got = F.aligner(ctx, p, F.output_options(True, 3)).align_reads(reads).records()
        for read, v in d.items():
            if len(v) >= 6:
                assert sorted(r[4] for r in got if r[0] == read) == sorted(x[3] for x in v)[:3], read
    ctx.close()


def _words(run):
    return [r[:5] + (run.cigars[r[5]: r[5] + r[6]].tobytes(),) for r in (tuple(int(x) for x in row) for row in run.rows)]


def test_resident_host_and_batched_reads_give_the_same_runs(uniform, monkeypatch):
    genome, idx, ctx, oidx = uniform
    reads = S.make_reads(genome, 200, 2500, 0.07, seed=55)[0]
    p = F.params(error_probability=0.07)
    for drop, cap in [(True, 0), (True, 2), (False, 1)]:
        al = F.aligner(ctx, p, F.output_options(drop, cap))
        host = al.align_reads(reads)
        rr = F.resident_reads(ctx, reads)
        resident = al.align_reads(rr)
        rr.close()
        assert _words(resident) == _words(host)
        batched = []
        for lo in range(0, len(reads), 70):
            part = al.align_reads(reads[lo:lo + 70])
            batched += [(r[0] + lo,) + r[1:] for r in _words(part)]
        assert batched == _words(host)
        monkeypatch.setenv("FLX_CHUNK_READS", "9")          # many chunks over the context's lanes
        assert _words(al.align_reads(reads)) == _words(host)
        monkeypatch.delenv("FLX_CHUNK_READS")
        assert host.records() == restated(oidx.run(reads, O.params(error_probability=0.07), threads=8).records(), drop, cap)


def test_statistics_and_found_counters_do_not_change(uniform):
    """--stats and root_alignments_found describe what verification found; records counts what is written, records_dropped the rest"""
    from test_gpu_parity import _parse_stats_toml
    genome, idx, _, _ = uniform
    reads = S.make_reads(genome, 30, 5000, 0.06, seed=57)[0]
    p = F.params(error_probability=0.06)
    out = {}
    for name, opt in [("plain", None), ("options", F.output_options(True, 2))]:
        ctx = F.context(idx)
        st = F.statistics("simulated").attach(ctx)
        run = F.aligner(ctx, p, opt).align_reads(reads)
        out[name] = (_parse_stats_toml(st.format(toml=True)), ctx.path_counters(), run.n_records)
        ctx.close()
    (ts, pc, n), (ts2, pc2, n2) = out["plain"], out["options"]
    for sec in ts:
        if sec.startswith("milliseconds_spent_in_"):             # wall-clock values
            continue
        assert ts[sec] == ts2[sec], sec
    assert len(ts) >= 17 and ts["alignments_per_query"]["num_values"] == 30
    assert pc["records"] == n and pc["records_dropped"] == 0
    assert pc2["records"] == n2 and n2 < n
    assert pc["records"] - pc2["records"] == pc2["records_dropped"]
    for k in pc:
        if k not in ("records", "records_dropped"):
            assert pc[k] == pc2[k], k


def test_cli_output_options_one_and_two_device_contexts(tmp_path):
    exe, sim = os.path.join(ROOT, "floxer_amd", "floxer"), os.path.join(ROOT, "floxer_amd", "simulated_dataset")
    fa, fq = str(tmp_path / "g.fasta"), str(tmp_path / "r.fastq")
    subprocess.run([sim, "create", "--genomes", fa, "--reads", fq, "-c", "300000", "-n", "3", "-l", "3000", "-m", "120", "-e", "0.07",
                    "-s", "8", "--revcomp-fraction", "0.5"], check=True)

    def run(out, *extra):
        cmd = [exe, "--reference", fa, "--queries", fq, "--output", out, "--error-probability", "0.07", *extra]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, FLX_BATCH_READS="32"))
        assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
        return [l for l in open(out).read().splitlines() if not l.startswith("@")]

    plain = run(str(tmp_path / "plain.sam"))
    rows = []
    for line in plain:
        f = line.split("\t")
        nm = [int(t[5:]) for t in f[11:] if t.startswith("NM:i:")]
        rows.append((f[0], int(f[1]), f[2], int(f[3]), nm[0] if nm else 0, f[5]))
    exp = [l for l, k in zip(plain, restate(rows, True, 3)) if k]
    assert len(exp) < len(plain)
    assert run(str(tmp_path / "one.sam"), "--drop-duplicate-alignments", "--max-alignments", "3") == exp
    assert run(str(tmp_path / "two.sam"), "-D", "-N", "3", "--devices", "0,0", "--threads", "3") == exp


def test_full_size_reads_keep_no_duplicates(capsys):
    """10-kb reads at 8 % on a uniform text: records per read with and without dropping duplicates (logged), and no two kept records
    of a read are duplicates"""
    pool, chroms = S.make_genome_fast(4_000_000, 2, seed=61)
    idx = F.fmindex(chroms, device=0)
    ctx = F.context(idx)
    (rp, ro), _ = S.make_reads_fast(pool, [len(c) for c in chroms], 512, 10000, 0.08, seed=62)
    p = F.params(error_probability=0.08)
    plain = F.aligner(ctx, p).align_reads((rp, ro))
    dropped = F.aligner(ctx, p, F.output_options(drop_duplicates=True)).align_reads((rp, ro))
    n_reads = len(ro) - 1
    keys = [(int(r[0]), int(r[1]) & 16, int(r[2]), int(r[3]), int(r[4]), dropped.cigars[r[5]: r[5] + r[6]].tobytes())
            for r in dropped.rows if not int(r[1]) & 4]
    assert len(keys) == len(set(keys))
    assert dropped.records() == restated(plain.records(), True, 0)
    with capsys.disabled():
        print(f"\n10 kb @ 8 %, {n_reads} reads: {plain.n_records / n_reads:.2f} records per read as floxer writes them, "
              f"{dropped.n_records / n_reads:.2f} with duplicates dropped")
    ctx.close()
