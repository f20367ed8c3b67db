"""Mapping quality on the GPU path (flx_output_options.mapq, CLI -Q). The expected values are the plain-Python restatement of the rule
(tests/test_mapq_host.py) applied to the oracle's records for the same reads, never to the product's own. Needs an MI355X (-m gpu)."""
import os
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import simulate as S
import oracle_lib as O
from test_mapq_host import loci_per_read, restate_mapq
from test_output_options_host import restate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 0.04            # the error budget of the runs
READ_RATE = 0.03       # the reads' own errors: below the budget, so that a copy with a few edits more is still within it
FIELDS = ["read", "flag", "ref", "pos", "nm", "coff", "clen"]


def _planted():
    """a uniform text of two sequences with planted repeats: segment A once more (exact), segment B twice more (exact), segment C once
    more with six mismatches; and reads of A, B, C and of the whole text: reads with one, two and three loci, ties and near ties"""
    rng = np.random.default_rng(17)
    chroms = [c.copy() for c in S.make_genome(400_000, 2, seed=16)]
    a, b, c = (chroms[0][s:s + 3000].copy() for s in (50_000, 120_000, 200_000))
    chroms[1][30_000:33_000] = a
    chroms[1][90_000:93_000] = b
    chroms[0][300_000:303_000] = b
    c2 = c.copy()
    for p in rng.choice(len(c2), size=6, replace=False):
        c2[p] = c2[p] % 4 + 1
    chroms[1][250_000:253_000] = c2
    reads = []
    for seg, seed in [(a, 1), (b, 2), (c, 3), (c2, 4)]:
        reads += S.make_reads([seg], 10, 2000, READ_RATE, seed=100 + seed)[0]
    reads += S.make_reads(chroms, 20, 2000, READ_RATE, seed=105)[0]
    reads += [np.zeros(0, np.uint8), np.array([1, 2, 3], np.uint8), rng.integers(1, 5, size=2000, dtype=np.uint8)]   # skipped, skipped, unmapped
    return chroms, reads


@pytest.fixture(scope="module")
def planted():
    chroms, reads = _planted()
    idx = F.fmindex(chroms)
    ctx = F.context(idx)
    yield chroms, reads, ctx, O.Index(chroms)
    ctx.close()


def _same_but_reserved(a, b):
    assert len(a.raw) == len(b.raw)
    for f in FIELDS:
        assert (a.raw[f] == b.raw[f]).all(), f
    assert (a.cigars == b.cigars).all() and a.skipped.tolist() == b.skipped.tolist()


@pytest.mark.parametrize("kw,okw", [(dict(), dict()), (dict(interval_optimization=True), dict(interval_opt=True)),
                                     (dict(without_cigar=True), dict(without_cigar=True))])
def test_mapq_is_the_rule_on_the_oracles_records(planted, kw, okw):
    chroms, reads, ctx, oidx = planted
    lens = [len(r) for r in reads]
    exp = oidx.run(reads, O.params(error_probability=RATE, **okw), threads=8)
    rows = exp.records()
    want = restate_mapq(rows, lens)
    # not vacuous: reads with one, two and three or more loci, and the qualities that go with them
    n_loci = loci_per_read(rows, lens)
    for cls in (lambda n: n == 1, lambda n: n == 2, lambda n: n >= 3):
        assert sum(1 for n in n_loci.values() if cls(n)) >= 5
    prim = {w for w, r in zip(want, rows) if not r[1] & (4 | 256)}
    assert {60, 3, 2} <= prim and any(10 <= q <= 50 for q in prim)
    assert any(r[1] & 4 for r in rows)

    p = F.params(error_probability=RATE, **kw)
    plain = F.aligner(ctx, p).align_reads(reads)
    assert plain.records() == rows and not plain.mapq.any()
    assert not F.aligner(ctx, p, F.output_options(True, 1)).align_reads(reads).mapq.any()       # options without mapq: 0 as before
    got = F.aligner(ctx, p, F.output_options(mapq=True)).align_reads(reads)
    _same_but_reserved(got, plain)                                       # no field but `reserved` changes
    assert got.mapq.tolist() == want
    assert F.assign_mapq(plain, lens).tolist() == want                   # the host helper on the product's records: the same
    # with -D -N 1 the kept primary carries the quality the rule gives it on the full record set
    for drop, cap in [(True, 1), (True, 0), (False, 2)]:
        keep = restate(rows, drop, cap)
        sel = F.aligner(ctx, p, F.output_options(drop, cap, True)).align_reads(reads)
        assert sel.records() == [r for r, k in zip(rows, keep) if k], (drop, cap)
        assert sel.mapq.tolist() == [w for w, k in zip(want, keep) if k], (drop, cap)
        _same_but_reserved(sel, F.aligner(ctx, p, F.output_options(drop, cap)).align_reads(reads))
    one = F.aligner(ctx, p, F.output_options(True, 1, True)).align_reads(reads)
    assert all(not r[1] & 256 for r in one.records())
    assert {int(q) for q in one.mapq} >= {60, 3, 2, 0}


def test_resident_host_and_batched_reads_give_the_same_mapqs(planted, monkeypatch):
    chroms, reads, ctx, oidx = planted
    reads = reads + S.make_reads(chroms, 140, 1500, READ_RATE, seed=55)[0]
    p = F.params(error_probability=RATE)
    want = restate_mapq(oidx.run(reads, O.params(error_probability=RATE), threads=8).records(), [len(r) for r in reads])
    for opt in [F.output_options(mapq=True), F.output_options(True, 1, True)]:
        al = F.aligner(ctx, p, opt)
        host = al.align_reads(reads)
        if not opt.drop_duplicates:
            assert host.mapq.tolist() == want
        rr = F.resident_reads(ctx, reads)
        resident = al.align_reads(rr)
        rr.close()
        assert resident.mapq.tolist() == host.mapq.tolist() and resident.records() == host.records()
        for batch in (70, 33):
            mq, recs = [], []
            for lo in range(0, len(reads), batch):
                part = al.align_reads(reads[lo:lo + batch])
                mq += part.mapq.tolist()
                recs += [(r[0] + lo,) + r[1:] for r in part.records()]
            assert mq == host.mapq.tolist() and recs == host.records(), batch
        monkeypatch.setenv("FLX_CHUNK_READS", "9")          # many chunks over the context's lanes
        chunked = al.align_reads(reads)
        monkeypatch.delenv("FLX_CHUNK_READS")
        assert chunked.mapq.tolist() == host.mapq.tolist() and chunked.records() == host.records()


def test_counters_do_not_change_with_mapq(planted):
    chroms, reads, ctx, _ = planted
    p = F.params(error_probability=RATE)
    out = []
    for opt in (None, F.output_options(mapq=True)):
        c = F.context(F.fmindex(chroms))
        F.aligner(c, p, opt).align_reads(reads)
        out.append(c.path_counters())
        c.close()
    assert out[0] == out[1] and out[1]["records_dropped"] == 0


def test_cli_mapping_quality_end_to_end(tmp_path):
    """the whole program on the golden inputs (the flags of test_cli_whole_program): without -Q the SAM is, byte for byte, the oracle's
    records in floxer's SAM form with MAPQ 255; with -Q only column 5 differs and is the rule on the oracle's records"""
    from test_oracle_pins import _read_fasta, _read_fastq
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    refs = _read_fasta(os.path.join(g, "reference.fasta"))
    reads = _read_fastq(os.path.join(g, "queries.fastq"))
    rows = O.Index([O.chars_to_ranks(s) for _, s in refs]).run([O.chars_to_ranks(s) for _, s, _ in reads],
                                                               O.params(query_errors=2, seed_errors=1, extra_ratio=2.0, interval_opt=True)).records()
    want = restate_mapq(rows, [len(s) for _, s, _ in reads])
    assert len(set(want)) >= 2

    def expected(mapqs):
        text = "@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{name.split(' ')[0]}\tLN:{len(s)}\n" for name, s in refs)
        for (read, flag, ref, pos, nm, cig), q in zip(rows, mapqs):
            name, seq, qual = reads[read]
            with_seq = flag & 4 or not flag & 256
            text += "\t".join([name.split(" ")[0], str(flag), "*" if flag & 4 else refs[ref][0].split(" ")[0], str(pos + 1), str(q), cig or "*",
                               "*", "0", "0", seq if with_seq else "*", qual if with_seq else "*"] + ([] if flag & 4 else [f"NM:i:{nm}"])) + "\n"
        return text

    def run(out, *extra):
        cmd = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"), "--output", out,
               "--interval-optimization", "--query-errors", "2", "--seed-errors", "1", "--extra-verification-ratio", "2", "--threads", "1", *extra]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
        return open(out).read()

    assert run(str(tmp_path / "plain.sam")) == expected([255] * len(rows))
    assert run(str(tmp_path / "q.sam"), "-Q") == expected(want)
    assert run(str(tmp_path / "q2.sam"), "--mapping-quality", "--devices", "0,0") == expected(want)
    keep = restate(rows, True, 1)
    kept = run(str(tmp_path / "q1.sam"), "-D", "-N", "1", "-Q").splitlines()[1 + len(refs):]
    assert kept == [l for l, k in zip(expected(want).splitlines()[1 + len(refs):], keep) if k]
