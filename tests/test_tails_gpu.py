"""Chimeric tails of reads mapped in full, on the GPU. The kernel alone (cigar_tails through flx_cigar_tails_batch) against the host rule
(flx_cigar_tails, itself checked against the Python rule in test_tails_host.py), all eight numbers exactly; then the pipeline in the
world of test_partial_gpu.py: reads that fit their errors in full but end in junk or in a piece of another locus are split into a
clipped primary and supplementaries, everything else stays byte for byte, off is off."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
from floxer_amd import simulate as S
import oracle_lib as O
from test_extend_gpu import check_extended, core_of, sa_strings
from test_partial_gpu import CHROM, LEN, RATE, by_read, check_record, chimera_ok, letters, make_halves, mutate, oriented, root_children, same, words_of
from test_tails_host import DEL, EQ, INS, X, Cases, edge_cases, random_cases, rule, w

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"=": EQ, "X": X, "I": INS, "D": DEL}
JUNK, FOREIGN, SPAN = 400, 650, 300                              # rows of a junk tail, of a tail from another locus, and the min_query_span it is run with


def core_words(cigar):
    return [w(n, OPS[op]) for n, op in words_of(cigar) if op != "S"]


# ------------------------------------------------------------------------------------------------ the world
def make_tailed(rng, chroms, kind):
    """a 1 %-error body and a tail that does not belong to it. kind 'right' / 'left': JUNK random rows behind / in front of the body;
    'rc': the right-tailed read reverse complemented; 'foreign': FOREIGN rows of another locus (1 % errors) behind the body.
    Returns (read, orientation of the body, chromosome, window of the whole read in the body's locus, side of the tail in that
    orientation, rows of the tail)."""
    n_tail = FOREIGN if kind == "foreign" else JUNK
    body = LEN - n_tail
    ch = int(rng.integers(0, len(chroms)))
    p = int(rng.integers(2000, CHROM // 2 - LEN))
    sa = mutate(rng, chroms[ch][p: p + body], body // 100)
    if kind == "foreign":
        cb, pb = int(rng.integers(0, len(chroms))), int(rng.integers(CHROM // 2 + 1000, CHROM - LEN - 1000))
        tail = mutate(rng, chroms[cb][pb: pb + n_tail], n_tail // 100)
    else:
        tail = rng.integers(1, 5, size=n_tail, dtype=np.uint8)
    k, _ = root_children()
    if kind == "left":
        return np.concatenate([tail, sa]), 0, ch, (p - n_tail - k, p + body + k), "left", n_tail
    read = np.concatenate([sa, tail])
    return (O.revcomp(read) if kind == "rc" else read), (1 if kind == "rc" else 0), ch, (p - k, p + LEN + k), "right", n_tail


def tail_of(numbers, side):
    """(rows of the tail on `side`, rows of the other one) of the rule's eight numbers"""
    return (numbers[4], numbers[0]) if side == "right" else (numbers[0], numbers[4])


def tailed_ok(chroms, k, made):
    """on the CPU: the whole read aligns in its body's locus within k, and the rule finds the intended tail on that alignment's CIGAR"""
    read, o, ch, (lo, hi), side, n_tail = made
    a = O.align(chroms[ch][max(0, lo): hi], oriented(read, o), k, mode=2)
    if a is None:
        return False
    rows, other = tail_of(rule(core_words(a[2])), side)
    return other == 0 and abs(rows - n_tail) <= 100


def build_batch():
    pool, chroms = S.make_genome_fast(CHROM, 2, seed=41)
    (rp, ro), _ = S.make_reads_fast(pool, [CHROM, CHROM], 6, 3000, 0.04, seed=42)
    reads = [rp[int(ro[i]): int(ro[i + 1])].copy() for i in range(6)]
    rng = np.random.default_rng(53)
    k, _ = root_children()
    tailed, rescued = {}, []

    def draw(kind):
        for _ in range(20):
            made = make_tailed(rng, chroms, kind)
            if tailed_ok(chroms, k, made):
                tailed[len(reads)] = (kind,) + made[1:]
                reads.append(made[0])
                return
        raise AssertionError(f"no {kind}-tailed read that the CPU agrees with in 20 draws")

    draw("right")
    draw("left")
    for _ in range(20):                                              # a chimera of two halves: unmapped, rescued (between the split reads)
        c = make_halves(rng, chroms, "ff", 0.5)
        if chimera_ok(chroms, k, c):
            rescued.append(len(reads))
            reads.append(c.read)
            break
    assert rescued, "no chimera that the CPU agrees with in 20 draws"
    draw("rc")
    draw("foreign")
    draw("foreign")
    reads.append(rng.integers(1, 5, size=LEN, dtype=np.uint8))      # unmapped, and no part of it aligns anywhere
    return chroms, reads, tailed, rescued


def aligner(ctx, split=None, extend=None, span=SPAN):
    return F.aligner(ctx, F.params(error_probability=RATE), F.output_options(max_alignments=1, mapq=True), md=True,
                     partial=F.partial_options(min_query_span=span), extend=extend, split=split)


@pytest.fixture(scope="module")
def world():
    chroms, reads, tailed, rescued = build_batch()
    ctx = F.context(F.fmindex(chroms))
    ctx.enable_kernel_timing(True)
    runs, stats, pcs = {}, {}, {}
    for name, split, extend in (("off", None, None), ("split", F.split_options(), None), ("off_ext", None, F.extend_options()),
                                ("split_ext", F.split_options(), F.extend_options())):
        ctx.reset_kernel_stats()
        ctx.path_counters(reset=True)
        runs[name] = aligner(ctx, split, extend).align_reads(reads)
        stats[name], pcs[name] = ctx.kernel_stats(), ctx.path_counters(reset=True)
    ctx.enable_kernel_timing(False)
    yield dict(chroms=chroms, reads=reads, tailed=tailed, rescued=rescued, ctx=ctx, runs=runs, stats=stats, pcs=pcs)
    ctx.close()


def expected_tails(w_):
    """the rule on the primary's CIGAR of the run without split: {read: eight numbers}"""
    out = {}
    rows = by_read(w_["runs"]["off"])
    for i in w_["tailed"]:
        ((_, rec),) = rows[i]
        out[i] = rule(core_words(rec[5]))
    return out


# ------------------------------------------------------------------------------------------------ the kernel alone
def pass_boundary_cases():
    c = Cases()
    rng = np.random.default_rng(19)
    for T in (1, 2, 63, 64, 65, 128, 129, 1500):
        body = [w(int(rng.integers(20, 90)), EQ) if t % 2 == 0 else w(1, (X, INS, DEL)[t % 3]) for t in range(T)]
        c.add(f"{T} words, no tail", body)
        c.add(f"{T} words, the last one a tail", body[:-1] + [w(160, X)])
        c.add(f"{T} words, the first one a tail", [w(160, INS)] + body[1:])
        c.add(f"{T} words, tails in the words at both ends", [w(160, X)] + body[1:-1] + [w(170, INS)] if T > 2 else body)
    drift = [w(1, X), w(2, EQ)] * 70
    c.add("first maximum in pass 0, the drop in the last pass", [w(500, EQ)] + drift + [w(150, X)])
    c.add("last minimum in the last pass, the drop in pass 0", [w(150, X)] + [w(2, EQ), w(1, X)] * 70 + [w(500, EQ)])
    c.add("the maximum again in pass 1: the first wins", [w(500, EQ)] + [w(1, X), w(3, EQ)] * 40 + [w(200, X)])
    c.add("the minimum already in pass 0: the last wins", [w(200, X)] + [w(3, EQ), w(1, X)] * 40 + [w(500, EQ)])
    c.add("maximum in lane 63, tail from lane 0 of the next pass", [w(10, EQ)] * 64 + [w(3, X), w(1, EQ)] * 50)
    c.add("minimum in lane 63", [w(1, EQ), w(3, X)] * 32 + [w(10, EQ)] * 100)
    c.add("both tails, three passes", [w(120, X)] + [w(40, EQ), w(1, DEL)] * 80 + [w(40, EQ), w(130, INS), w(3, EQ)])
    return c


@gpu
def test_kernel_matches_the_host_rule_on_edge_cases_and_pass_boundaries(world):
    ctx = world["ctx"]
    for c in (edge_cases(), pass_boundary_cases()):
        host = F.cigar_tails(c.words, c.jobs)
        res = c.check(host)                                          # the host rule is the Python rule
        got = F.cigar_tails_batch(ctx, c.words, c.jobs)
        for name, g, e in zip(c.names, got.tolist(), host.tolist()):
            assert g == e, (name, g, e)
    # not vacuous: what the cases are about did happen
    assert res["first maximum in pass 0, the drop in the last pass"][4:] == [150 + 210, 150 + 210, 150 + 70, 141]
    assert res["last minimum in the last pass, the drop in pass 0"][:4] == [150 + 210, 150 + 210, 150 + 70, 141]
    assert res["the maximum again in pass 1: the first wins"][7] == 81 and res["the minimum already in pass 0: the last wins"][3] == 81
    assert res["maximum in lane 63, tail from lane 0 of the next pass"][4:] == [200, 200, 150, 100] and res["minimum in lane 63"][:4] == [128, 128, 96, 64]
    assert res["1500 words, tails in the words at both ends"][3] == 2 and res["1500 words, tails in the words at both ends"][7] == 1
    assert res["both tails, three passes"][3] == 1 and res["both tails, three passes"][7] == 2


@gpu
def test_kernel_300_random_jobs_in_one_launch_and_bad_jobs_launch_nothing(world):
    ctx = world["ctx"]
    c = random_cases(23, 300, 300)
    rng = np.random.default_rng(24)
    for n in (700, 1100, 2000):                                       # a few long ones among them
        words = [w(int(rng.integers(1, 60)), EQ) if t % 2 == 0 else w(int(rng.integers(1, 3)), (X, INS, DEL)[int(rng.integers(0, 3))]) for t in range(n)]
        c.add(f"long {n}", [w(140, X)] + words + [w(180, X)])
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_stats()
    got = F.cigar_tails_batch(ctx, c.words, c.jobs)
    st = ctx.kernel_stats()
    assert st["cigar_tails"]["launches"] == 1 and st["cigar_tails"]["work_units"] == len(c.jobs) and list(st) == ["cigar_tails"]
    c.check(got)
    assert (got[:, 0] > 0).sum() > 20 and (got[:, 4] > 0).sum() > 20
    # bad jobs are refused on the host and nothing is launched
    ctx.reset_kernel_stats()
    words = [w(10, EQ), w(3, X), w(5, 4), w(9, EQ)]
    for bad in ((0, 5), (5, 0), (3, 2), (1, 2), (0, 1, 65536), (0, 1, 0, (1 << 30) + 1), (0, 1, 0, 0, 1 << 19)):
        with pytest.raises(F.FloxerError):
            F.cigar_tails_batch(ctx, words, [(0, 2), bad])
    assert ctx.kernel_stats() == {}
    assert F.cigar_tails_batch(ctx, words, []).shape == (0, 8) and F.cigar_tails_batch(ctx, [], [(0, 0)]).tolist() == [[0] * 8]
    ctx.enable_kernel_timing(False)


# ------------------------------------------------------------------------------------------------ the pipeline
@gpu
def test_off_is_exact_and_launches_nothing(world):
    ctx, reads, off = world["ctx"], world["reads"], world["runs"]["off"]
    assert "cigar_tails" not in world["stats"]["off"] and "cigar_tails" not in world["stats"]["off_ext"]
    st = world["stats"]["split"]["cigar_tails"]
    assert st["launches"] >= 1 and st["work_units"] > 0 and st["device_ms"] > 0
    # the earlier entry point against the new one with no struct, a zeroed one and one switched off
    L = capi.lib()
    p = F.params(error_probability=RATE)
    pool, offs, n = F._pool_and_offsets(reads)
    out_opt, tags, part = F.output_options(max_alignments=1, mapq=True), F.tag_options(md=True), F.partial_options(min_query_span=SPAN)
    bundle = capi.RunOptions()
    bundle.output, bundle.tags, bundle.partial = C.pointer(out_opt), C.pointer(tags), C.pointer(part)
    run = C.c_void_p()
    capi.check(L.flx_align_reads_opt(ctx.h, C.byref(p), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n, C.byref(bundle), C.byref(run)))
    old = F._collect_run(run, n, md=True)
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_stats()
    for split in (None, capi.SplitOptions(), F.split_options(enable=False, x_drop=30)):
        got = aligner(ctx, split).align_reads(reads)
        for other in (old, off):
            same(got, other)
            assert got.md == other.md and got.mapq.tolist() == other.mapq.tolist()
            assert (got.raw["coff"] == other.raw["coff"]).all() and len(got.cigars) == len(other.cigars)
            for a, b in zip(got.rows, other.rows):
                assert (got.cigars[a[5]: a[5] + a[6]] == other.cigars[b[5]: b[5] + b[6]]).all()
    assert "cigar_tails" not in ctx.kernel_stats()
    ctx.enable_kernel_timing(False)
    # not vacuous: every tailed read is one full-length record here, the chimera is rescued, the random read unmapped
    rows = by_read(off)
    for i in world["tailed"]:
        assert len(rows[i]) == 1 and "S" not in rows[i][0][1][5], i
    assert [r[1] for _, r in rows[len(reads) - 1]] == [4] and all(len(rows[i]) == 2 for i in world["rescued"])


@gpu
def test_split_reads_are_a_clipped_primary_and_supplementaries_inside_the_tails(world):
    chroms, reads, tailed = world["chroms"], world["reads"], world["tailed"]
    want = expected_tails(world)
    run = world["runs"]["split"]
    rows, plain = by_read(run), by_read(world["runs"]["off"])
    iv = run.query_intervals([len(r) for r in reads])
    n_sup = 0
    for i, (kind, o, ch, _, side, n_tail) in tailed.items():
        t = want[i]
        tail_rows, other = tail_of(t, side)
        assert other == 0 and abs(tail_rows - n_tail) <= 100, (i, kind, t)        # the intended tail, on the GPU's own CIGAR
        recs = rows[i]
        (j0, prim), old = recs[0], plain[i][0][1]
        assert prim[1] == old[1] == (16 if o else 0) and prim[2] == old[2] == ch
        fwd, ori = check_record(chroms, reads[i], prim, run.md[j0])
        assert ori == (t[0], len(reads[i]) - 1 - t[4]), (i, ori, t)               # the rule's kept interval
        assert prim[3] >= old[3] + t[1] and core_of(prim)[2] <= core_of(old)[2] - t[5]     # inside the kept part's reference window
        assert prim[4] <= old[4] - t[2] - t[6]
        assert int(run.mapq[j0]) == int(world["runs"]["off"].mapq[plain[i][0][0]])  # the value of the read's root records
        # the tail in forward coordinates
        n = len(reads[i])
        lo, hi = (n - tail_rows, n - 1) if (side == "right") != bool(o) else (0, tail_rows - 1)
        taken = [tuple(iv[j0])]
        for j, rec in recs[1:]:
            assert rec[1] & ~16 == 2048
            f, _ = check_record(chroms, reads[i], rec, run.md[j])
            assert lo <= f[0] and f[1] <= hi and f[1] - f[0] + 1 >= SPAN, (i, f, lo, hi)
            assert all(f[1] < a or f[0] > b for a, b in taken), (i, f, taken)
            taken.append(f)
            n_sup += 1
        assert [tuple(iv[j]) for j, _ in recs[1:]] == sorted(tuple(iv[j]) for j, _ in recs[1:])
        if kind == "foreign":
            assert len(recs) == 2, (i, recs)
        else:
            assert len(recs) == 1, (i, recs)                                       # junk: a single clipped primary
    assert n_sup == sum(1 for v in tailed.values() if v[0] == "foreign")


@gpu
def test_extension_carries_every_end_to_the_break(world):
    chroms, reads, tailed = world["chroms"], world["reads"], world["tailed"]
    base, ext = world["runs"]["split"], world["runs"]["split_ext"]
    moved = check_extended(chroms, reads, base, ext, list(tailed) + world["rescued"])
    assert moved >= sum(1 for v in tailed.values() if v[0] == "foreign")
    iv = ext.query_intervals([len(r) for r in reads])
    rows = by_read(ext)
    for i, (kind, o, ch, _, side, n_tail) in tailed.items():
        if kind != "foreign":
            continue
        (a, b) = sorted(tuple(iv[j]) for j, _ in rows[i])
        brk = LEN - n_tail
        assert abs(a[1] + 1 - brk) <= 100 and abs(b[0] - brk) <= 100, (i, a, b)   # both records now end at the break, within x_drop rows


@gpu
def test_other_reads_are_untouched_and_the_counters_add_up(world):
    reads, tailed, rescued = world["reads"], world["tailed"], world["rescued"]
    for on, off in (("split", "off"), ("split_ext", "off_ext")):
        a, b = world["runs"][on], world["runs"][off]
        ra, rb = by_read(a), by_read(b)
        for i in range(len(reads)):
            if i in tailed:
                continue
            assert [r for _, r in ra[i]] == [r for _, r in rb[i]], i
            for (j, _), (j0, _) in zip(ra[i], rb[i]):
                x, y = a.rows[j], b.rows[j0]
                assert (a.cigars[x[5]: x[5] + x[6]] == b.cigars[y[5]: y[5] + y[6]]).all() and a.md[j] == b.md[j0] and a.mapq[j] == b.mapq[j0]
        assert a.skipped.tolist() == b.skipped.tolist()
        pa, pb = world["pcs"][on], world["pcs"][off]
        n_split_records = sum(len(ra[i]) for i in tailed)
        assert pa["reads_split"] == len(tailed) and pb["reads_split"] == 0
        assert pa["reads_rescued"] == pb["reads_rescued"] == len(rescued)
        assert pa["partial_records"] == pb["partial_records"] + n_split_records and pb["partial_records"] == sum(len(rb[i]) for i in rescued)
        assert pa["records_dropped"] == pb["records_dropped"] + len(tailed)        # the primary that was written before is not any more
        assert pa["records"] == a.n_records == pb["records"] + n_split_records - len(tailed)
        for key in ("root_alignments_found", "root_alignments_requested", "inner_tests_requested", "reads", "anchors"):
            assert pa[key] == pb[key], key
    # without partial, without -N 1 or with -w the option is refused
    ctx, p = world["ctx"], F.params(error_probability=RATE)
    with pytest.raises(F.FloxerError, match="needs flx_partial_options"):
        F.aligner(ctx, p, F.output_options(max_alignments=1), split=F.split_options()).align_reads(reads)
    with pytest.raises(F.FloxerError, match="max_alignments_per_read == 1"):
        F.aligner(ctx, p, partial=F.partial_options(), split=F.split_options()).align_reads(reads)
    with pytest.raises(F.FloxerError, match="without_cigar"):
        F.aligner(ctx, F.params(error_probability=RATE, without_cigar=True), F.output_options(max_alignments=1), partial=F.partial_options(),
                  split=F.split_options()).align_reads(reads)


def dump(path):
    """the records of the batch with split and extend on, as JSON; run in a process of its own: some switches are read once per process"""
    chroms, reads, _, _ = build_batch()
    ctx = F.context(F.fmindex(chroms))
    run = aligner(ctx, F.split_options(), F.extend_options()).align_reads(reads)
    with open(path, "w") as f:
        json.dump(dict(records=run.records(), md=[m.decode() if m else None for m in run.md], mapq=run.mapq.tolist(), host_rounds=os.environ.get("FLX_HOST_ROUNDS")), f)
    ctx.close()


@gpu
def test_same_records_for_resident_reads_a_cut_batch_host_rounds_and_other_conventions(world, tmp_path, monkeypatch):
    ctx, reads, ext = world["ctx"], world["reads"], world["runs"]["split_ext"]
    al = aligner(ctx, F.split_options(), F.extend_options())
    rr = F.resident_reads(ctx, reads)
    resident = al.align_reads(rr)
    rr.close()
    monkeypatch.setenv("FLX_CHUNK_READS", str((len(reads) + 1) // 2))
    cut = al.align_reads(reads)
    monkeypatch.delenv("FLX_CHUNK_READS")
    for other in (resident, cut):
        same(other, ext)
        assert other.md == ext.md and other.mapq.tolist() == ext.mapq.tolist()
    out = str(tmp_path / "host_rounds.json")
    code = f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_tails_gpu as T; T.dump({out!r})"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FLX_HOST_ROUNDS="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = json.load(open(out))
    assert got["host_rounds"] == "1" and got["records"] == [list(x) for x in ext.records()]
    assert got["md"] == [m.decode() if m else None for m in ext.md] and got["mapq"] == ext.mapq.tolist()
    # other conventions: a tail must have more rows than any of these has, or a drop no read shows: nothing is split
    off = world["runs"]["off"]
    for split in (F.split_options(min_tail_rows=1500), F.split_options(x_drop=1 << 20)):
        run = aligner(ctx, split).align_reads(reads)
        same(run, off)
    # a larger span than any node inside a tail has: the reads with a foreign tail are a clipped primary alone
    run = aligner(ctx, F.split_options(), span=1000).align_reads(reads)
    rows = by_read(run)
    for i in world["tailed"]:
        assert len(rows[i]) == 1 and "S" in rows[i][0][1][5], i


@gpu
def test_cli_writes_the_librarys_records_with_sa_on_both(world, tmp_path):
    chroms, reads, ext = world["chroms"], world["reads"], world["runs"]["split_ext"]
    fasta, fastq = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq")
    with open(fasta, "w") as f:
        for i, c in enumerate(chroms):
            f.write(f">chr{i}\n" + "\n".join(letters(c[o: o + 100]) for o in range(0, len(c), 100)) + "\n")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
    recs = ext.records()
    names = [f"chr{i}" for i in range(len(chroms))]
    want_sa = sa_strings(recs, names, ext.mapq.tolist())
    out = str(tmp_path / "out.sam")
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    r = subprocess.run([exe, "--reference", fasta, "--queries", fastq, "--output", out, "--error-probability", str(RATE), "--threads", "2", "-N", "1", "-Q",
                        "--md-tag", "--partial-alignments", "--partial-min-span", str(SPAN), "--partial-extend", "--split-tails", "--sa-tag"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = []
    for line in open(out).read().splitlines():
        if line.startswith("@"):
            continue
        f = line.split("\t")
        tags = dict((t[:2], t[5:]) for t in f[11:])
        got.append(((int(f[0][4:]), int(f[1]), -1 if f[2] == "*" else names.index(f[2]), int(f[3]) - 1, int(tags.get("NM", 0)), "" if f[5] == "*" else f[5]),
                    int(f[4]), tags.get("MD"), tags.get("SA")))
    assert [x[0] for x in got] == recs
    assert [x[1] for x in got] == ext.mapq.tolist()
    assert [x[2] for x in got] == [m.decode() if m else None for m in ext.md]
    assert [x[3] for x in got] == want_sa
    # SA:Z on both records of every read with a foreign tail, none on a junk-tailed read's single record
    rows = by_read(ext)
    for i, v in world["tailed"].items():
        for j, _ in rows[i]:
            assert (want_sa[j] is not None) == (v[0] == "foreign"), (i, j)
