"""Partial alignments on the GPU, through the C ABI: constructed chimeras whose halves are PEX nodes (so what must come out is known
exactly), checked column by column against the reference text and against the CPU oracle's alignment of each part; off is off;
the same records whatever the rounds' driver, the batch cut, the lanes and where the reads live; MD, -Q, -w, -d, the CLI, counters."""
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

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 0.07
LEN = 6000
CHROM = 1_000_000
FIELDS = ["read", "flag", "ref", "pos", "nm", "clen", "res"]


def letters(r):
    return "".join("$ACGTN"[x] for x in r)


def tree(n=LEN):
    k = int(capi.lib().flx_floating_point_error_aware_ceil(n * RATE))
    t = F.pex_tree(n, k, 2)
    return k, t.inner_nodes, t.leaves


def root_children(n=LEN):
    k, inner, leaves = tree(n)
    kids = sorted((nd for nd in inner + leaves if nd[0] == 0 and nd is not inner[0]), key=lambda nd: nd[1])
    assert len(kids) == 2 and kids[0][1] == 0 and kids[0][2] + 1 == kids[1][1] and kids[1][2] == n - 1
    return k, kids


def mutate(rng, seg, n_edits):
    """at most n_edits edits that keep the length: substitutions, and pairs of one deletion and one insertion (two edits)"""
    seg = seg.copy()
    n_pairs = n_edits // 8
    for p in rng.choice(len(seg), size=n_edits - 2 * n_pairs, replace=False):
        seg[p] = 1 + (seg[p] - 1 + int(rng.integers(1, 4))) % 4
    for _ in range(n_pairs):
        d, i = (int(x) for x in rng.integers(10, len(seg) - 10, size=2))
        seg = np.delete(seg, d)
        seg = np.insert(seg, i, int(rng.integers(1, 5)))
    return seg


class Chimera:
    """read: the rank sequence; parts: [(orientation, (from, to, errors) of a node in the oriented sequence, chromosome, truth start)],
    the records that must come out; windows: [(orientation, chromosome, start, end)], where the whole read is tried on the CPU"""

    def __init__(self, read, parts, windows):
        self.read, self.parts, self.windows = read, parts, windows


def oriented(read, o):
    return read if o == 0 else O.revcomp(read)


def chimera_ok(chroms, k, c):
    """on the CPU: the whole read aligns in neither truth window within k, and every expected part is within its node's errors in the
    window the truth gives it"""
    for o, ch, lo, hi in c.windows:
        if O.align(chroms[ch][max(0, lo): hi], oriented(c.read, o), k, mode=0) is not None:
            return False
    for o, (frm, to, e), ch, start in c.parts:
        lo = max(0, start - e)
        if O.align(chroms[ch][lo: start + (to - frm + 1) + e + 1], oriented(c.read, o)[frm: to + 1], e, mode=0) is None:
            return False
    return True


def make_halves(rng, chroms, kind, share=1.0):
    """the spans of the root's two children from two loci. kind 'ff': both on the read's strand; 'rr': the same read reverse
    complemented (both nodes are nodes of the reverse complement's tree); 'fr': the second half from the other strand - the reverse
    complement's tree then has its FIRST child wholly inside that half, so the two records are the first child in each orientation."""
    k, (a, b) = root_children()
    la, lb = a[2] - a[1] + 1, b[2] - b[1] + 1
    ca, cb = (int(x) for x in rng.integers(0, len(chroms), size=2))
    pa, pb = int(rng.integers(1000, CHROM // 2 - LEN)), int(rng.integers(CHROM // 2, CHROM - LEN - 1000))
    sa = mutate(rng, chroms[ca][pa: pa + la], int(a[3] * share))
    sb = mutate(rng, chroms[cb][pb: pb + lb], int(b[3] * share))
    win = lambda ch, p, o: (o, ch, p - LEN - k, p + 2 * LEN + k)
    if kind == "fr":
        read = np.concatenate([sa, O.revcomp(sb)])
        return Chimera(read, [(0, a[1:], ca, pa), (1, a[1:], cb, pb)], [win(ca, pa, 0), win(cb, pb, 0), win(ca, pa, 1), win(cb, pb, 1)])
    osq = np.concatenate([sa, sb])
    o = 0 if kind == "ff" else 1
    return Chimera(oriented(osq, o), [(o, a[1:], ca, pa), (o, b[1:], cb, pb)], [win(ca, pa, o), win(cb, pb, o)])


def make_break_at_30(rng, chroms):
    """the break at 1800 of 6000: the second child of the root lies wholly behind it; of the first child only its first child does"""
    k, inner, leaves = tree()
    _, (a, b) = root_children()
    a1 = min((nd for nd in inner + leaves if nd[0] == inner.index(a)), key=lambda nd: nd[1])
    brk = 1800
    assert a1[2] < brk < a[2] and a1[2] - a1[1] + 1 >= 1000
    ca, cb = (int(x) for x in rng.integers(0, len(chroms), size=2))
    pa, pb = int(rng.integers(1000, CHROM // 2 - LEN)), int(rng.integers(CHROM // 2, CHROM - LEN - 1000))
    sa = mutate(rng, chroms[ca][pa: pa + brk], 18)                      # 1 %: every node of a side stays far inside its budget
    sb = mutate(rng, chroms[cb][pb: pb + LEN - brk], 42)
    read = np.concatenate([sa, sb])
    win = lambda ch, p: (0, ch, p - LEN - k, p + 2 * LEN + k)
    return Chimera(read, [(0, b[1:], cb, pb + b[1] - brk), (0, a1[1:], ca, pa)], [win(ca, pa), win(cb, pb)])


def build_batch():
    """deterministic: ordinary simulated reads, chimeras (redrawn until the CPU agrees with their construction), a random read"""
    pool, chroms = S.make_genome_fast(CHROM, 2, seed=41)
    (rp, ro), _ = S.make_reads_fast(pool, [CHROM, CHROM], 20, 3000, 0.04, seed=42)
    reads = [rp[int(ro[i]): int(ro[i + 1])].copy() for i in range(20)]
    rng = np.random.default_rng(43)
    k, _ = root_children()
    chim = {}

    def draw(make, *a):
        for _ in range(20):
            c = make(rng, chroms, *a)
            if chimera_ok(chroms, k, c):
                return c
        raise AssertionError("no chimera that the CPU agrees with in 20 draws")

    for kind in ("ff", "rr", "fr", "ff", "rr", "fr"):
        chim[len(reads)] = draw(make_halves, kind, 1.0 if len(chim) < 3 else 0.5)
        reads.append(chim[len(reads)].read)
    thirty = {}
    for _ in range(2):
        thirty[len(reads)] = draw(make_break_at_30)
        reads.append(thirty[len(reads)].read)
    reads.append(rng.integers(1, 5, size=LEN, dtype=np.uint8))          # unmapped, and no part of it aligns anywhere
    reads += [np.zeros(0, np.uint8), np.array([1, 2, 3], np.uint8)]     # skipped
    return chroms, reads, chim, thirty


@pytest.fixture(scope="module")
def world():
    chroms, reads, chim, thirty = build_batch()
    ctx = F.context(F.fmindex(chroms))
    yield chroms, reads, chim, thirty, ctx
    ctx.close()


def same(a, b):
    assert len(a.raw) == len(b.raw)
    for f in FIELDS:
        assert (a.raw[f] == b.raw[f]).all(), f
    assert a.records() == b.records() and a.skipped.tolist() == b.skipped.tolist()


def by_read(run):
    out = {}
    for i, r in enumerate(run.records()):
        out.setdefault(r[0], []).append((i, r))
    return out


def words_of(cigar):
    out, n = [], 0
    for ch in cigar:
        if ch.isdigit():
            n = 10 * n + int(ch)
        else:
            out.append((n, ch))
            n = 0
    return out


def check_record(chroms, read, rec, md=None):
    """the CIGAR consumes the whole read, S included; every '=' column matches and every 'X' column differs; NM = #X + #I + #D; NM is
    the oracle's for the aligned part against the reference interval the record covers. Returns (forward interval, oriented interval)."""
    _, flag, ref, pos, nm, cigar = rec
    q = oriented(read, 1 if flag & 16 else 0)
    ops = words_of(cigar)
    lead = ops[0][0] if ops[0][1] == "S" else 0
    trail = ops[-1][0] if ops[-1][1] == "S" and len(ops) > 1 else 0
    core = ops[(1 if lead else 0): (len(ops) - 1 if trail else len(ops))]
    assert all(op in "=XID" and n > 0 for n, op in core), cigar
    qi, ri, errors, md_want, run = lead, pos, 0, "", 0
    for n, op in core:
        if op == "=":
            assert (q[qi: qi + n] == chroms[ref][ri: ri + n]).all(), (cigar, qi)
            qi, ri, run = qi + n, ri + n, run + n
        elif op == "X":
            assert (q[qi: qi + n] != chroms[ref][ri: ri + n]).all(), (cigar, qi)
            for t in range(n):
                md_want += str(run) + letters(chroms[ref][ri + t: ri + t + 1])
                run = 0
            qi, ri, errors = qi + n, ri + n, errors + n
        elif op == "I":
            qi, errors = qi + n, errors + n
        else:
            md_want += str(run) + "^" + letters(chroms[ref][ri: ri + n])
            run = 0
            ri, errors = ri + n, errors + n
    md_want += str(run)
    assert qi + trail == len(read) and errors == nm, (cigar, qi, trail, errors, nm)
    frm, to = lead, len(read) - 1 - trail
    best = O.align(chroms[ref][pos: ri], q[frm: to + 1], nm, mode=1)
    assert best is not None and best[0] == nm, (best, nm)
    if md is not None:
        assert md == md_want.encode(), (md, md_want)
    fwd = (len(read) - 1 - to, len(read) - 1 - frm) if flag & 16 else (frm, to)
    return fwd, (frm, to)


def budget_of(n, interval):
    _, inner, leaves = tree(n)
    (e,) = [nd[3] for nd in inner + leaves if (nd[1], nd[2]) == interval]
    return e


# ------------------------------------------------------------------------------------------------ off is off
@gpu
def test_off_is_off_and_mapped_reads_keep_their_records(world):
    chroms, reads, chim, thirty, ctx = world
    L = capi.lib()
    import ctypes as C
    p = F.params(error_probability=RATE)
    pool, offs, n = F._pool_and_offsets(reads)
    plain = F.aligner(ctx, p).align_reads(reads)
    zeroed = capi.PartialOptions()
    for bundle_partial in (None, zeroed):
        for with_bundle in ((True, False) if bundle_partial is None else (True,)):
            run = C.c_void_p()
            bundle = capi.RunOptions()
            if bundle_partial is not None:
                bundle.partial = C.pointer(bundle_partial)
            capi.check(L.flx_align_reads_opt(ctx.h, C.byref(p), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n,
                                             C.byref(bundle) if with_bundle else None, C.byref(run)))
            got = F._collect_run(run, n)
            same(got, plain)
            assert (got.cigars == plain.cigars).all() and (got.raw["coff"] == plain.raw["coff"]).all()
    off = F.aligner(ctx, p, partial=F.partial_options(enable=False)).align_reads(reads)
    same(off, plain)
    assert (off.cigars == plain.cigars).all()
    # not vacuous: the chimeras and the random read are unmapped, the simulated reads are mapped, two reads are skipped
    rows = by_read(plain)
    for i in list(chim) + list(thirty) + [len(reads) - 3]:
        assert [r[1] for _, r in rows[i]] == [4], i
    assert all(not rows[i][0][1][1] & 4 for i in range(20)) and plain.skipped.tolist()[-2:] == [1, 1]
    on = F.aligner(ctx, p, partial=F.partial_options()).align_reads(reads)
    got = by_read(on)
    for i in range(20):
        assert [r for _, r in got[i]] == [r for _, r in rows[i]]
        for (j, _), (j0, _) in zip(got[i], rows[i]):                    # word for word
            a, b = on.rows[j], plain.rows[j0]
            assert (on.cigars[a[5]: a[5] + a[6]] == plain.cigars[b[5]: b[5] + b[6]]).all()
    assert [r[1] for _, r in got[len(reads) - 3]] == [4] and on.skipped.tolist() == plain.skipped.tolist()


# ------------------------------------------------------------------------------------------------ constructed chimeras
@gpu
def test_constructed_chimeras_give_their_two_halves(world):
    chroms, reads, chim, thirty, ctx = world
    ctx.path_counters(reset=True)
    on = F.aligner(ctx, F.params(error_probability=RATE), partial=F.partial_options()).align_reads(reads)
    pc = ctx.path_counters()
    got = by_read(on)
    for i, c in chim.items():
        recs = [r for _, r in got[i]]
        assert len(recs) == 2 and recs[0][1] & ~16 == 0 and recs[1][1] & ~16 == 2048, recs
        seen = {}
        for rec in recs:
            fwd, ori = check_record(chroms, reads[i], rec)
            seen[(1 if rec[1] & 16 else 0, ori)] = rec
        assert sorted(seen) == sorted((o, (nd[0], nd[1])) for o, nd, _, _ in c.parts), (i, sorted(seen))
        for o, nd, ch, start in c.parts:
            rec = seen[o, (nd[0], nd[1])]
            assert rec[2] == ch and abs(rec[3] - start) <= nd[2] and rec[4] <= nd[2], (rec[:5], start, nd)
    # counters: every chimera is rescued, nothing else is
    n_partial = sum(1 for r in on.records() if any(op == "S" for _, op in words_of(r[5])))
    assert pc["reads_rescued"] == len(chim) + len(thirty) and pc["partial_records"] == n_partial == 2 * (len(chim) + len(thirty))
    assert pc["records"] == on.n_records and pc["reads"] == len(reads)
    assert (on.clips.sum(axis=1) > 0).sum() == n_partial
    iv = on.query_intervals([len(r) for r in reads])
    for i, c in chim.items():
        for j, rec in got[i]:
            assert tuple(iv[j]) == check_record(chroms, reads[i], rec)[0]


@gpu
def test_smaller_nodes_and_the_span_filter(world):
    chroms, reads, chim, thirty, ctx = world
    p = F.params(error_probability=RATE)
    brk = 1800
    _, (a, b) = root_children()
    for span, n_want in [(0, 2), (1000, 2), (1500, 1), (b[2] - b[1] + 2, 0)]:
        on = F.aligner(ctx, p, partial=F.partial_options(min_query_span=span)).align_reads(reads)
        got = by_read(on)
        for i, c in thirty.items():
            recs = [r for _, r in got[i]]
            if n_want == 0:
                assert [r[1] for r in recs] == [4]                      # the unmapped record is back
                continue
            assert len(recs) == n_want and recs[0][1] == 0, recs
            for rec, (o, nd, ch, start) in zip(recs, c.parts):
                fwd, ori = check_record(chroms, reads[i], rec)
                assert fwd == (nd[0], nd[1]) and (fwd[1] < brk or fwd[0] >= brk) and fwd[1] - fwd[0] + 1 >= max(span, 1000)
                assert rec[2] == ch and abs(rec[3] - start) <= nd[2] and rec[4] <= budget_of(LEN, fwd)
            if n_want == 2:
                assert recs[1][1] == 2048
        if n_want == 0:
            for i in chim:
                assert [r[1] for _, r in got[i]] == [4]


# ------------------------------------------------------------------------------------------------ invariance
def dump(path, tile=1):
    """the records of the batch (`tile` copies of it, one behind the other: a context uses as many lanes as the batch has 64 reads) with
    the option on, as JSON; run in a process of its own: some switches are read once per process"""
    chroms, reads, _, _ = build_batch()
    reads = reads * tile
    ctx = F.context(F.fmindex(chroms))
    run = F.aligner(ctx, F.params(error_probability=RATE), F.output_options(mapq=True), md=True, partial=F.partial_options()).align_reads(reads)
    with open(path, "w") as f:
        json.dump(dict(records=run.records(), md=[m.decode() if m else None for m in run.md], mapq=run.mapq.tolist(),
                       lanes=os.environ.get("FLX_LANES"), host_rounds=os.environ.get("FLX_HOST_ROUNDS")), f)
    ctx.close()


def in_process(tmp_path, name, tile=1, **env):
    out = str(tmp_path / f"{name}.json")
    code = f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_partial_gpu as T; T.dump({out!r}, {tile})"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return json.load(open(out))


@gpu
def test_same_records_whatever_the_driver_the_cut_the_lanes_and_the_reads_home(world, tmp_path, monkeypatch):
    chroms, reads, chim, thirty, ctx = world
    p = F.params(error_probability=RATE)
    al = F.aligner(ctx, p, F.output_options(mapq=True), md=True, partial=F.partial_options())
    base = al.align_reads(reads)
    assert sum(1 for r in base.records() if r[1] & 2048) == len(chim) + len(thirty)
    rr = F.resident_reads(ctx, reads)
    resident = al.align_reads(rr)
    rr.close()
    monkeypatch.setenv("FLX_CHUNK_READS", "5")
    chunked = al.align_reads(reads)
    monkeypatch.delenv("FLX_CHUNK_READS")
    for other in (resident, chunked):
        same(other, base)
        assert other.md == base.md
    # -I: fewer root alignments are asked for, the candidates are the same
    a, b = (F.aligner(ctx, F.params(error_probability=RATE, interval_optimization=io), partial=F.partial_options()).align_reads(reads) for io in (False, True))
    ra, rb = by_read(a), by_read(b)
    for i in list(chim) + list(thirty):
        assert [r for _, r in ra[i]] == [r for _, r in rb[i]], i
    want = dict(records=[list(r) for r in base.records()], md=[m.decode() if m else None for m in base.md], mapq=base.mapq.tolist())
    got = in_process(tmp_path, "host_rounds", FLX_HOST_ROUNDS="1")
    assert got["records"] == want["records"] and got["md"] == want["md"] and got["mapq"] == want["mapq"]
    # two lanes against sixteen: 36 copies of the batch, so that sixteen lanes have 64 reads each
    tile = 36
    tiled = [[r[0] + t * len(reads)] + r[1:] for t in range(tile) for r in want["records"]]
    for lanes in ("2", "16"):
        got = in_process(tmp_path, f"lanes{lanes}", tile, FLX_LANES=lanes, FLX_CHUNK_READS="64")
        assert got["lanes"] == lanes and got["records"] == tiled and got["md"] == want["md"] * tile and got["mapq"] == want["mapq"] * tile, lanes


# ------------------------------------------------------------------------------------------------ MD, -Q, -w, -d
@gpu
def test_md_of_partial_records_is_the_rule_on_their_own_cigar(world):
    chroms, reads, chim, thirty, ctx = world
    p = F.params(error_probability=RATE)
    on = F.aligner(ctx, p, md=True, partial=F.partial_options()).align_reads(reads)
    same(on, F.aligner(ctx, p, partial=F.partial_options()).align_reads(reads))
    n = 0
    for (j, rec), md in zip(enumerate(on.records()), on.md):
        if rec[1] & 4:
            assert md is None
        elif rec[0] in chim or rec[0] in thirty:
            check_record(chroms, reads[rec[0]], rec, md)
            n += 1
    assert n == 2 * (len(chim) + len(thirty))
    assert any(b"^" in m for m in on.md if m) and any(m and not m.isdigit() for m in on.md)


@gpu
def test_mapq_without_cigar_and_direct_full_verification(world):
    chroms, reads, chim, thirty, ctx = world
    p = F.params(error_probability=RATE)
    q = F.aligner(ctx, p, F.output_options(True, 1, True), partial=F.partial_options()).align_reads(reads)
    got = by_read(q)
    for i in list(chim) + list(thirty):
        assert len(got[i]) == 2 and [int(q.mapq[j]) for j, _ in got[i]] == [60, 60], i      # -D / -N 1 leave both records; each half is unique
    assert all(len(got[i]) == 1 for i in range(20))
    with pytest.raises(F.FloxerError, match="without_cigar"):
        F.aligner(ctx, F.params(error_probability=RATE, without_cigar=True), partial=F.partial_options()).align_reads(reads)
    d = F.aligner(ctx, F.params(error_probability=RATE, direct_full_verification=True), partial=F.partial_options()).align_reads(reads)
    rows = by_read(d)
    for i in list(chim) + list(thirty):
        assert [r[1] for _, r in rows[i]] == [4]                        # nothing climbs: the candidates are leaves, far below the default span
    same(d, F.aligner(ctx, F.params(error_probability=RATE, direct_full_verification=True)).align_reads(reads))


# ------------------------------------------------------------------------------------------------ CLI
@gpu
def test_cli_writes_the_librarys_records(world, tmp_path):
    chroms, reads, chim, thirty, ctx = world
    from test_partial_host import _bam
    keep = [i for i, r in enumerate(reads) if len(r) > 100]
    fasta, fastq = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq")
    with open(fasta, "w") as f:
        for i, c in enumerate(chroms):
            f.write(f">chr{i}\n" + "\n".join(letters(c[o: o + 100]) for o in range(0, len(c), 100)) + "\n")
    with open(fastq, "w") as f:
        for i in keep:
            f.write(f"@read{i}\n{letters(reads[i])}\n+\n{'I' * len(reads[i])}\n")
    lib_run = F.aligner(ctx, F.params(error_probability=RATE), md=True, partial=F.partial_options(min_query_span=1200, max_records=3)).align_reads([reads[i] for i in keep])
    want = [(f"read{keep[r[0]]}", r[1], "*" if r[2] < 0 else f"chr{r[2]}", r[3] + 1, r[5] or "*", None if r[1] & 4 else r[4], m.decode() if m else None)
            for r, m in zip(lib_run.records(), lib_run.md)]
    assert sum(1 for x in want if x[1] & 2048) == len(chim) + len(thirty)
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    for ext in ("sam", "bam"):
        out = str(tmp_path / f"out.{ext}")
        r = subprocess.run([exe, "--reference", fasta, "--queries", fastq, "--output", out, "--error-probability", str(RATE), "--threads", "2",
                            "--partial-alignments", "--partial-min-span", "1200", "--partial-max", "3", "--md-tag"],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        if ext == "sam":
            got = []
            for line in open(out).read().splitlines():
                if line.startswith("@"):
                    continue
                f = line.split("\t")
                tags = dict((t[:2], t[5:]) for t in f[11:])
                got.append((f[0], int(f[1]), f[2], int(f[3]), f[5], int(tags["NM"]) if "NM" in tags else None, tags.get("MD")))
                assert f[9] == letters(reads[int(f[0][4:])]) or int(f[1]) & 256
            assert got == want
        else:
            recs = _bam(out)
            # (l_seq: the whole read in every record that carries SEQ, a supplementary one too; a secondary record carries none)
            assert [(b["flag"], b["ref"], b["pos"] + 1, b["cigar"] or "*", b["l_seq"]) for b in recs] == \
                   [(x[1], -1 if x[2] == "*" else int(x[2][3:]), x[3], x[4], 0 if x[1] & 256 else len(reads[int(x[0][4:])])) for x in want]
