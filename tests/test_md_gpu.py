"""The MD tag on the GPU path (flx_tag_options.md, flx_align_batch_md, CLI --md-tag). The expected strings are the plain-Python rule
(tests/test_md_host.py md_from_cigar) applied to the oracle's records and CIGARs, never to the product's own. The tests marked gpu need
an MI355X; the one that checks what the crafted inputs cover runs on the oracle alone."""
import os
import re
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import simulate as S
import oracle_lib as O
from test_md_host import bam_records, cigar_words, md_from_cigar, reference_from_md
from test_output_options_host import restate

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 0.04
READ_RATE = 0.03
FIELDS = ["read", "flag", "ref", "pos", "nm", "coff", "clen", "res"]
LETTERS = "NACGTN"


def letters(r):
    return "".join(LETTERS[int(x)] if int(x) < 6 else "N" for x in r)


def other(x):
    return x % 4 + 1


# ------------------------------------------------------------------------------------------------ 1. crafted pairs
def crafted_pairs():
    """[(name, reference window, query, allowed errors, mode)]: the query is a stretch of the window with the named edits"""
    rng = np.random.default_rng(23)
    pairs = []

    def window(n):
        return rng.integers(1, 5, size=n, dtype=np.uint8)

    def case(name, n, edit, k, flank=30, mode=F.MODE_WITH_CIGAR, ref_edit=None, prep=None):
        w = window(n + 2 * flank)
        if prep:
            prep(w, flank)
        q = edit(w[flank: flank + n].copy())
        if ref_edit:
            ref_edit(w, flank)
        pairs.append((name, w, np.asarray(q, dtype=np.uint8), k, mode))

    def sub(q, at):                                              # a letter that its column and both neighbours do not hold: the
        q0 = q.copy()                                            # mismatch cannot be explained away by a shift
        for p in at:
            q[p] = min(set((1, 2, 3, 4)) - {int(q0[max(p - 1, 0)]), int(q0[p]), int(q0[min(p + 1, len(q0) - 1)])})
        return q

    def same_behind(w, flank):                                   # the base behind the stretch repeats its last one: the changed last
        w[flank + 300] = w[flank + 299]                          # query symbol matches neither, so the column stays a mismatch
    case("first_last", 300, lambda q: sub(q, [0, len(q) - 1]), 6, ref_edit=same_behind)
    case("adjacent_x", 300, lambda q: sub(q, [100, 101, 102, 200, 201]), 8)
    def clean_stretches(w, flank):                               # a stretch to delete holds neither of the letters next to it, so that
        for a, b in ((100, 101), (300, 305), (600, 670)):        # no part of it can be matched and the deletion stays one op
            free = sorted(set((1, 2, 3, 4)) - {int(w[flank + a - 1]), int(w[flank + b])})
            w[flank + a: flank + b] = [free[i % 2] for i in range(b - a)]
    case("deletions", 900, lambda q: np.concatenate([q[:100], q[101:300], q[305:600], q[670:]]), 90, prep=clean_stretches)
    case("insertion", 300, lambda q: np.concatenate([q[:150], np.array([other(q[150])] * 1, np.uint8), q[150:]]), 4)
    def d_then_x(w, flank):                                      # A CCCC G A in the window, A T A in the query: four deleted, one mismatch
        w[flank + 199: flank + 206] = [1, 2, 2, 2, 2, 3, 1]

    def d_then_x_query(q):
        q = np.concatenate([q[:200], q[204:]])
        q[200] = 4
        return q
    case("d_next_to_x", 400, d_then_x_query, 10, prep=d_then_x)

    def with_n(w, flank):
        w[flank + 50] = 5
        w[flank + 120: flank + 124] = 5
        w[flank + 200] = 0
    case("non_acgt", 300, lambda q: np.concatenate([q[:119], q[125:]]), 12, ref_edit=with_n)
    def long_x_ref(w, flank):                                    # eighty A in the window against eighty C in the query, between letters
        w[flank + 159: flank + 241] = [3] + [1] * 80 + [4]       # that pin the diagonal: one X run of more than 64 columns

    def long_x_query(q):
        q[160:240] = 2
        return q
    case("x_run_80", 400, long_x_query, 90, prep=long_x_ref)
    case("words_65", 3000, lambda q: sub(q, range(20, 3000, 60)), 80)
    case("words_4097", 30000, lambda q: sub(q, range(5, 30000, 12)), 2600)
    case("perfect", 2000, lambda q: q, 3)
    case("no_alignment", 200, lambda q: window(200), 3)
    case("exists_mode", 200, lambda q: sub(q, [50]), 3, mode=F.MODE_EXISTS)
    return pairs


CLASSES = {
    "first_last": lambda c, md: md.endswith(b"0") and c.endswith("1X"),
    "adjacent_x": lambda c, md: re.search(rb"[A-Z]0[A-Z]0[A-Z]", md) is not None and "3X" in c,
    "deletions": lambda c, md: all(f"{n}D" in c for n in (1, 5, 70)) and re.search(rb"\^[A-Z]{70}", md) is not None,
    "insertion": lambda c, md: re.fullmatch(r"\d+=\d+I\d+=", c) is not None and md.isdigit(),
    "d_next_to_x": lambda c, md: re.search(r"\d+D\d+X|\d+X\d+D", c) is not None,
    "non_acgt": lambda c, md: md.count(b"N") >= 3 and re.search(rb"\^[A-Z]*N[A-Z]*", md) is not None,
    "x_run_80": lambda c, md: "80X" in c and re.search(rb"A(0A){79}", md) is not None,
    "words_65": lambda c, md: 64 < len(cigar_words(c)) <= 4096,
    "words_4097": lambda c, md: len(cigar_words(c)) > 4096,
    "perfect": lambda c, md: md == b"2000",
}


def _oracle_expect(pairs):
    out = []
    for name, w, q, k, mode in pairs:
        r = O.align(w, q, k)
        out.append(None if r is None else (r[0], r[1], r[2], md_from_cigar(w, r[1], cigar_words(r[2]))))
    return out


def test_crafted_pairs_cover_every_class_on_the_oracle():
    """What the crafted inputs exercise, from the oracle's own CIGARs (no GPU). A mismatch in the query's first column never is an X in
    the reference's alignment: the traceback of the alignment library it calls prefers an insertion over a diagonal move of equal cost, so with the
    window's free start the first reference-consuming column is always a match and no MD of this aligner starts with 0 - asserted here
    as what it is; a mismatch in the last column is an X and the MD ends with 0."""
    pairs = crafted_pairs()
    exp = dict(zip([p[0] for p in pairs], _oracle_expect(pairs)))
    for name, ok in CLASSES.items():
        assert exp[name] is not None, name
        assert ok(exp[name][2], exp[name][3]), (name, exp[name][2][:80], exp[name][3][:80])
    assert exp["first_last"][2].startswith("1I") and not exp["first_last"][3].startswith(b"0")
    assert exp["no_alignment"] is None and exp["exists_mode"] is not None
    # the companion inverts the rule on every pair
    for name, w, q, k, mode in pairs:
        if exp[name] is not None:
            nm, begin, cig, md = exp[name]
            span = sum(x >> 4 for x in cigar_words(cig) if x & 15 in (2, 7, 8))
            assert reference_from_md(letters(q), cigar_words(cig), md) == letters(w[begin: begin + span]).replace("$", "N"), name


@pytest.fixture(scope="module")
def small_ctx():
    g = S.make_genome(100000, 1, seed=3)
    ctx = F.context(F.fmindex(g))
    yield ctx
    ctx.close()


@gpu
def test_crafted_pairs_through_align_batch_md(small_ctx):
    pairs = crafted_pairs()
    exp = _oracle_expect(pairs)
    ref_pool = np.concatenate([p[1] for p in pairs])
    q_pool = np.concatenate([p[2] for p in pairs])
    jobs, ro, qo = [], 0, 0
    for name, w, q, k, mode in pairs:
        jobs.append((ro, len(w), qo, len(q), k, mode))
        ro += len(w)
        qo += len(q)
    got = F.align_batch(small_ctx, q_pool, jobs, reference_pool=ref_pool, md=True)
    plain = F.align_batch(small_ctx, q_pool, jobs, reference_pool=ref_pool)
    for (name, w, q, k, mode), g, p, e in zip(pairs, got, plain, exp):
        if name == "no_alignment":
            assert g is None and p is None
        elif mode == F.MODE_EXISTS:
            assert g is not None and g[3] is None and g[:3] == p       # no CIGAR, no MD
        else:
            assert g[:3] == p == e[:3], name
            assert g[3] == e[3], (name, g[3][:60], e[3][:60])
    # one pair at a time gives the same strings
    for (name, w, q, k, mode), e in zip(pairs[:6], exp[:6]):
        assert F.align(small_ctx, w, q, k, md=True) == e, name


# ------------------------------------------------------------------------------------------------ 2.-4. whole path
def _planted():
    """the planted two-sequence text of tests/test_mapq_gpu.py's kind, plus reads with a multi-base deletion and adjacent mismatches"""
    rng = np.random.default_rng(17)
    chroms = [c.copy() for c in S.make_genome(400_000, 2, seed=16)]
    a, b = (chroms[0][s:s + 3000].copy() for s in (50_000, 120_000))
    chroms[1][30_000:33_000] = a
    chroms[1][90_000:93_000] = b
    chroms[0][300_000:303_000] = b
    reads = []
    for seg, seed in [(a, 1), (b, 2)]:
        reads += S.make_reads([seg], 8, 2000, READ_RATE, seed=100 + seed)[0]
    reads += S.make_reads(chroms, 24, 2000, READ_RATE, seed=105)[0]
    for start in (10_000, 222_000):
        r = chroms[1][start: start + 2000].copy()
        r = np.concatenate([r[:700], r[706:]])                   # a deletion of six
        for p in (300, 301, 302, 1500, 1501):
            r[p] = other(r[p])                                   # adjacent mismatches
        reads.append(r)
        reads.append(O.revcomp(r))
    reads += [np.zeros(0, np.uint8), np.array([1, 2, 3], np.uint8), rng.integers(1, 5, size=2000, dtype=np.uint8)]   # skipped, skipped, unmapped
    return chroms, reads


@pytest.fixture(scope="module")
def planted():
    chroms, reads = _planted()
    ctx = F.context(F.fmindex(chroms))
    yield chroms, reads, ctx, O.Index(chroms)
    ctx.close()


def _expected_mds(chroms, rows):
    return [None if flag & 4 else md_from_cigar(chroms[ref], pos, cigar_words(cig)) for (_, flag, ref, pos, _, cig) in rows]


def _check_inverse(chroms, reads, rows, mds):
    for (read, flag, ref, pos, nm, cig), md in zip(rows, mds):
        if flag & 4:
            assert md is None
            continue
        q = reads[read] if not flag & 16 else O.revcomp(reads[read])
        span = sum(x >> 4 for x in cigar_words(cig) if x & 15 in (2, 7, 8))
        assert reference_from_md(letters(q), cigar_words(cig), md) == letters(chroms[ref][pos: pos + span]), (read, flag, pos)


def _same_records(a, b):
    assert len(a.raw) == len(b.raw)
    for f in FIELDS:
        assert (a.raw[f] == b.raw[f]).all(), f
    assert (a.cigars == b.cigars).all() and a.skipped.tolist() == b.skipped.tolist()


@gpu
@pytest.mark.parametrize("kw,okw", [(dict(), dict()), (dict(interval_optimization=True), dict(interval_opt=True))])
def test_whole_path_md_is_the_rule_on_the_oracles_records(planted, kw, okw):
    chroms, reads, ctx, oidx = planted
    rows = oidx.run(reads, O.params(error_probability=RATE, **okw), threads=8).records()
    want = _expected_mds(chroms, rows)
    # not vacuous
    assert {r[1] & 16 for r in rows if not r[1] & 4} == {0, 16} and any(r[1] & 4 for r in rows)
    assert any(re.search(rb"\^[A-Z]{2,}", m) for m in want if m) and any(re.search(rb"[A-Z]0[A-Z]", m) for m in want if m)
    p = F.params(error_probability=RATE, **kw)
    plain = F.aligner(ctx, p).align_reads(reads)
    assert plain.records() == rows and plain.md is None
    got = F.aligner(ctx, p, md=True).align_reads(reads)
    _same_records(got, plain)                                            # every other field, the CIGAR pool and `skipped`
    assert got.md == want
    _check_inverse(chroms, reads, rows, got.md)
    # 3. the kept records' MDs are the full run's MDs of the same records
    for drop, cap, mapq in [(True, 1, True), (True, 0, False), (False, 2, False)]:
        keep = restate(rows, drop, cap)
        sel = F.aligner(ctx, p, F.output_options(drop, cap, mapq), md=True).align_reads(reads)
        assert sel.records() == [r for r, k in zip(rows, keep) if k], (drop, cap)
        assert sel.md == [m for m, k in zip(want, keep) if k], (drop, cap)
        _same_records(sel, F.aligner(ctx, p, F.output_options(drop, cap, mapq)).align_reads(reads))


@gpu
def test_run_without_md_has_no_md_bytes_and_tag_options_are_checked(planted):
    import ctypes as C
    from floxer_amd import capi
    chroms, reads, ctx, _ = planted
    L = capi.lib()
    p = F.params(error_probability=RATE)
    pool = np.concatenate([r for r in reads[:6]])
    offs = np.cumsum([0] + [len(r) for r in reads[:6]]).astype(np.uint64)
    counts = []
    for tags in (None, capi.TagOptions(), F.tag_options(md=True)):
        run = C.c_void_p()
        capi.check(L.flx_align_reads_with_tags(ctx.h, C.byref(p), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), 6, None,
                                               C.byref(tags) if tags is not None else None, C.byref(run)))
        counts.append((L.flx_run_num_records(run), L.flx_run_num_md_bytes(run), L.flx_run_copy_md(run, None, None)))
        L.flx_run_free(run)
    assert counts[0] == counts[1] and counts[0][1] == 0 and counts[0][2] == -1         # zeroed is NULL: no MD bytes, nothing to copy
    assert counts[2][0] == counts[0][0] and counts[2][1] > 0 and counts[2][2] == 0
    with pytest.raises(F.FloxerError, match="without_cigar"):
        F.aligner(ctx, F.params(error_probability=RATE, without_cigar=True), md=True).align_reads(reads[:4])
    bad = capi.TagOptions()
    bad.md = 2
    run = C.c_void_p()
    assert L.flx_align_reads_with_tags(ctx.h, C.byref(p), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), 6, None, C.byref(bad), C.byref(run)) == -1


@gpu
def test_resident_host_and_chunked_reads_give_the_same_mds(planted, monkeypatch):
    chroms, reads, ctx, oidx = planted
    reads = reads + S.make_reads(chroms, 100, 1500, READ_RATE, seed=55)[0]
    p = F.params(error_probability=RATE)
    rows = oidx.run(reads, O.params(error_probability=RATE), threads=8).records()
    want = _expected_mds(chroms, rows)
    for opt in (None, F.output_options(True, 1, True)):
        al = F.aligner(ctx, p, opt, md=True)
        host = al.align_reads(reads)
        if opt is None:
            assert host.records() == rows and host.md == want
        rr = F.resident_reads(ctx, reads)
        resident = al.align_reads(rr)
        rr.close()
        monkeypatch.setenv("FLX_CHUNK_READS", "9")          # many slices over the context's lanes: the offsets are rebased over the parts
        chunked = al.align_reads(reads)
        monkeypatch.delenv("FLX_CHUNK_READS")
        for other_run in (resident, chunked):
            assert other_run.records() == host.records() and other_run.md == host.md
        # the resident and the host run have the same refs (the bytes between the strings are slab gaps: unspecified); the chunked
        # run's refs are rebased over its parts and stay inside its bytes
        assert (resident.md_refs == host.md_refs).all() and len(resident.md_bytes) == len(host.md_bytes)
        for lo, n in chunked.md_refs:
            assert int(lo) + int(n) <= len(chunked.md_bytes)


# ------------------------------------------------------------------------------------------------ 5. the metric's read shape
@gpu
def test_metric_read_shape_and_a_99kb_read():
    genome = S.make_genome(3_000_000, 2, seed=71)
    reads, _, _ = S.make_reads(genome, 12, 10000, 0.08, seed=72)
    ctx = F.context(F.fmindex(genome))
    got = F.aligner(ctx, F.params(error_probability=0.08), md=True).align_reads(reads)
    rows = O.Index(genome).run(reads, O.params(error_probability=0.08), threads=8).records()
    assert got.records() == rows
    assert got.md == _expected_mds(genome, rows)
    _check_inverse(genome, reads, rows, got.md)
    words = [len(cigar_words(r[5])) for r in rows if not r[1] & 4]
    # not vacuous: CIGARs of ~1500 words; ~800 edits, of which the mismatches and deletions (two in three) take two bytes or more each
    assert min(words) > 1000 and min(len(m) for m in got.md if m) > 1000
    ctx.close()
    # one read close to the length limit (-I keeps the oracle's root alignments of it few)
    g = S.make_genome(150000, 1, seed=81)
    rng = np.random.default_rng(82)
    # (the stretch to delete holds neither of the letters next to it, and no mismatch lies near it: no part of it can be matched, so
    # the deletion stays one op - see crafted_pairs)
    free = sorted(set((1, 2, 3, 4)) - {int(g[0][59999]), int(g[0][60100])})
    g[0][60000:60100] = [free[i % 2] for i in range(100)]
    long_read = g[0][20000:20000 + 99000].copy()
    for pos in rng.choice(len(long_read), size=600, replace=False):
        if not 39900 <= pos < 40200:
            long_read[pos] = other(long_read[pos])
    long_read = np.concatenate([long_read[:40000], long_read[40100:]])               # and a deletion of a hundred
    ctx = F.context(F.fmindex(g))
    got = F.aligner(ctx, F.params(error_probability=0.01, interval_optimization=True), md=True).align_reads([long_read])
    rows = O.Index(g).run([long_read], O.params(error_probability=0.01, interval_opt=True), threads=4).records()
    assert got.records() == rows and not rows[0][1] & 4
    assert got.md == _expected_mds(g, rows)
    _check_inverse(g, [long_read], rows, got.md)
    assert any("100D" in r[5] for r in rows) and any(re.search(rb"\^[A-Z]{100}", m) for m in _expected_mds(g, rows))      # the input holds it
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. no host text
@gpu
def test_context_on_an_image_with_a_meta_imported_index_gives_the_same_mds():
    import torch
    genome = S.make_genome(300000, 3, seed=51)
    reads, _, _ = S.make_reads(genome, 60, 1500, 0.06, seed=52)
    idx = F.fmindex(genome, device=0)
    base_ctx = F.context(idx)
    light = F.fmindex.from_meta(idx.meta())                  # no arrays: the host holds no text
    image = [torch.empty(n, dtype=torch.uint8, device="cuda:0") for n in idx.image_layout()]
    idx.image_upload(0, [b.data_ptr() for b in image])
    ctx = F.context(light, image=image)
    rows = O.Index(genome).run(reads, O.params(error_probability=0.06), threads=8).records()
    want = _expected_mds(genome, rows)
    for kw in (dict(), dict(interval_optimization=True)):
        p = F.params(error_probability=0.06, **kw)
        base = F.aligner(base_ctx, p, md=True).align_reads(reads)
        got = F.aligner(ctx, p, md=True).align_reads(reads)
        assert got.records() == base.records() and got.md == base.md
        if not kw:
            assert got.records() == rows and got.md == want
    ctx.close()
    base_ctx.close()


# ------------------------------------------------------------------------------------------------ 7. CLI
def _cli_md_check(tmp_path, fasta, fastq, flags, oparams, with_letters):
    """FASTQ -> SAM and -> BAM with --md-tag: each record's MD is the rule on that record's own POS / CIGAR and the FASTA, and equals
    the rule on the oracle's record"""
    from test_oracle_pins import _read_fasta, _read_fastq
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    refs = _read_fasta(fasta)
    ref_ranks = [O.chars_to_ranks(s) for _, s in refs]
    names = [n.split(" ")[0] for n, _ in refs]
    reads = _read_fastq(fastq)
    rows = O.Index(ref_ranks).run([O.chars_to_ranks(s) for _, s, _ in reads], oparams, threads=4).records()
    want = _expected_mds(ref_ranks, rows)
    if with_letters:                                         # (the golden inputs' alignments hold matches and insertions only)
        assert any(m and re.search(rb"\^[A-Z]{2,}", m) for m in want) and any(m and re.search(rb"[A-Z]0[A-Z]", m) for m in want)

    def run(out, *extra):
        cmd = [exe, "--reference", fasta, "--queries", fastq, "--output", out, *flags, "--threads", "1", *extra]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
        return open(out, "rb").read()

    plain = run(str(tmp_path / "plain.sam")).decode().splitlines()
    for extra in ([], ["--devices", "0,0"]):
        tagged = run(str(tmp_path / "md.sam"), "--md-tag", *extra).decode().splitlines()
        assert len(tagged) == len(plain)
        body = [l.split("\t") for l in tagged if not l.startswith("@")]
        assert len(body) == len(rows)
        for f, l0, m in zip(body, [l for l in plain if not l.startswith("@")], want):
            if f[2] == "*":
                assert "\t".join(f) == l0 and m is None
                continue
            own = md_from_cigar(ref_ranks[names.index(f[2])], int(f[3]) - 1, cigar_words(f[5]))
            assert f[-1] == "MD:Z:" + own.decode() and own == m and f[-2].startswith("NM:i:") and "\t".join(f[:-1]) == l0
    bam = bam_records(run(str(tmp_path / "md.bam"), "--md-tag"))
    assert [dict((t, v) for t, _, v in r["tags"]).get("MD") for r in bam] == want
    assert bam_records(run(str(tmp_path / "plain.bam"))) == [dict(r, tags=[t for t in r["tags"] if t[0] != "MD"]) for r in bam]
    kept = run(str(tmp_path / "one.sam"), "--md-tag", "-D", "-N", "1", "-Q").decode().splitlines()
    keep = restate(rows, True, 1)
    assert [l.split("\t")[-1] for l in kept if not l.startswith("@") and "MD:Z:" in l] == ["MD:Z:" + m.decode() for m, k in zip(want, keep) if k and m]
    r = subprocess.run([exe, "--reference", fasta, "--queries", fastq, "--output", str(tmp_path / "w.sam"), "-e", "2", "--md-tag", "-w"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr


@gpu
def test_cli_md_tag_sam_and_bam(tmp_path):
    g = os.path.join(ROOT, "tests", "golden")
    _cli_md_check(tmp_path, os.path.join(g, "reference.fasta"), os.path.join(g, "queries.fastq"),
                  ["--interval-optimization", "--query-errors", "2", "--seed-errors", "1", "--extra-verification-ratio", "2"],
                  O.params(query_errors=2, seed_errors=1, extra_ratio=2.0, interval_opt=True), with_letters=False)


@gpu
def test_cli_md_tag_on_reads_with_mismatches_and_deletions(tmp_path):
    """the same through files written here: the golden inputs' MDs are numbers only"""
    chroms, reads = _planted()
    reads = [r for r in reads if len(r) > 100]
    fasta, fastq = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq")
    with open(fasta, "w") as f:
        for i, c in enumerate(chroms):
            f.write(f">chr{i} planted\n" + "\n".join(letters(c[o: o + 80]) for o in range(0, len(c), 80)) + "\n")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
    _cli_md_check(tmp_path, fasta, fastq, ["--error-probability", str(RATE)], O.params(error_probability=RATE), with_letters=True)


# ------------------------------------------------------------------------------------------------ 8. kernel statistics
@gpu
def test_kernel_stats_show_md_build_only_with_md(planted):
    chroms, reads, _, _ = planted
    p = F.params(error_probability=RATE)
    stats = []
    for md in (False, True):
        c = F.context(F.fmindex(chroms))
        c.enable_kernel_timing(True)
        F.aligner(c, p, md=md).align_reads(reads)
        stats.append(c.kernel_stats())
        c.close()
    off, on = stats
    assert "md_build" not in off and on["md_build"]["launches"] > 0
    assert on["md_build"]["launches"] == on["ed_traceback"]["launches"]
    assert on["md_build"]["algorithmic_bytes"] > 0 and on["md_build"]["work_units"] > 0
    assert {n: k["launches"] for n, k in on.items() if n != "md_build"} == {n: k["launches"] for n, k in off.items()}
