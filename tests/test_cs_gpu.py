"""The cs tag on the GPU path (flx_cs_options: kernel cs_build behind md_build; flx_align_batch_cs, flx_cs_batch, runs, CLI --cs-tag and
--cs-tag-long). The expected strings are the plain-Python rule of tests/cs_ref.py applied to the oracle's records and CIGARs (or, where
the oracle has no such stage, to each record's own written words), and every string is also read back through the rule's inverse and
compared with the sequences themselves. The tests marked gpu need an MI355X; the one that checks what the crafted inputs cover runs on
the oracle alone."""
import os
import re
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
from floxer_amd import simulate as S
import oracle_lib as O
import cs_ref as R
from test_cs_host import _raw_cs, bam_records, pack_jobs, random_paths
from test_md_gpu import READ_RATE, RATE, _planted, _same_records, letters, other
from test_output_options_host import restate

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [False, True]           # long?


# ------------------------------------------------------------------------------------------------ 1. crafted pairs
def crafted_pairs():
    """[(name, reference window, query, allowed errors, mode)]: the query is a stretch of the window with the named edits"""
    rng = np.random.default_rng(29)
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

    def runs(lengths):                                           # '=' runs of these lengths with one X column between them
        at, pos = [], 0
        for n in lengths[:-1]:
            pos += n
            at.append(pos)
            pos += 1
        return pos + lengths[-1], at

    def same_behind(w, flank):                                   # (tests/test_md_gpu.py: the changed last query symbol stays a mismatch)
        w[flank + 300] = w[flank + 299]
    case("first_last", 300, lambda q: sub(q, [0, len(q) - 1]), 6, ref_edit=same_behind)
    # the long form's '=' runs: 63, 64 and 65 letters (a lane's own loop against the whole wave's copy), four runs of 65 in a row, which
    # start at all four output offsets modulo 4, and one of 2000
    n, at = runs([40, 63, 64, 65, 65, 65, 65, 2000, 30])
    case("eq_runs_long", n, lambda q, at=at: sub(q, at), 12)
    # the short form's counts: every number of digits on either side of a power of ten
    n, at = runs([20, 9, 10, 99, 100, 999, 1000, 25])
    case("eq_runs_short", n, lambda q, at=at: sub(q, at), 10)

    def long_x_ref(w, flank):                                    # eighty A in the window against eighty C in the query, between letters
        w[flank + 159: flank + 241] = [3] + [1] * 80 + [4]       # that pin the diagonal: one X run of more than 64 columns
    def long_x_query(q):
        q[160:240] = 2
        return q
    case("x_run_80", 400, long_x_query, 90, prep=long_x_ref)

    def clean_80(w, flank):                                      # a stretch to delete holds neither of the letters next to it, so that
        free = sorted(set((1, 2, 3, 4)) - {int(w[flank + 199]), int(w[flank + 280])})      # no part of it can be matched
        w[flank + 200: flank + 280] = [free[i % 2] for i in range(80)]
    case("d_run_80", 500, lambda q: np.concatenate([q[:200], q[280:]]), 90, prep=clean_80)

    def insert_80(q):                                            # the same for a stretch the query has and the window does not
        free = sorted(set((1, 2, 3, 4)) - {int(q[199]), int(q[200])})
        return np.concatenate([q[:200], np.array([free[i % 2] for i in range(80)], np.uint8), q[200:]])
    case("i_run_80", 400, insert_80, 90)

    def d_then_x(w, flank):                                      # A CCCC G A in the window, A T A in the query: four deleted, one mismatch
        w[flank + 199: flank + 206] = [1, 2, 2, 2, 2, 3, 1]
    def d_then_x_query(q):
        q = np.concatenate([q[:200], q[204:]])
        q[200] = 4
        return q
    case("d_next_to_x", 400, d_then_x_query, 10, prep=d_then_x)

    # ranks 0 and 5: under '=' (window and query hold them alike), under X (against a letter), in a deleted and in an inserted stretch
    def ranks_prep(w, flank):
        w[flank + 40] = 5
        w[flank + 41] = 0
        free = sorted(set((1, 2, 3, 4)) - {int(w[flank + 119]), int(w[flank + 126])})
        w[flank + 120: flank + 126] = [free[0], 5, free[1], 0, free[0], free[1]]
    def ranks_query(q):
        free = sorted(set((1, 2, 3, 4)) - {int(q[219]), int(q[220])})
        ins = np.array([free[0], 5, 0, free[1]], np.uint8)
        return np.concatenate([q[:120], q[126:220], ins, q[220:]])
    def ranks_ref_edit(w, flank):
        w[flank + 80] = 5
        w[flank + 85] = 0
    case("ranks_0_5", 300, ranks_query, 20, prep=ranks_prep, ref_edit=ranks_ref_edit)

    # the pass carries: exactly 64, 65 and 129 words, and more than 4096
    case("words_65", 32 * 40 + 30, lambda q: sub(q, range(20, 32 * 40, 40)), 40)
    case("words_129", 64 * 30 + 25, lambda q: sub(q, range(15, 64 * 30, 30)), 80)
    def w64_prep(w, flank):
        d_then_x(w, flank)
    def w64_query(q):
        q = d_then_x_query(q)
        return sub(q, range(240, 240 + 30 * 40, 40))
    case("words_64", 1500, w64_query, 50, prep=w64_prep)
    case("words_4097", 30000, lambda q: sub(q, range(5, 30000, 12)), 2600)
    case("perfect", 2000, lambda q: q, 3)
    case("no_alignment", 200, lambda q: window(200), 3)
    case("exists_mode", 200, lambda q: sub(q, [50]), 3, mode=F.MODE_EXISTS)
    return pairs


def _eq_offsets(cs):
    """{run length: [offset of the run's first letter in the long string]}"""
    out, at = {}, 0
    for t in R.tokens(cs):
        if t[0] == "=":
            out.setdefault(len(t) - 1, []).append(at + 1)
        at += len(t)
    return out


CLASSES = {
    "first_last": lambda c, s, l: c.startswith("1I") and c.endswith("1X") and s.startswith(b"+"),
    "eq_runs_long": lambda c, s, l: all(f"{n}=" in c for n in (63, 64, 65, 2000)) and sorted(o % 4 for o in _eq_offsets(l)[65]) == [0, 1, 2, 3]
    and any(o % 2 for o in _eq_offsets(l)[65]),
    "eq_runs_short": lambda c, s, l: all(f":{n}*" in s.decode() for n in (9, 10, 99, 100, 999, 1000)),
    "x_run_80": lambda c, s, l: "80X" in c and re.search(rb"(\*ac){80}", s) is not None,
    "d_run_80": lambda c, s, l: "80D" in c and re.search(rb"-[acgt]{80}[:=]", s) is not None,
    "i_run_80": lambda c, s, l: "80I" in c and re.search(rb"\+[acgt]{80}[:=]", s) is not None,
    "d_next_to_x": lambda c, s, l: re.search(r"\d+D\d+X|\d+X\d+D", c) is not None and re.search(rb"-[a-z]+\*|\*[a-z]{2}-", s) is not None,
    "ranks_0_5": lambda c, s, l: re.search(rb"=[ACGT]*N[ACGT]*N|=[ACGT]*NN", l) is not None and re.search(rb"\*n[acgt]", s) is not None
    and re.search(rb"-[acgt]*n[acgt]*n", s) is not None and re.search(rb"\+[acgt]*nn", s) is not None,
    "words_64": lambda c, s, l: len(R.cigar_words(c)) == 64,
    "words_65": lambda c, s, l: len(R.cigar_words(c)) == 65,
    "words_129": lambda c, s, l: len(R.cigar_words(c)) == 129,
    "words_4097": lambda c, s, l: len(R.cigar_words(c)) > 4096,
    "perfect": lambda c, s, l: s == b":2000" and len(l) == 2001,
}


def _oracle_expect(pairs):
    """None | (nm, begin, cigar, short cs, long cs) of every pair, from the oracle's alignment"""
    out = []
    for name, w, q, k, mode in pairs:
        r = O.align(w, q, k)
        out.append(None if r is None else (r[0], r[1], r[2]) + tuple(R.cs_from_cigar(w, r[1], q, R.cigar_words(r[2]), long) for long in FORMS))
    return out


@pytest.fixture(scope="module")
def crafted():
    pairs = crafted_pairs()
    return pairs, _oracle_expect(pairs)


def test_crafted_pairs_cover_every_class_on_the_oracle(crafted):
    """What the crafted inputs exercise, from the oracle's own CIGARs (no GPU), and the rule's inverse on every pair: both sequences
    from the long string, the letters at X, I and D from the short one."""
    pairs, expect = crafted
    exp = dict(zip([p[0] for p in pairs], expect))
    for name, ok in CLASSES.items():
        assert exp[name] is not None, name
        assert ok(exp[name][2], exp[name][3], exp[name][4]), (name, exp[name][2][:120], exp[name][3][:120])
    assert exp["no_alignment"] is None and exp["exists_mode"] is not None
    for name, w, q, k, mode in pairs:
        if exp[name] is not None:
            nm, begin, cig, short, long = exp[name]
            R.check_inverse(short, w, begin, q, R.cigar_words(cig), False)
            R.check_inverse(long, w, begin, q, R.cigar_words(cig), True, true_path=True)
            rows = sum(x >> 4 for x in R.cigar_words(cig) if x & 15 != 2)
            assert len(short) <= R.slab_bound(nm, rows, False) and len(long) <= R.slab_bound(nm, rows, True), name


@pytest.fixture(scope="module")
def small_ctx():
    g = S.make_genome(100000, 1, seed=3)
    ctx = F.context(F.fmindex(g))
    yield ctx, g
    ctx.close()


def _batch_of(pairs):
    ref_pool = np.concatenate([p[1] for p in pairs])
    q_pool = np.concatenate([p[2] for p in pairs])
    jobs, ro, qo = [], 0, 0
    for name, w, q, k, mode in pairs:
        jobs.append((ro, len(w), qo, len(q), k, mode))
        ro += len(w)
        qo += len(q)
    return ref_pool, q_pool, jobs


@gpu
@pytest.mark.parametrize("long", FORMS)
def test_crafted_pairs_through_align_batch_cs(small_ctx, crafted, long):
    ctx, _ = small_ctx
    pairs, exp = crafted
    ref_pool, q_pool, jobs = _batch_of(pairs)
    got = F.align_batch_cs(ctx, q_pool, jobs, F.cs_options(long=long), reference_pool=ref_pool, md=True)
    plain = F.align_batch(ctx, q_pool, jobs, reference_pool=ref_pool, md=True)
    zeroed = F.align_batch_cs(ctx, q_pool, jobs, capi.CsOptions(), reference_pool=ref_pool, md=True)
    for (name, w, q, k, mode), g, p, z, e in zip(pairs, got, plain, zeroed, exp):
        if name == "no_alignment":
            assert g is None and p is None and z is None
        elif mode == F.MODE_EXISTS:
            assert g is not None and g[5] is None and g[:4] == p                  # no CIGAR, no MD, no cs (length 0)
        else:
            assert g[:4] == p and g[:3] == e[:3], name                             # records, CIGARs and MD are as without the option
            assert g[5] == e[4 if long else 3], (name, g[5][:80], e[4 if long else 3][:80])
            R.check_inverse(g[5], w, g[1], q, R.cigar_words(g[2]), long, true_path=True)
            assert z[:4] == p and z[5] is None
    # one pair at a time gives the same strings as the batch
    for (name, w, q, k, mode), g in list(zip(pairs, got))[:8]:
        (one,) = F.align_batch_cs(ctx, q, [(0, len(w), 0, len(q), k, mode)], F.cs_options(long=long), reference_pool=w)
        assert one[5] == g[5] and one[:3] == g[:3], name
    # the pool's capacity: what the call reports is what it needs
    L = capi.lib()
    import ctypes as C
    arr = (capi.AlignJob * len(jobs))(*[capi.AlignJob(ro, qo, rl, ql, k, mode) for ro, rl, qo, ql, k, mode in jobs])
    res = (capi.AlignResult * len(jobs))()
    cig = np.zeros(1 << 20, dtype=np.uint32)
    refs = (capi.MdRef * len(jobs))()
    need = None
    for cap, want in ((0, -3), (None, 0), (-1, -3)):
        cap = need if cap is None else need - 1 if cap == -1 else cap
        pool = np.zeros(max(1, cap), dtype=np.uint8)
        words, n = C.c_uint64(len(cig)), C.c_uint64(cap)
        rc = L.flx_align_batch_cs(ctx.h, capi.ptr(ref_pool, capi.u8p), len(ref_pool), capi.ptr(q_pool, capi.u8p), len(q_pool), arr, len(jobs), res,
                                  capi.ptr(cig, capi.u32p), C.byref(words), None, None, None, None, None, None, C.byref(F.cs_options(long=long)), refs,
                                  capi.ptr(pool, capi.u8p), C.byref(n))
        assert rc == want and (need is None or n.value == need)
        need = n.value
    assert need > 0


# ------------------------------------------------------------------------------------------------ 2. the kernel alone
def _kernel_cases():
    """paths for flx_cs_batch: the random paths of the host test, and words that cross every boundary of the kernel: runs of 64, 65 and
    300 letters of each kind, paths of 63, 64, 65, 128, 129 and 5000 words, a gap as the first word"""
    paths = random_paths(120, seed=31)
    rng = np.random.default_rng(32)

    def path(words, begin=3):
        cols = sum(w >> 4 for w in words if w & 15 != 1)
        rows = sum(w >> 4 for w in words if w & 15 != 2)
        return (rng.integers(0, 6, size=begin + cols + 2, dtype=np.uint8), begin, rng.integers(0, 6, size=rows + 1, dtype=np.uint8), words)
    for n in (64, 65, 300):
        paths.append(path([n << 4 | 7, n << 4 | 8, n << 4 | 1, n << 4 | 2, 5 << 4 | 7]))
        paths.append(path([1 << 4 | 1, n << 4 | 2, 1 << 4 | 8, n << 4 | 7]))
    for n_words in (63, 64, 65, 128, 129, 5000):
        paths.append(path([(1 + i % 7) << 4 | (7, 8, 7, 1, 7, 2)[i % 6] for i in range(n_words)]))
    return paths


@gpu
def test_kernel_alone_equals_the_host_rule_and_the_reference(small_ctx):
    ctx, genome = small_ctx
    paths = _kernel_cases()
    ref_pool, q_pool, words, jobs = pack_jobs(paths)
    for long in FORMS:
        host = F.cs_string(ref_pool, q_pool, words, jobs, long=long)
        dev = F.cs_batch(ctx, q_pool, words, jobs, long=long, reference_pool=ref_pool)
        assert dev == host
        for (ref, begin, qry, w), g in zip(paths, dev):
            assert g == R.cs_from_cigar(ref, begin, qry, w, long)
    # reference_pool=None: the context's text. The same jobs with windows in the genome (one sequence: text position = its position)
    text = genome[0]
    jobs_text, at = [], 1000
    for (co, cl, ro, rl, begin, qo, ql) in jobs:
        jobs_text.append((co, cl, at, rl, begin, qo, ql))
        at += rl + 7
    assert at < len(text)
    for long in FORMS:
        dev = F.cs_batch(ctx, q_pool, words, jobs_text, long=long)
        assert dev == F.cs_string(text, q_pool, words, jobs_text, long=long)
        for (ref, begin, qry, w), (co, cl, ro, rl, b, qo, ql), g in zip(paths, jobs_text, dev):
            assert g == R.cs_from_cigar(text[ro: ro + rl], begin, qry, w, long)
    # the capacity: equal to the need passes, one byte less does not
    raw_jobs = [(co, cl, 0, ro, rl, b, qo, ql, 0) for co, cl, ro, rl, b, qo, ql in jobs[:6]]
    L = capi.lib()
    for long in FORMS:
        want = F.cs_string(ref_pool, q_pool, words, jobs[:6], long=long)
        need = sum(len(s) for s in want)
        rc, n, _, got = _raw_cs(raw_jobs, words, ref_pool, q_pool, F.cs_options(long=long), cap=need, fn=L.flx_cs_batch, head=(ctx.h,))
        assert rc == 0 and n == need and got == want
        rc, n, err, _ = _raw_cs(raw_jobs, words, ref_pool, q_pool, F.cs_options(long=long), cap=need - 1, fn=L.flx_cs_batch, head=(ctx.h,))
        assert rc == -3 and n == need and "too small" in err
    # a bad job among good ones launches nothing
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_stats()
    with pytest.raises(F.FloxerError, match="do not fit"):
        F.cs_batch(ctx, q_pool, words, jobs[:5] + [(0, 3, 0, 2, 0, 0, 2)], reference_pool=ref_pool)
    assert "cs_build" not in ctx.kernel_stats()
    F.cs_batch(ctx, q_pool, words, jobs[:5], reference_pool=ref_pool)
    st = ctx.kernel_stats()["cs_build"]
    assert st["launches"] == 1 and st["work_units"] == sum(len(s) for s in F.cs_string(ref_pool, q_pool, words, jobs[:5]))
    ctx.enable_kernel_timing(False)


# ------------------------------------------------------------------------------------------------ 3. whole path
@pytest.fixture(scope="module")
def planted():
    chroms, reads = _planted()
    ctx = F.context(F.fmindex(chroms))
    oidx = O.Index(chroms)
    rows = oidx.run(reads, O.params(error_probability=RATE), threads=8).records()
    yield dict(chroms=chroms, reads=reads, ctx=ctx, oidx=oidx, rows=rows)
    ctx.close()


def record_cs(chroms, reads, row, long):
    """the rule on one record's own words: the oriented read from behind its left clip, the reference from POS"""
    read, flag, ref, pos, nm, cig = row
    if flag & 4:
        return None
    q = reads[read] if not flag & 16 else O.revcomp(reads[read])
    return R.cs_from_cigar(chroms[ref], pos, q[R.left_clip(cig):], R.cigar_words(cig), long)


def check_records(chroms, reads, rows, css, long, mds=None):
    """every record's string through the inverse against the sequences; with MD strings: both tags name the same reference letters under
    X and D"""
    for i, (row, cs) in enumerate(zip(rows, css)):
        read, flag, ref, pos, nm, cig = row
        if flag & 4:
            assert cs is None
            continue
        q = reads[read] if not flag & 16 else O.revcomp(reads[read])
        R.check_inverse(cs, chroms[ref], pos, q[R.left_clip(cig):], R.cigar_words(cig), long, true_path=True)
        if mds is not None:
            assert "".join(re.findall(r"[A-Z]", mds[i].decode())) == R.edits_from_cs(cs)[0], (read, flag, pos)


@gpu
@pytest.mark.parametrize("long", FORMS)
def test_whole_path_cs_is_the_rule_on_the_oracles_records(planted, long):
    chroms, reads, ctx, rows = planted["chroms"], planted["reads"], planted["ctx"], planted["rows"]
    want = [record_cs(chroms, reads, r, long) for r in rows]
    # not vacuous: both strands, an unmapped read, an insertion, a deletion of at least 2, adjacent X columns
    assert {r[1] & 16 for r in rows if not r[1] & 4} == {0, 16} and any(r[1] & 4 for r in rows)
    assert any(re.search(rb"\+[acgt]", s) for s in want if s) and any(re.search(rb"-[acgt]{2,}", s) for s in want if s)
    assert any(re.search(rb"(\*[acgt]{2}){2}", s) for s in want if s)
    p = F.params(error_probability=RATE)
    plain = F.aligner(ctx, p, md=True).align_reads(reads)
    assert plain.records() == rows and plain.cs is None
    got = F.aligner(ctx, p, md=True, cs=F.cs_options(long=long)).align_reads(reads)
    _same_records(got, plain)                                            # every other field, the CIGAR pool and `skipped`
    assert got.md == plain.md
    assert got.cs == want
    check_records(chroms, reads, rows, got.cs, long, got.md)
    # records that share a CIGAR share their cs bytes
    shared = {}
    for (coff, clen), (o, n) in zip(zip(got.raw["coff"], got.raw["clen"]), got.cs_refs):
        if clen:
            assert shared.setdefault((int(coff), int(clen)), (int(o), int(n))) == (int(o), int(n))
    # the kept records' strings are the full run's strings of the same records
    for drop, cap, mapq in [(True, 1, True), (True, 0, False), (False, 2, False)]:
        keep = restate(rows, drop, cap)
        sel = F.aligner(ctx, p, F.output_options(drop, cap, mapq), cs=F.cs_options(long=long)).align_reads(reads)
        assert sel.records() == [r for r, k in zip(rows, keep) if k], (drop, cap)
        assert sel.cs == [s for s, k in zip(want, keep) if k], (drop, cap)
        _same_records(sel, F.aligner(ctx, p, F.output_options(drop, cap, mapq)).align_reads(reads))
    # without MD the strings are the same
    assert F.aligner(ctx, p, cs=F.cs_options(long=long)).align_reads(reads).cs == want


@gpu
def test_resident_host_and_chunked_reads_and_an_image_context_give_the_same_strings(planted, monkeypatch):
    import torch
    chroms, reads = planted["chroms"], planted["reads"]
    reads = reads + S.make_reads(chroms, 60, 1500, READ_RATE, seed=55)[0]
    p = F.params(error_probability=RATE)
    idx = F.fmindex(chroms, device=0)
    light = F.fmindex.from_meta(idx.meta())                  # no arrays: the host holds no text
    image = [torch.empty(n, dtype=torch.uint8, device="cuda:0") for n in idx.image_layout()]
    idx.image_upload(0, [b.data_ptr() for b in image])
    ictx = F.context(light, image=image)
    for long in FORMS:
        al = F.aligner(planted["ctx"], p, cs=F.cs_options(long=long))
        host = al.align_reads(reads)
        rows = host.records()
        assert host.cs == [record_cs(chroms, reads, r, long) for r in rows]
        rr = F.resident_reads(planted["ctx"], reads)
        resident = al.align_reads(rr)
        rr.close()
        monkeypatch.setenv("FLX_CHUNK_READS", "9")          # many slices over the context's lanes: the offsets are rebased over the parts
        chunked = al.align_reads(reads)
        monkeypatch.delenv("FLX_CHUNK_READS")
        on_image = F.aligner(ictx, p, cs=F.cs_options(long=long)).align_reads(reads)
        for other_run in (resident, chunked, on_image):
            assert other_run.records() == rows and other_run.cs == host.cs
        assert (resident.cs_refs == host.cs_refs).all() and len(resident.cs_bytes) == len(host.cs_bytes)
        for lo, n in chunked.cs_refs:
            assert int(lo) + int(n) <= len(chunked.cs_bytes)
    ictx.close()


# ------------------------------------------------------------------------------------------------ 4. with the other stages
@gpu
@pytest.mark.parametrize("long", FORMS)
def test_left_aligned_and_realigned_runs_get_the_string_of_their_final_words(planted, long):
    chroms, reads, ctx = planted["chroms"], planted["reads"], planted["ctx"]
    p = F.params(error_probability=RATE)
    base = F.aligner(ctx, p).align_reads(reads).records()
    changed = 0
    for kw in (dict(gaps=F.gap_options()), dict(realign=F.realign_options()), dict(gaps=F.gap_options(), realign=F.realign_options())):
        off = F.aligner(ctx, p, md=True, **kw).align_reads(reads)
        got = F.aligner(ctx, p, md=True, cs=F.cs_options(long=long), **kw).align_reads(reads)
        _same_records(got, off)
        assert got.md == off.md
        rows = got.records()
        assert got.cs == [record_cs(chroms, reads, r, long) for r in rows], list(kw)
        check_records(chroms, reads, rows, got.cs, long, got.md)
        changed += sum(a[5] != b[5] for a, b in zip(rows, base))
    assert changed > 0                                                   # the stages in front did rewrite words


@pytest.fixture(scope="module")
def chimeric():
    from test_tails_gpu import RATE as TAIL_RATE, SPAN, build_batch
    chroms, reads, tailed, rescued = build_batch()
    ctx = F.context(F.fmindex(chroms))
    yield dict(chroms=chroms, reads=reads, tailed=tailed, rescued=rescued, ctx=ctx, rate=TAIL_RATE, span=SPAN)
    ctx.close()


@gpu
@pytest.mark.parametrize("long", FORMS)
def test_partial_extended_and_split_records_get_the_string_of_their_core(chimeric, long):
    c = chimeric
    chroms, reads, ctx = c["chroms"], c["reads"], c["ctx"]
    p = F.params(error_probability=c["rate"])
    for split in (None, F.split_options()):
        kw = dict(output=F.output_options(max_alignments=1, mapq=True), md=True, partial=F.partial_options(min_query_span=c["span"]),
                  extend=F.extend_options(), split=split)
        off = F.aligner(ctx, p, **kw).align_reads(reads)
        got = F.aligner(ctx, p, cs=F.cs_options(long=long), **kw).align_reads(reads)
        _same_records(got, off)
        assert got.md == off.md
        rows = got.records()
        # not vacuous: clipped records on both strands, supplementary ones among them, and with split a clipped primary
        clipped = [r for r in rows if "S" in r[5]]
        assert any(r[1] & 2048 for r in clipped) and any(R.left_clip(r[5]) > 0 for r in clipped)
        if split is not None:
            assert any(not r[1] & 2048 and r[0] in c["tailed"] for r in clipped)
        assert got.cs == [record_cs(chroms, reads, r, long) for r in rows]
        check_records(chroms, reads, rows, got.cs, long, got.md)


# ------------------------------------------------------------------------------------------------ 5. off is off
@gpu
def test_off_launches_nothing_and_a_run_without_mapped_records_neither(planted):
    import ctypes as C
    chroms, reads = planted["chroms"], planted["reads"]
    p = F.params(error_probability=RATE)
    L = capi.lib()
    stats = {}
    for name, cs in (("off", None), ("zeroed", capi.CsOptions()), ("short", F.cs_options()), ("long", F.cs_options(long=True))):
        c = F.context(F.fmindex(chroms))
        c.enable_kernel_timing(True)
        run = F.aligner(c, p, md=True, cs=cs).align_reads(reads)
        stats[name] = (c.kernel_stats(), run)
        if name == "short":
            # no mapped record: nothing to trace, no launch
            c.reset_kernel_stats()
            rng = np.random.default_rng(5)
            junk = [rng.integers(1, 5, size=1500, dtype=np.uint8) for _ in range(4)]
            none = F.aligner(c, p, cs=cs).align_reads(junk)
            assert all(r[1] & 4 for r in none.records()) and none.cs == [None] * 4 and "cs_build" not in c.kernel_stats()
        c.close()
    off, zeroed, short, long = (stats[n] for n in ("off", "zeroed", "short", "long"))
    assert "cs_build" not in off[0] and "cs_build" not in zeroed[0] and off[1].cs is None and zeroed[1].cs is None
    _same_records(off[1], zeroed[1])
    assert off[1].md == zeroed[1].md
    for on in (short, long):
        st = on[0]
        assert st["cs_build"]["launches"] == st["ed_traceback"]["launches"] == st["md_build"]["launches"]
        assert st["cs_build"]["algorithmic_bytes"] > 0 and st["cs_build"]["work_units"] > 0
        assert {n: k["launches"] for n, k in st.items() if n != "cs_build"} == {n: k["launches"] for n, k in off[0].items()}
    assert long[0]["cs_build"]["work_units"] > short[0]["cs_build"]["work_units"]
    # flx_run_copy_cs on a run made without the option
    pool = np.concatenate(reads[:6])
    offs = np.cumsum([0] + [len(r) for r in reads[:6]]).astype(np.uint64)
    counts = []
    for cs in (None, capi.CsOptions(), F.cs_options()):
        run = C.c_void_p()
        capi.check(L.flx_align_reads_cs(planted["ctx"].h, C.byref(p), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), 6, None, None, None, None,
                                        C.byref(cs) if cs is not None else None, C.byref(run)))
        counts.append((L.flx_run_num_records(run), L.flx_run_num_cs_bytes(run), L.flx_run_copy_cs(run, None, None)))
        L.flx_run_free(run)
    assert counts[0] == counts[1] and counts[0][1] == 0 and counts[0][2] == -1
    assert counts[2][0] == counts[0][0] and counts[2][1] > 0 and counts[2][2] == 0
    with pytest.raises(F.FloxerError, match="without_cigar"):
        F.aligner(planted["ctx"], F.params(error_probability=RATE, without_cigar=True), cs=F.cs_options()).align_reads(reads[:4])


# ------------------------------------------------------------------------------------------------ 6. CLI
@gpu
def test_cli_cs_tag_sam_and_bam(planted, tmp_path):
    chroms, rows_all = planted["chroms"], planted["rows"]
    reads = [r for r in planted["reads"] if len(r) > 100]
    fasta, fastq = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq")
    with open(fasta, "w") as f:
        for i, c in enumerate(chroms):
            f.write(f">chr{i} planted\n" + "\n".join(letters(c[o: o + 80]) for o in range(0, len(c), 80)) + "\n")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
    rows = O.Index(chroms).run(reads, O.params(error_probability=RATE), threads=8).records()
    exe = os.path.join(ROOT, "floxer_amd", "floxer")

    def run(out, *extra):
        cmd = [exe, "--reference", fasta, "--queries", fastq, "--output", out, "--error-probability", str(RATE), "--threads", "1", *extra]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
        return open(out, "rb").read()

    plain = [l for l in run(str(tmp_path / "plain.sam")).decode().splitlines() if not l.startswith("@")]
    plain_md = [l for l in run(str(tmp_path / "plain_md.sam"), "--md-tag").decode().splitlines() if not l.startswith("@")]
    plain_bam = bam_records(run(str(tmp_path / "plain.bam")))
    assert len(plain) == len(rows)
    for flag, long in (("--cs-tag", False), ("--cs-tag-long", True)):
        want = [record_cs(chroms, reads, r, long) for r in rows]
        body = [l.split("\t") for l in run(str(tmp_path / "cs.sam"), flag).decode().splitlines() if not l.startswith("@")]
        for f, l0, s in zip(body, plain, want):
            if f[2] == "*":
                assert "\t".join(f) == l0 and s is None                  # mapped records only
            else:
                assert f[-1] == "cs:Z:" + s.decode() and f[-2].startswith("NM:i:") and "\t".join(f[:-1]) == l0
        both = [l.split("\t") for l in run(str(tmp_path / "both.sam"), flag, "--md-tag").decode().splitlines() if not l.startswith("@")]
        assert ["\t".join(f[:-1]) if f[2] != "*" else "\t".join(f) for f in both] == plain_md
        assert [f[-1] for f in both if f[2] != "*"] == ["cs:Z:" + s.decode() for s in want if s]
        bam = bam_records(run(str(tmp_path / "cs.bam"), flag))
        assert [dict((t, v) for t, _, v in r["tags"]).get("cs") for r in bam] == want
        assert [dict(r, tags=[t for t in r["tags"] if t[0] != "cs"]) for r in bam] == plain_bam
        kept = run(str(tmp_path / "one.sam"), flag, "-D", "-N", "1", "-Q").decode().splitlines()
        keep = restate(rows, True, 1)
        assert [l.split("\t")[-1] for l in kept if not l.startswith("@") and "cs:Z:" in l] == ["cs:Z:" + s.decode() for s, k in zip(want, keep) if k and s]
    for extra in (["--cs-tag", "--cs-tag-long"], ["--cs-tag", "-w"], ["--cs-tag-long", "-w"]):
        r = subprocess.run([exe, "--reference", fasta, "--queries", fastq, "--output", str(tmp_path / "w.sam"), "-e", "2", *extra],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr, extra
