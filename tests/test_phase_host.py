"""Phasing without a GPU (flx_phase): the numpy reference against its own naive loop, flx_phase_host against the reference on random
records and on the special rows, a diploid sample made without the aligner, the ABI's sizes and names, the refusals, the parser and
the VCF reader of floxer_phase through its two switches, and tests/phase_check.cpp: the rule header against a column walk under
ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import phase_ref as R
import pileup_ref as P
from variants_ref import random_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "floxer_amd", "floxer_phase")
GOLDEN = os.path.join(ROOT, "tests", "golden")
w = R.word


def same(got, want):
    for g, x in zip(got, want):
        assert len(g) == len(x), (len(g), len(x))
        if g.tobytes() != x.tobytes():
            bad = next(i for i in range(len(g)) if g[i] != x[i])
            assert False, (bad, g[bad], x[bad])
    return got


def sites_from_records(rng, text, lengths, rec, words, reads, o, every=3, extra=20):
    """sites that the records can show: every `every`-th X column, I word and D word of the counted records becomes a site with the
    record's own allele (where the rule allows one), plus `extra` SNV sites anywhere; sorted, one per (position, kind)"""
    starts = R.starts_of(lengths)
    found = {}
    n = 0
    for r in R.counted(rec, o):
        seq = P.oriented(reads[int(r["read"])], r["flag"])
        ref = int(r["ref"])
        p, row = int(r["pos"]), 0
        for op, ln in R.words_of(r, words):
            n += 1
            a = int(starts[ref]) + p
            if n % every == 0:
                if op == 8 and 1 <= int(seq[row]) <= 4 and 1 <= int(text[a]) <= 4 and int(seq[row]) != int(text[a]):
                    found.setdefault((ref, p, R.SNV), (ref, p, R.SNV, int(seq[row]), 1, ()))
                elif op == 1 and p > int(r["pos"]) and ln <= 32 and all(1 <= int(x) <= 4 for x in seq[row: row + ln]):
                    found.setdefault((ref, p - 1, R.INS), (ref, p - 1, R.INS, 0, ln, [int(x) for x in seq[row: row + ln]]))
                elif op == 2 and p > int(r["pos"]):
                    found.setdefault((ref, p - 1, R.DEL), (ref, p - 1, R.DEL, 0, ln, ()))
            if op in (7, 8, 2):
                p += ln
            if op in (7, 8, 1, 4):
                row += ln
    for _ in range(extra):
        ref = int(rng.integers(0, len(lengths)))
        p = int(rng.integers(0, lengths[ref]))
        t = int(text[int(starts[ref]) + p])
        if 1 <= t <= 4:
            found.setdefault((ref, p, R.SNV), (ref, p, R.SNV, 1 + t % 4, 1, ()))
    return R.sites_of([found[k] for k in sorted(found)])


def special_rows():
    """records round one stretch of reference 0 (positions 100..), with the sites of SPECIAL_SITES: see test_phase_gpu's list of cases"""
    return [
        (0, 0, 100, 0, [w("=", 10), w("X", 1), w("=", 9)]),                             # SNV at 110: X
        (0, 0, 100, 0, [w("=", 20)]),                                                   # all REF; ends on 119: the indel site there is NONE
        (0, 0, 100, 0, [w("=", 11), w("D", 2), w("=", 7)]),                             # DEL of 2 behind 110
        (0, 0, 100, 0, [w("=", 11), w("D", 3), w("=", 6)]),                             # the right anchor, the wrong length
        (0, 0, 100, 0, [w("=", 11), w("I", 2), w("=", 9)]),                             # INS behind 110
        (16, 0, 100, 0, [w("=", 11), w("I", 2), w("=", 9)]),                            # the same on the other strand
        (0, 0, 100, 0, [w("=", 11), w("I", 2), w("D", 2), w("=", 7)]),                  # I and D side by side at one anchor
        (0, 0, 100, 0, [w("=", 11), w("D", 2), w("I", 2), w("=", 7)]),                  # an I word behind a D column: its anchor is 112
        (0, 0, 100, 0, [w("=", 5), w("D", 10), w("=", 5)]),                             # 110 inside a D word
        (0, 0, 111, 0, [w("=", 9)]),                                                    # starts behind 110: no slot for the sites there
        (0, 0, 100, 0, [w("S", 3), w("=", 11), w("X", 1), w("=", 8), w("S", 2)]),       # SNV at 111
        (0, 0, 110, 0, [w("X", 1), w("=", 9)]),                                         # the record's first column
        (0, 0, 101, 0, [w("=", 9), w("X", 1)]),                                         # the record's last column
        (0, 0, 130, 0, [w("=", 3)]),                                                    # no site at all
    ]


SPECIAL_SITES = [(0, 110, R.SNV, 0, 1, ()), (0, 110, R.DEL, 0, 2, ()), (0, 110, R.INS, 0, 2, (2, 4)), (0, 111, R.SNV, 0, 1, ()), (0, 112, R.INS, 0, 2, (2, 4)),
                 (0, 119, R.DEL, 0, 1, ()), (0, 119, R.INS, 0, 1, (3,))]


def special_batch(rng, copies=3):
    """(text, lengths, sites, records, words, reads): the special rows, `copies` of each with a read of its own; the X letters are the
    SNVs' alt or a third letter by turns, the I letters the site's (C T) or others by turns"""
    lengths = [400, 40]
    text = rng.integers(1, 5, size=sum(lengths)).astype(np.uint8)
    rec, words, reads = R.records_with_reads(rng, special_rows() * copies)
    alt = {p: 1 + int(text[p]) % 4 for p in (110, 111)}
    third = {p: next(x for x in range(1, 5) if x != int(text[p]) and x != alt[p]) for p in alt}
    sites = R.sites_of([(r, p, k, alt.get(p, 0) if k == R.SNV else 0, ln, le) for r, p, k, a, ln, le in SPECIAL_SITES])
    for i, r in enumerate(rec):
        seq = P.oriented(reads[i], r["flag"]).copy()
        seq[(seq == 0) | (seq == 5)] = 1
        p, row = int(r["pos"]), 0
        for op, ln in R.words_of(r, words):
            if op == 8:
                seq[row] = (alt if (i // len(special_rows())) % 2 == 0 else third).get(p, 1 + int(text[p]) % 4)
            if op == 1 and ln == 2:
                seq[row: row + 2] = (2, 4) if (i // len(special_rows())) % 3 != 2 else (2, 3)
            if op in (7, 8, 2):
                p += ln
            if op in (7, 8, 1, 4):
                row += ln
        reads[i] = P.oriented(seq, r["flag"])                           # (back to the read as given)
    return text, lengths, sites, rec, words, reads


def batches():
    rng = np.random.default_rng(20261021)
    out = []
    for case in range(10):
        lengths = [int(x) for x in rng.integers(30, 120, size=int(rng.integers(1, 4)))]
        rec, words = P.random_records(rng, lengths, 120 + 30 * case, max_words=12)
        reads = P.attach_reads(rng, rec, words)
        text = random_text(rng, sum(lengths))
        o = R.options(count_secondary=bool(case % 2), min_mapq=0 if case % 4 else 20, min_link=int(rng.integers(0, 4)), min_margin=int(rng.integers(0, 3)),
                      refine_rounds=int(rng.integers(0, 4)), skip_refine=case % 5 == 3)
        out.append((text, lengths, sites_from_records(rng, text, lengths, rec, words, reads, o), rec, words, reads, o))
    for o in (R.options(), R.options(min_link=1, skip_refine=True), R.options(min_link=3, min_margin=2, refine_rounds=3)):
        out.append(special_batch(rng) + (o,))
    return out


BATCHES = batches()


def test_reference_against_its_naive_loop():
    seen, phased, haps = set(), 0, set()
    for text, lengths, sites, rec, words, reads, o in BATCHES:
        want = R.phase(lengths, sites, rec, words, reads, o)
        same(R.phase_naive(lengths, sites, rec, words, reads, o), want)
        for r in R.counted(rec, o):
            seen |= {int(x) for x in R.observe(lengths, sites, r, words, reads)[1]}
        phased += int(want[0]["phased"].sum())
        haps |= {int(h) for h in want[1]["hap"]}
        assert len(want[1]) == len(R.counted(rec, o))
    assert seen == {R.REF, R.ALT, R.NONE} and phased > 20 and haps == {0, 1, 2}


def test_host_rule_equals_the_reference():
    kinds = set()
    for text, lengths, sites, rec, words, reads, o in BATCHES:
        same(F.phase_host(text, lengths, sites, rec, words, reads, R.c_options(o)), R.phase(lengths, sites, rec, words, reads, o))
        kinds |= {int(k) for k in sites["kind"]}
    assert kinds == {R.SNV, R.DEL, R.INS}


def test_the_special_rows_one_by_one():
    text, lengths, sites, rec, words, reads, o = BATCHES[-3]
    n = len(special_rows())
    obs = [R.observe(lengths, sites, r, words, reads) for r in rec[: 3 * n]]
    by_site = lambda j: dict(zip(range(obs[j][0], obs[j][0] + len(obs[j][1])), (int(x) for x in obs[j][1])))      # noqa: E731
    # sites: 0 SNV 110, 1 DEL 110 (2), 2 INS 110 (CT), 3 SNV 111, 4 INS 112 (CT), 5 DEL 119, 6 INS 119
    assert by_site(0) == {0: R.ALT, 1: R.REF, 2: R.REF, 3: R.REF, 4: R.REF, 5: R.NONE, 6: R.NONE}      # X with the alt; the indel sites on the last column are NONE
    assert by_site(n)[0] == R.NONE                                       # X with a third letter
    assert by_site(1) == {0: R.REF, 1: R.REF, 2: R.REF, 3: R.REF, 4: R.REF, 5: R.NONE, 6: R.NONE}
    assert by_site(2) == {0: R.REF, 1: R.ALT, 2: R.NONE, 3: R.NONE, 4: R.NONE, 5: R.NONE, 6: R.NONE}   # 111, 112 are D columns; 112 has an = behind: empty E, a D column
    assert by_site(3)[1] == R.NONE and by_site(3)[2] == R.NONE           # the right anchor and the wrong length
    assert by_site(4)[2] == R.ALT and by_site(4)[1] == R.NONE and by_site(5)[2] == R.ALT      # both strands
    assert by_site(2 * n + 4)[2] == R.NONE                               # the right length and other letters
    assert by_site(6)[1] == R.ALT and by_site(6)[2] == R.ALT             # I and D side by side
    assert by_site(7)[1] == R.ALT and by_site(7)[2] == R.NONE and by_site(7)[4] == R.ALT      # an I word behind a D column
    assert by_site(8)[0] == R.NONE and by_site(8)[1] == R.NONE           # inside a D word
    assert set(by_site(9)) == {3, 4, 5, 6} and by_site(9)[3] == R.REF and by_site(9)[4] == R.REF
    assert by_site(10)[3] == R.ALT and by_site(10)[0] == R.REF
    assert by_site(11)[0] == R.ALT and by_site(12)[0] == R.ALT and set(by_site(12)) == {0, 1, 2}
    assert by_site(12)[1] == R.NONE                                      # an indel site on the record's last column
    assert by_site(13) == {}


# ------------------------------------------------------------------------------------------------ a diploid sample without the aligner
# The reference alone was run on seeds 0..7 at both error rates. All eight hold the three caps at both (exactly two phase sets and no
# unphased site among 21 to 27; every p the planted haplotype up to one constant per set; no record with |h1 - h2| >= 2 on the wrong
# haplotype), seed 0 at 0.08 included, where a prototype on simulated observations had shown one such record. What the cap leaves
# out, records tagged to the wrong haplotype by a margin of 1: none or one of about 425 tagged at 0.02, one to five of about 413 at
# 0.08 (seeds 0..7: 2 3 3 5 4 1 1 2).
SAMPLE_SEED = 1


def diploid_sample(rate, seed=SAMPLE_SEED):
    """12 kb of reference; het SNVs 150 to 700 apart, each on a randomly chosen haplotype, with one stretch of 1300 positions without a
    site (longer than a read); a het deletion of three bases and a het insertion of two; reads over 1000 reference positions from each
    haplotype start every 50 positions, with substitution errors at `rate`; the CIGARs are written here from the truth. Returns (text,
    sites, records, words, reads, hap_of_site, hap_of_record)."""
    rng = np.random.default_rng(seed)
    text = rng.integers(1, 5, size=12_000).astype(np.uint8)
    positions, p = [], 400
    while p < 11_500:
        positions.append(p)
        p += int(rng.integers(150, 701)) if not 5000 <= p < 5700 or len([q for q in positions if q > 5000]) != 1 else 1300
    del_anchor, ins_anchor = positions[3], positions[-4]
    snvs = [q for q in positions if q not in (del_anchor, ins_anchor)]
    hap_of = {q: int(rng.integers(0, 2)) for q in positions}             # the haplotype that carries the ALT
    alt = {q: 1 + (int(text[q]) + int(rng.integers(0, 3))) % 4 for q in snvs}
    ins_letters = (2, 4)
    rows, reads, hap_of_record = [], [], []
    for hap in (0, 1):
        for start in range(0, 11_001, 50):
            ops, letters = [], []
            for q in range(start, start + 1000):
                if hap == hap_of[del_anchor] and del_anchor < q <= del_anchor + 3:
                    ops.append("D")
                    continue
                true = alt[q] if q in alt and hap == hap_of[q] else int(text[q])
                seen = 1 + (true + int(rng.integers(0, 3))) % 4 if rng.random() < rate else true
                ops.append("=" if seen == int(text[q]) else "X")
                letters.append(seen)
                if q == ins_anchor and hap == hap_of[ins_anchor] and q + 1 < start + 1000:
                    for x in ins_letters:
                        ops.append("I")
                        letters.append(x)
            while ops[-1] == "D":                                        # (a record does not end on a deletion)
                ops.pop()
            ws, k = [], 0
            while k < len(ops):
                e = k
                while e < len(ops) and ops[e] == ops[k]:
                    e += 1
                ws.append(w(ops[k], e - k))
                k = e
            flag = 16 if (start // 50 + hap) % 2 else 0
            rows.append((flag, 0, start, 0, ws))
            seq = np.array(letters, dtype=np.uint8)
            reads.append(P.COMPLEMENT[seq[::-1]] if flag else seq)
            hap_of_record.append(hap)
    rec, words = R.records_of(rows)
    rec["read"] = np.arange(len(rec))
    site_rows = [(0, q, R.SNV, alt[q], 1, ()) for q in snvs] + [(0, del_anchor, R.DEL, 0, 3, ()), (0, ins_anchor, R.INS, 0, 2, ins_letters)]
    site_rows.sort()
    return text, R.sites_of(site_rows), rec, words, reads, [hap_of[q] for _, q, *_ in site_rows], hap_of_record


def planted_truth_holds(sites, res, tags, hap_of_site, hap_of_record, n_sets):
    """exactly n_sets phase sets, every site in one; p is the planted haplotype up to one constant per set; no record with
    |h1 - h2| >= 2 tagged to the wrong haplotype (each cap 0). Returns the number of tagged records."""
    assert int(res["phased"].sum()) == len(sites) and len(set(int(s) for s in res["phase_set"])) == n_sets, sorted(set(int(s) for s in res["phase_set"]))
    const = {}
    for i, r in enumerate(res):
        c = int(r["phase"]) ^ hap_of_site[i]                             # p = 0: ALT on haplotype 1
        assert const.setdefault(int(r["phase_set"]), c) == c, (i, r)
    wrong = tagged = 0
    for t, hap in zip(tags, hap_of_record):
        if int(t["hap"]) == 0:
            continue
        tagged += 1
        mine = (int(t["hap"]) - 1) ^ const[int(t["phase_set"])]
        if mine != hap and abs(int(t["h1"]) - int(t["h2"])) >= 2:
            wrong += 1
    assert wrong == 0, wrong
    return tagged


@pytest.mark.parametrize("rate", [0.02, 0.08])
def test_a_diploid_sample_made_without_the_aligner(rate):
    text, sites, rec, words, reads, hap_of_site, hap_of_record = diploid_sample(rate)
    assert {R.SNV, R.DEL, R.INS} == {int(k) for k in sites["kind"]} and 20 < len(sites) < 80 and {0, 1} == set(hap_of_site)
    gaps = np.diff(sites["pos"].astype(np.int64))
    assert int(gaps.max()) > 1000 and sorted(gaps)[-2] <= 700 and int(gaps.min()) >= 150
    want = R.phase([12_000], sites, rec, words, reads, R.options())
    res, tags = same(F.phase_host(text, [12_000], sites, rec, words, reads), want)
    tagged = planted_truth_holds(sites, res, tags, hap_of_site, hap_of_record, 2)
    assert tagged > 0.9 * len(rec) and {0, 16} == {int(f) for f in rec["flag"]}


# ------------------------------------------------------------------------------------------------ the ABI
def test_symbols_sizes_and_python_names():
    L = capi.lib()
    names = [n for n in capi.EXPORTED if n.startswith("flx_phase_")]
    header = open(os.path.join(ROOT, "include", "floxer_amd.h")).read()
    assert set(names) == {n for n in re.findall(r"\b(flx_[a-z0-9_]+)\s*\(", header) if n.startswith("flx_phase_")}
    for name in names:
        getattr(L, name)
    assert set(names) == {"flx_phase_create", "flx_phase_create_for_text", "flx_phase_free", "flx_phase_add_records", "flx_phase_add_run", "flx_phase_add_run_resident",
                          "flx_phase_finish", "flx_phase_num_sites", "flx_phase_copy_results", "flx_phase_num_tags", "flx_phase_copy_tags", "flx_phase_geometry", "flx_phase_host"}
    assert [C.sizeof(s) for s in (capi.PhaseOptions, capi.PhaseSite, capi.PhaseResult, capi.PhaseTag)] == [32, 32, 32, 32]
    for dtype, struct in ((F.PHASE_SITE_DTYPE, capi.PhaseSite), (F.PHASE_RESULT_DTYPE, capi.PhaseResult), (F.PHASE_TAG_DTYPE, capi.PhaseTag)):
        assert dtype.itemsize == 32 and [dtype.fields[n][1] for n in dtype.names] == [getattr(struct, f[0]).offset for f in struct._fields_]
    o = F.phase_options(count_secondary=True, min_mapq=7, min_link=3, min_margin=2, refine_rounds=4, skip_refine=True)
    assert (o.count_secondary, o.min_mapq, o.min_link, o.min_margin, o.refine_rounds, o.skip_refine, list(o.reserved)) == (1, 7, 3, 2, 4, 1, [0, 0])
    cap, waves, tile, longest = F.phase_geometry()
    assert cap >= 1 and waves == 4 and tile == 4096 and longest == 32
    for name in ("phase", "phase_options", "phase_host", "phase_geometry", "phase_sites_from_rows"):
        assert hasattr(F, name)
    for method in ("add_records", "add", "finish", "results", "tags", "close"):
        assert callable(getattr(F.phase, method))
    rows = np.zeros(3, dtype=F.VARIANT_DTYPE)
    rows["gt"], rows["pos"], rows["kind"], rows["alt_rank"], rows["length"], rows["letters"] = [1, 2, 1], [5, 6, 7], [0, 0, 2], [3, 2, 0], [1, 1, 2], [0, 0, R.pack((2, 4))]
    sites = F.phase_sites_from_rows(rows)
    assert sites.tobytes() == R.sites_of([(0, 5, R.SNV, 3, 1, ()), (0, 7, R.INS, 0, 2, (2, 4))]).tobytes()
    with pytest.raises(F.FloxerError):                                   # no device: the host form is phase_host
        F.phase(text=[np.ones(5, dtype=np.uint8)], sites=[], device=-1)


def test_refusals_of_the_host_rule():
    rng = np.random.default_rng(9)
    text = np.array([1, 2, 3, 4] * 15, dtype=np.uint8)
    text[30], text[31] = 0, 5
    rec, words, reads = R.records_with_reads(rng, [(0, 0, 3, 0, [w("=", 20), w("I", 2), w("X", 3), w("D", 2), w("=", 1)])] * 4)
    run = lambda sites, o=None, lengths=(60,): F.phase_host(text, list(lengths), sites, rec, words, reads, o)      # noqa: E731
    site = lambda **kw: np.array([tuple(dict(dict(ref=0, pos=10, kind=0, alt_rank=1, length=1, reserved=0, letters=0), **kw)[k] for k in F.PHASE_SITE_DTYPE.names)],      # noqa: E731
                                 dtype=F.PHASE_SITE_DTYPE)
    run(site())                                                          # text[10] = 3, alt 1
    bad_sites = [site(alt_rank=3), site(alt_rank=0), site(alt_rank=5), site(pos=30), site(pos=31), site(pos=60), site(ref=1), site(ref=-1), site(kind=3), site(reserved=1),
                 site(letters=1 << 62), site(kind=1, length=0), site(kind=1, pos=57, length=3), site(kind=1, length=2, letters=1), site(kind=2, length=0), site(kind=2, length=33),
                 site(kind=2, length=2, letters=1 << 56), np.concatenate([site(pos=12), site(pos=11)]), np.concatenate([site(), site()]),
                 np.concatenate([site(kind=1, length=1), site()])]
    for s in bad_sites:
        with pytest.raises(F.FloxerError, match="site"):
            run(s)
    for s in (site(kind=1, pos=57, length=2), site(kind=2, length=32, letters=(1 << 64) - 1), site(kind=2, length=2, letters=3 << 60),
              np.concatenate([site(), site(kind=1, length=1), site(kind=2, length=1)])):
        run(s)
    bad = capi.PhaseOptions()
    bad.reserved[1] = 1
    for o in (bad, F.phase_options(refine_rounds=9)):
        with pytest.raises(F.FloxerError, match="flx_phase_options"):
            run(site(), o)
    run(site(), F.phase_options(refine_rounds=8, min_link=1 << 31, min_margin=1 << 31))
    with pytest.raises(F.FloxerError, match="rank above 5"):
        F.phase_host(np.full(60, 6, dtype=np.uint8), [60], site(), rec, words, reads)
    # everything pileup_plan refuses: past the end, a sequence that is not there, an M word, no reference-consuming column, no word
    for rows in ([(0, 0, 50, 0, [w("=", 11)])], [(0, 1, 0, 0, [w("=", 1)])], [(0, 0, 0, 0, [w("M", 5)])], [(0, 0, 0, 0, [w("S", 5), w("I", 1)])], [(0, 0, 0, 0, [])]):
        rec2, words2, reads2 = R.records_with_reads(rng, [(0, 0, 3, 0, [w("=", 20)])] * 2 + rows)
        with pytest.raises(F.FloxerError):
            F.phase_host(text, [60], site(), rec2, words2, reads2)
    rec2, words2, reads2 = R.records_with_reads(rng, [(0, 0, 3, 0, [w("=", 20)])] * 2)
    with pytest.raises(F.FloxerError):                                   # the query-consuming lengths and the read disagree
        F.phase_host(text, [60], site(), rec2, words2, [reads2[0], reads2[1][:-1]])
    rec2["read"][1] = 2
    with pytest.raises(F.FloxerError, match="read_index"):
        F.phase_host(text, [60], site(), rec2, words2, reads2)
    res, tags = F.phase_host(text, [60], site()[:0], rec, words, reads)  # no site: no result, a tag per record
    assert len(res) == 0 and len(tags) == 4 and int(tags["n_slots"].sum()) == 0 and set(int(x) for x in tags["phase_set"]) == {R.NO_SET}


# ------------------------------------------------------------------------------------------------ the tool's parser and its VCF reader
def tool(*args, switch="FLX_PHASE_PARSE_ONLY"):
    env = dict(os.environ, **{switch: "1"})                             # no device is touched, nothing is written
    return subprocess.run([TOOL] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def parsed(*args):
    r = tool(*args)
    assert r.returncode == 0 and r.stdout == b"" and b"CLI PARSER ERROR" not in r.stderr, (args, r.stderr)
    return dict(l.split("=", 1) for l in r.stderr.decode().splitlines())


VCF_HEAD = "##fileformat=VCFv4.2\n##source=floxer_variants\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"


def test_tool_parser(tmp_path):
    ref, reads = os.path.join(GOLDEN, "reference.fasta"), os.path.join(GOLDEN, "queries.fastq")
    calls, out, tsv = str(tmp_path / "calls.vcf"), str(tmp_path / "phased.vcf"), str(tmp_path / "tags.tsv")
    open(calls, "w").write(VCF_HEAD)
    base = ["--reference", ref, "--queries", reads, "--variants", calls, "--output", out]
    h = subprocess.run([TOOL, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0 and h.stdout == b""
    lines = h.stderr.decode().splitlines()
    names = ("reference", "queries", "variants", "output", "haplotags", "query-errors", "error-probability", "device", "min-link", "min-tag-margin", "refine-rounds", "no-refine",
             "secondary", "min-mapq", "realign-affine", "batch-reads")
    for name in names:
        assert len([l for l in lines if re.search(rf"^\s+(-\w, )?--{name}(\s|$)", l)]) == 1, name
    assert len(lines) == 1 + len(names) and lines[0].startswith("floxer_phase")
    d = parsed(*base, "--error-probability", "0.08")
    assert (d["min-link"], d["min-tag-margin"], d["refine-rounds"], d["no-refine"], d["secondary"], d["min-mapq"], d["realign-affine"], d["batch-reads"], d["device"], d["output"],
            d["variants"], d["haplotags"], d["error-probability"]) == ("0", "0", "0", "0", "0", "0", "0", "16384", "0", out, calls, "", "0.08")
    d = parsed(*base, "-p", "0.05", "--haplotags", tsv, "--min-link", "3", "--min-tag-margin", "2", "--refine-rounds", "8", "--secondary", "--min-mapq", "5", "--realign-affine",
               "--batch-reads=9", "--device", "1")
    assert (d["haplotags"], d["min-link"], d["min-tag-margin"], d["refine-rounds"], d["secondary"], d["min-mapq"], d["realign-affine"], d["batch-reads"], d["device"]) == \
        (tsv, "3", "2", "8", "1", "5", "1", "9", "1")
    assert parsed(*base, "-e", "3", "--no-refine")["no-refine"] == "1"
    bad = ([], ["-e", "1"], ["-p", "1"], ["-p", "x"], ["-p", "0.05", "--device", "1024"], ["-p", "0.05", "--min-link", "0"], ["-p", "0.05", "--min-tag-margin", "0"],
           ["-p", "0.05", "--refine-rounds", "0"], ["-p", "0.05", "--refine-rounds", "9"], ["-p", "0.05", "--no-refine", "--refine-rounds", "2"], ["-p", "0.05", "--min-mapq", "255"],
           ["-p", "0.05", "--batch-reads", "0"], ["-p", "0.05", "--min-link"], ["-p", "0.05", "--sam"], ["-p", "0.05", "--sample", "S"], ["-p", "0.05", "stray"],
           ["-p", "0.05", "--haplotags", str(tmp_path / "tags.txt")])
    for extra in bad:
        r = tool(*base, *extra)
        assert r.returncode == 255 and r.stderr.startswith(b"[CLI PARSER ERROR]\n") and r.stdout == b"", (extra, r.stderr)
    link = str(tmp_path / "link.vcf")
    os.symlink(calls, link)
    for args, what in ((base[2:] + ["-p", "0.05"], b"-r/--reference is required"), (base[:2] + base[4:] + ["-p", "0.05"], b"-q/--queries is required"),
                       (base[:4] + base[6:] + ["-p", "0.05"], b"-v/--variants is required"), (base[:6] + ["-p", "0.05"], b"-o/--output is required"),
                       (base[:6] + ["--output", str(tmp_path / "phased.bcf"), "-p", "0.05"], b"[vcf]"), (base[:6] + ["--output", str(tmp_path / "phased.vcf.gz"), "-p", "0.05"], b"[vcf]"),
                       (base[:4] + ["--variants", str(tmp_path / "none.vcf"), "--output", out, "-p", "0.05"], b"does not exist"),
                       (base[:4] + ["--variants", reads, "--output", out, "-p", "0.05"], b"-v/--variants"),
                       (base[:6] + ["--output", calls, "-p", "0.05"], b"the output is the input"), (base[:6] + ["--output", link, "-p", "0.05"], b"the output is the input"),
                       (base, b"Either a fixed number of errors"), (base + ["-e", "1"], b"PEX tree leaves")):
        r = tool(*args)
        assert r.returncode == 255 and r.stderr.startswith(b"[CLI PARSER ERROR]\n") and what in r.stderr, (args, r.stderr)
    assert sorted(os.listdir(tmp_path)) == ["calls.vcf", "link.vcf"]


def test_tool_vcf_reader(tmp_path):
    """which lines are sites and which pass through, and what is refused, on small files written here over the golden reference"""
    reads = os.path.join(GOLDEN, "queries.fastq")
    rng = np.random.default_rng(3)
    names, seqs = ["chrA", "chrB"], ["".join("ACGT"[x] for x in rng.integers(0, 4, size=n)) for n in (200, 60)]
    (tmp_path / "in").mkdir()
    (tmp_path / "out").mkdir()
    ref = str(tmp_path / "in" / "ref.fa")
    open(ref, "w").write("".join(f">{n} a contig\n{q}\n" for n, q in zip(names, seqs)))
    chrom, s = names[0], seqs[0]
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    fmt = "GT:GQ:DP:AD:PL"
    smp = lambda gt: f"{gt}:50:20:10,10:100,0,100"                        # noqa: E731
    row = lambda pos, r, a, f=fmt, sample=None, gt="0/1": f"{chrom}\t{pos}\t.\t{r}\t{a}\t50.00\t.\tDP=20\t{f}\t{sample if sample is not None else smp(gt)}\n"      # noqa: E731
    ins33 = s[79] + "ACGT" * 8 + "A"
    body = [row(11, s[10], other[s[10]]),                                # SNV site
            row(11, s[10:13], s[10]),                                    # a deletion of two behind the same position: a site behind the SNV
            row(11, s[10], s[10] + "CT", gt="1/0"),                      # an insertion: a site, GT 1/0
            row(21, s[20], other[s[20]], gt="1/1"),                      # homozygous: passes through
            row(31, s[30], other[s[30]] + "," + other[other[s[30]]], gt="1/2"),      # multi-allelic
            row(41, s[40], "<DEL>"), row(51, s[50], "*"),                # symbolic and * alleles
            row(61, s[60], other[s[60]], f="DP", sample="20"),           # no GT
            row(71, s[70], other[s[70]], gt="0|1"),                      # phased already: not 0/1
            row(80, s[79], ins33),                                       # an insertion of 33 letters
            row(81, s[80], s[80] + "ACGT" * 8),                          # an insertion of 32: a site
            row(91, s[90:93], s[90] + "G"),                              # a replacement: no form floxer_variants writes
            row(101, s[100], other[s[100]].lower()),                     # lower case: passes through
            f"{chrom}\t111\t.\t{s[110]}\t{other[s[110]]}\t50.00\t.\tDP=20\n",        # eight columns: no sample
            row(121, s[120], other[s[120]], f="GT:PS", sample="0/1:7").rstrip("\n") + "\t1/1:9\r\n"]      # a second sample, a PS field, a CR LF
    calls = str(tmp_path / "in" / "calls.vcf")
    base = ["--reference", ref, "--queries", reads, "--variants", calls, "--output", str(tmp_path / "out" / "phased.vcf"), "-p", "0.05"]
    open(calls, "w", newline="").write(VCF_HEAD + "".join(body))
    r = tool(*base, switch="FLX_PHASE_SITES_ONLY")
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    got = [dict(f.split("=") for f in l.split()[1:]) for l in r.stderr.decode().splitlines() if l.startswith("site ")]
    lines = (VCF_HEAD + "".join(body)).splitlines(keepends=True)
    at, sites = R.vcf_sites(lines, names)
    assert [int(g["line"]) - 1 for g in got] == at == [3, 4, 5, 13, 17]
    assert [(int(g["ref"]), int(g["pos"]), int(g["kind"]), int(g["alt"]), int(g["length"]), int(g["letters"], 16)) for g in got] == \
        [(int(x["ref"]), int(x["pos"]), int(x["kind"]), int(x["alt_rank"]), int(x["length"]), int(x["letters"])) for x in sites]
    assert b"ps-header=0" in r.stderr
    # the reference of the output on these lines: everything but the sites passes through, the PS header goes in front of #CHROM
    res = np.zeros(5, dtype=F.PHASE_RESULT_DTYPE)
    res["phase_set"], res["phased"], res["phase"] = [0, 0, 0, 3, 4], [1, 1, 1, 0, 0], [0, 1, 0, 0, 0]
    out = R.vcf_lines(lines, names, res)
    assert out[2] == R.PS_HEADER and len(out) == len(lines) + 1 and [o for i, o in enumerate(out[:2] + out[3:]) if i not in at] == [l for i, l in enumerate(lines) if i not in at]
    assert out[4].endswith(f"\t{fmt}:PS\t1|0:50:20:10,10:100,0,100:11\n") and out[5].endswith(":PS\t0|1:50:20:10,10:100,0,100:11\n") and out[6].split("\t")[9].startswith("1|0:")
    assert out[14].endswith(f"\t{fmt}:PS\t0/1:50:20:10,10:100,0,100:.\n") and out[18].endswith("\tGT:PS\t0/1:.\t1/1:.\r\n")
    open(calls, "w").write("##FORMAT=<ID=PS,Number=1,Type=Integer,Description=\"x\">\n" + VCF_HEAD + body[0])
    assert b"ps-header=1" in tool(*base, switch="FLX_PHASE_SITES_ONLY").stderr
    # refused as an input error, nothing written
    refused = {"unknown contig": [row(11, s[10], other[s[10]]).replace(chrom, "chrNone", 1)], "out of order": [body[3], body[0]], "one position": [body[1], body[0]],
               "REF": [row(11, other[s[10]], s[10])], "REF of a line that passes through": [row(21, other[s[20]], s[20], gt="1/1")], "POS": [row(0, s[0], other[s[0]])],
               "behind the contig": [row(len(s), s[-1] + "A", s[-1])], "columns": [f"{chrom}\t11\t.\n"]}
    refused["contigs out of order"] = [row(11, seqs[1][10], other[seqs[1][10]]).replace(chrom, names[1], 1), body[0]]
    for what, rows in refused.items():
        open(calls, "w").write(VCF_HEAD + "".join(rows))
        r = tool(*base, switch="FLX_PHASE_SITES_ONLY")
        assert r.returncode == 255 and b"error" in r.stderr and b"calls.vcf" in r.stderr and r.stdout == b"", (what, r.stderr)
    open(calls, "w").write("##fileformat=VCFv4.2\n" + body[0])
    assert tool(*base, switch="FLX_PHASE_SITES_ONLY").returncode == 255   # no #CHROM line
    assert os.listdir(tmp_path / "out") == [] and sorted(os.listdir(tmp_path / "in")) == ["calls.vcf", "ref.fa"]


def test_rule_header_against_a_column_walk_under_sanitizers(tmp_path):
    """tests/phase_check.cpp: flx_phase.hpp on random records, built with ASan + UBSan; nothing is preloaded"""
    exe = str(tmp_path / "phase_check")
    src = os.path.join(ROOT, "tests", "phase_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
