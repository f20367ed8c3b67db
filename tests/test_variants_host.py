"""Variant calls without a GPU (flx_variants): the numpy reference against its own naive loop, flx_variants_host against the reference on
random records and on pileup's special rows, the genotype function at its boundaries, a diploid sample made without the aligner, the
ABI's sizes and names, the refusals, the parser and the cost derivation of floxer_variants through its parse-only switch, and
tests/variants_check.cpp: the rule header against a column walk under ASan + UBSan."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import variants_ref as R
import pileup_ref as P
from test_pileup_gpu import special_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "floxer_amd", "floxer_variants")
GOLDEN = os.path.join(ROOT, "tests", "golden")
U32 = (1 << 32) - 1


def same(got, want):
    assert len(got[1]) == len(want[1]) and got[1].tobytes() == want[1].tobytes(), (got[1][:5], want[1][:5])
    assert len(got[0]) == len(want[0]) and got[0].tobytes() == want[0].tobytes(), (got[0][:5], want[0][:5])
    return got


def batches():
    """(text, lengths, records, words, reads, options): random records at several depths, thresholds and costs, then pileup's special rows"""
    rng = np.random.default_rng(20261021)
    out = []
    for case in range(12):
        lengths = [int(x) for x in rng.integers(1, 90, size=int(rng.integers(1, 4)))]
        rec, words = P.random_records(rng, lengths, 80 + 40 * case)
        reads = P.attach_reads(rng, rec, words)
        costs = dict(cost_match=int(rng.integers(1, 60)), cost_het=int(rng.integers(60, 400)), cost_mismatch=int(rng.integers(400, 3000))) if case % 3 == 1 else {}
        priors = dict(prior_het=int(rng.integers(1, 4000)), prior_hom=int(rng.integers(1, 4000))) if case % 4 == 2 else {}
        o = R.options(count_secondary=bool(case % 2), min_mapq=0 if case % 4 else 20, min_depth=int(rng.integers(0, 5)), min_qual=int(rng.integers(0, 3)) * int(rng.integers(1, 1500)),
                      max_del=int(rng.integers(0, 5)), **costs, **priors)
        out.append((R.random_text(rng, sum(lengths)), lengths, rec, words, reads, o))
    lengths = [700, 40]
    rec, words, reads = R.records_with_reads(rng, special_rows() * 3)       # three copies of each, each with a read of its own
    for o in (R.options(), R.options(min_depth=1, min_qual=1), R.options(min_depth=2, min_qual=300, max_del=70, prior_het=100, prior_hom=100)):
        out.append((R.random_text(rng, sum(lengths)), lengths, rec, words, reads, o))
    return out


BATCHES = batches()


def test_reference_against_its_naive_loop():
    n_rows, kinds, gts = 0, set(), set()
    for text, lengths, rec, words, reads, o in BATCHES:
        rows, al = R.variants(text, lengths, rec, words, reads, o)
        cnt = P.counts(lengths, rec, words, reads, o)
        assert (cnt == P.counts_naive(lengths, rec, words, reads, o)).all()
        assert R.call_naive(text, lengths, cnt, al, o).tobytes() == rows.tobytes()
        n_rows += len(rows)
        kinds |= {int(k) for k in rows["kind"]}
        gts |= {int(g) for g in rows["gt"]}
        order = [(int(r["ref"]), int(r["pos"]), int(r["kind"]) != R.SNV) for r in rows]
        assert order == sorted(order) and len(set(order)) == len(order)   # position order, the SNV first, two rows per position at most
    assert n_rows > 50 and kinds == {R.SNV, R.DEL, R.INS} and gts == {R.RA, R.AA}


def test_host_rule_equals_the_reference():
    kinds = set()
    for text, lengths, rec, words, reads, o in BATCHES:
        want = R.variants(text, lengths, rec, words, reads, o)
        same(F.variants_host(text, lengths, rec, words, reads, R.c_options(o)), want)
        kinds |= {int(k) for k in want[0]["kind"]}
    assert kinds == {R.SNV, R.DEL, R.INS}


# ------------------------------------------------------------------------------------------------ the genotype at its boundaries
def genotype(ref_n, alt_n, oth, **o):
    """the library's genotype, which the reference's must equal; plus the reference's L"""
    got = F.variants_genotype(ref_n, alt_n, oth, F.variants_options(**o) if o else None)
    want = R.genotype(ref_n, alt_n, oth, R.model(R.options(**o)))
    assert (got["gt"], got["gq"], got["qual"], got["pl"]) == (want["gt"], want["gq"], want["qual"], want["pl"])
    assert got["row"] == R.makes_row(want, ref_n + alt_n + oth, R.model(R.options(**o)))
    return dict(got, L=want["L"])


def test_the_genotype_at_its_boundaries():
    g = genotype(12, 12, 0)
    assert (g["gt"], g["qual"], g["L"], g["row"]) == (R.RA, 8520, [19320, 7800, 19320], True) and g["pl"] == [115, 0, 115] and g["gq"] == 85      # Q = (19320, 10800, 22621)
    g = genotype(19, 5, 0)
    assert g["gt"] == R.RR and not g["row"]
    g = genotype(17, 7, 0)
    assert (g["gt"], g["qual"], g["row"]) == (R.RA, 830, False)
    assert genotype(17, 7, 0, min_qual=830)["row"] and not genotype(17, 7, 0, min_qual=831)["row"]
    g = genotype(0, 4, 0)
    assert (g["gt"], g["qual"], g["row"]) == (R.AA, 2851, True)
    g = genotype(0, 3, 0)
    assert (g["gt"], g["qual"], g["row"]) == (R.AA, 1313, False)           # below the default min_qual, and below the default min_depth
    assert genotype(0, 3, 0, min_qual=1313, min_depth=3)["row"] and not genotype(0, 3, 0, min_qual=1313)["row"]
    assert genotype(1, 1, 0)["gt"] == R.RR
    # ties between Q values go RR, then RA, then AA: with m 1, h 2, x 3 two alt reads give L = (6, 4, 2)
    tie = dict(cost_match=1, cost_het=2, cost_mismatch=3)
    assert genotype(0, 2, 0, **tie)["L"] == [6, 4, 2]
    assert genotype(0, 2, 0, prior_het=2, prior_hom=4, **tie)["gt"] == R.RR                       # Q = (6, 6, 6)
    assert genotype(0, 2, 0, prior_het=2, prior_hom=5, **tie)["gt"] == R.RR                       # Q = (6, 6, 7): RR in front of RA
    assert genotype(0, 2, 0, prior_het=3, prior_hom=4, **tie)["gt"] == R.RR                       # Q = (6, 7, 6): RR in front of AA
    assert genotype(0, 2, 0, prior_het=1, prior_hom=3, **tie)["gt"] == R.RA                       # Q = (6, 5, 5): RA in front of AA
    assert genotype(0, 2, 0, prior_het=2, prior_hom=3, **tie)["gt"] == R.AA                       # Q = (6, 6, 5)
    assert genotype(0, 1, 1, prior_het=1, prior_hom=2, **tie)["gt"] == R.RR                       # L = (6, 5, 4), Q = (6, 6, 6)
    # qual and pl saturate at u32 with counts near 2^32, and are exact just below
    big = U32 - 1
    g = genotype(0, big, 0)                                              # L = big * (1574, 325, 36)
    assert g["gt"] == R.AA and g["qual"] == U32 and g["pl"] == [U32, U32, 0] and g["gq"] == 99 and g["row"]
    g = genotype(big, big, big)                                          # L = big * (3184, 2224, 3184)
    assert g["gt"] == R.RA and g["qual"] == U32 and g["pl"] == [U32, 0, U32] and g["gq"] == 99
    g = genotype(big, 0, 0)
    assert g["gt"] == R.RR and g["qual"] == 0 and g["pl"] == [0, U32, U32] and not g["row"]
    assert genotype(0, 2_792_000, 0)["qual"] == 2_792_000 * 1538 - 3301 == 4_294_092_699            # one step below 2^32 - 1
    assert genotype(0, 2_793_000, 0)["qual"] == U32
    with pytest.raises(F.FloxerError):
        F.variants_genotype(1 << 34, 0, 0)


def one_column(R_rank, planes, o, ins=(), dels=()):
    """a single position of rank R_rank between two A, as records of one column each: planes = dict(eq, A, C, G, T, DEL); ins: insertion
    strings behind the column, one record of [= 1, I n] each; dels: deletion lengths behind it, one record of [= 1, D n] each (both add to
    eq). Returns (text, lengths, records, words, reads)."""
    text = np.array([1, R_rank, 1] + [1] * (max(dels) if dels else 0), dtype=np.uint8)
    own = R_rank if 1 <= R_rank <= 4 else 1
    rows, reads = [], []
    for name, n in planes.items():
        for _ in range(n):
            if name == "DEL":
                rows.append((0, 0, 0, 0, [R.word("=", 1), R.word("D", 1), R.word("=", 1)]))
                reads.append([1, 1])
            elif name == "eq":
                rows.append((0, 0, 1, 0, [R.word("=", 1)]))
                reads.append([own])
            else:
                rows.append((0, 0, 1, 0, [R.word("X", 1)]))
                reads.append(["NACGT".index(name)])
    for s in ins:
        rows.append((0, 0, 1, 0, [R.word("=", 1), R.word("I", len(s))]))
        reads.append([own] + list(s))
    for n in dels:
        rows.append((0, 0, 1, 0, [R.word("=", 1), R.word("D", n)]))
        reads.append([own])
    rec, words = R.records_of(rows)
    return text, [len(text)], rec, words, [np.array(x, dtype=np.uint8) for x in reads]


LOW = R.options(min_depth=1, min_qual=1)
# (name, R, planes, options, insertions, deletions) -> the column's rows as (kind, alt_rank, length, ref_count, alt_count, cov, gt)
COLUMNS = [
    ("a het SNV", 2, dict(eq=12, A=12), R.options(), (), (), [(R.SNV, 1, 1, 12, 12, 24, R.RA)]),
    ("a hom SNV", 2, dict(T=4), R.options(), (), (), [(R.SNV, 4, 1, 0, 4, 4, R.AA)]),
    ("cov one below min_depth", 2, dict(T=3), R.options(min_qual=1), (), (), []),
    ("qual one below min_qual", 2, dict(eq=17, G=7), R.options(min_qual=831), (), (), []),
    ("qual at min_qual", 2, dict(eq=17, G=7), R.options(min_qual=830), (), (), [(R.SNV, 3, 1, 17, 7, 24, R.RA)]),
    ("the genotype is RR", 2, dict(eq=19, G=5), LOW, (), (), []),
    ("alt ties go to the smallest rank", 3, dict(T=5, A=5, eq=2), LOW, (), (), [(R.SNV, 1, 1, 2, 5, 12, R.RA)]),
    ("alt ties skip R", 1, dict(eq=5, G=5, C=5), LOW, (), (), [(R.SNV, 2, 1, 5, 5, 15, R.RA)]),
    ("no alt count: no candidate", 2, dict(eq=9), LOW, (), (), []),
    ("R = 0: no SNV candidate", 0, dict(G=9), LOW, (), (), []),
    ("R = 5: no SNV candidate", 5, dict(G=9), LOW, (), (), []),
    ("oth from a third letter", 2, dict(eq=6, A=6, T=3), LOW, (), (), [(R.SNV, 1, 1, 6, 6, 15, R.RA)]),
    ("oth from DEL columns", 2, dict(eq=6, A=6, DEL=3), LOW, (), (), [(R.SNV, 1, 1, 6, 6, 15, R.RA)]),
    ("oth weighs on RR and AA alike", 2, dict(A=4, DEL=40), R.options(), (), (), [(R.SNV, 1, 1, 0, 4, 44, R.AA)]),      # qual 2851 as (0, 4, 0)
    ("a het insertion", 3, dict(eq=5), LOW, ([4, 1],) * 5, (), [(R.INS, 0, 2, 5, 5, 10, R.RA)]),
    ("a hom deletion", 3, dict(), LOW, (), (2,) * 6, [(R.DEL, 0, 2, 0, 6, 6, R.AA)]),
    ("an insertion on R = 5", 5, dict(), LOW, ([2],) * 6, (), [(R.INS, 0, 1, 0, 6, 6, R.AA)]),
    ("DEL and INS tie: the deletion is the smaller key", 3, dict(), LOW, ([4, 1],) * 4, (3,) * 4, [(R.DEL, 0, 3, 0, 4, 8, R.AA)]),      # L = (12592, 7596, 6440)
    ("two insertions tie: the smaller letters", 3, dict(), LOW, ([4, 1], [2, 3]) * 4, (), [(R.INS, 0, 2, 0, 4, 8, R.AA)]),
    ("a shorter insertion is the smaller key", 3, dict(), LOW, ([4, 1], [4]) * 4, (), [(R.INS, 0, 1, 0, 4, 8, R.AA)]),
    ("three alleles: events is their sum", 3, dict(eq=2), LOW, ([4, 1],) * 7 + ([1],) * 2, (1,) * 3, [(R.INS, 0, 2, 2, 7, 14, R.RA)]),      # oth 5: L = (18960, 10795, 11270)
    ("a deletion longer than max_del is no allele", 3, dict(), R.options(min_depth=1, min_qual=1, max_del=2), (), (3,) * 6, []),
    ("an SNV row in front of an indel row", 2, dict(T=6), LOW, ([1, 1, 1],) * 6, (), [(R.SNV, 4, 1, 6, 6, 12, R.RA), (R.INS, 0, 3, 6, 6, 12, R.RA)]),
]


@pytest.mark.parametrize("case", COLUMNS, ids=[c[0] for c in COLUMNS])
def test_the_call_column_by_column(case):
    _, rank, planes, o, ins, dels, rows = case
    text, lengths, rec, words, reads = one_column(rank, planes, o, ins, dels)
    got = same(F.variants_host(text, lengths, rec, words, reads, R.c_options(o)), R.variants(text, lengths, rec, words, reads, o))
    mine = got[0][got[0]["pos"] == 1]
    assert [(int(c["kind"]), int(c["alt_rank"]), int(c["length"]), int(c["ref_count"]), int(c["alt_count"]), int(c["cov"]), int(c["gt"])) for c in mine] == rows, mine
    assert all(int(c["ref_rank"]) == rank for c in mine)


# ------------------------------------------------------------------------------------------------ a diploid sample without the aligner
HOM_SNVS, HET_SNVS = (1100, 1700, 2900), (1300, 2200, 2600)
DEL_ANCHOR, DEL_LEN, INS_ANCHOR, INS_LETTERS = 1500, 3, 2400, (2, 4)
# The reference alone was run on seeds 0..7 at both error rates under both sets of costs: every planted variant with its genotype and no
# other row, except that seeds 0 and 1 each show one false 0/1 SNV where fewer than 40 reads cover (positions 3520 and 266) when costs
# for an error of 0.02 judge reads with 0.08, a model four times too confident. Seeds 2..7 show none; the cap stays 0.
SAMPLE_SEED = 2


def costs_for(e, theta=0.001):
    cp = lambda p: int(math.floor(-1000 * math.log10(p) + 0.5))          # noqa: E731
    return dict(cost_match=cp(1 - e), cost_mismatch=cp(e / 3), cost_het=cp((1 - e) / 2 + e / 6), prior_het=cp(theta), prior_hom=cp(theta / 2))


def diploid_sample(rate, seed=SAMPLE_SEED):
    """one reference of 4000 letters; two haplotypes with three homozygous SNVs, three heterozygous ones on the first, a heterozygous
    deletion of three bases on the first and a homozygous insertion of two; reads over 1000 reference positions from each haplotype start
    every 50 positions (20 per haplotype over the interior) with substitution errors at `rate`; the CIGARs are written here from the
    truth. Returns (text, records, words, reads, the planted rows as {(pos, kind): gt})."""
    rng = np.random.default_rng(seed)
    text = rng.integers(1, 5, size=4000).astype(np.uint8)
    alt = {p: 1 + (int(text[p]) + int(rng.integers(0, 3))) % 4 for p in HOM_SNVS + HET_SNVS}     # another letter than the text's
    assert all(alt[p] != int(text[p]) for p in alt)
    rows, reads = [], []
    for hap in (0, 1):
        for start in range(0, 3001, 50):
            ops, letters = [], []
            for p in range(start, start + 1000):
                if hap == 0 and DEL_ANCHOR < p <= DEL_ANCHOR + DEL_LEN:
                    ops.append("D")
                    continue
                true = alt[p] if p in HOM_SNVS or (hap == 0 and p in HET_SNVS) else int(text[p])
                seen = 1 + (true + int(rng.integers(0, 3))) % 4 if rng.random() < rate else true
                ops.append("=" if seen == int(text[p]) else "X")
                letters.append(seen)
                if p == INS_ANCHOR:
                    for x in INS_LETTERS:
                        ops.append("I")
                        letters.append(1 + (x + int(rng.integers(0, 3))) % 4 if rng.random() < rate else x)
            ws, k = [], 0
            while k < len(ops):
                e = k
                while e < len(ops) and ops[e] == ops[k]:
                    e += 1
                ws.append(R.word(ops[k], e - k))
                k = e
            flag = 16 if (start // 50 + hap) % 2 else 0
            rows.append((flag, 0, start, 0, ws))
            seq = np.array(letters, dtype=np.uint8)
            reads.append(P.COMPLEMENT[seq[::-1]] if flag else seq)         # the read as given: the oriented sequence is SEQ
    rec, words = R.records_of(rows)
    rec["read"] = np.arange(len(rec))
    planted = {(p, R.SNV): R.AA for p in HOM_SNVS}
    planted.update({(p, R.SNV): R.RA for p in HET_SNVS})
    planted[(DEL_ANCHOR, R.DEL)] = R.RA
    planted[(INS_ANCHOR, R.INS)] = R.AA
    return text, rec, words, reads, planted, alt


@pytest.mark.parametrize("rate", [0.02, 0.08])
@pytest.mark.parametrize("costs", [0.08, 0.02], ids=["costs_for_0.08", "costs_for_0.02"])
def test_a_diploid_sample_made_without_the_aligner(rate, costs):
    """every planted variant is a row with its genotype and no other row exists, at min_depth 4 and min_qual 2000 (the cap on other rows
    is 0)"""
    text, rec, words, reads, planted, alt = diploid_sample(rate)
    interior = P.counts([4000], rec, words, reads, R.options())[:2, 1000:3000].sum(axis=0)
    assert (interior == 40).all()                                         # 20 reads per haplotype
    o = R.options(min_depth=4, min_qual=2000, **(costs_for(costs) if costs != 0.08 else {}))
    if costs == 0.08:
        assert costs_for(0.08) == dict(cost_match=36, cost_mismatch=1574, cost_het=325, prior_het=3000, prior_hom=3301)
    rows, al = same(F.variants_host(text, [4000], rec, words, reads, R.c_options(o)), R.variants(text, [4000], rec, words, reads, o))
    got = {(int(r["pos"]), int(r["kind"])): int(r["gt"]) for r in rows}
    assert got == planted, (sorted(set(got) ^ set(planted)), [(k, got[k], planted[k]) for k in got if k in planted and got[k] != planted[k]])
    by = {(int(r["pos"]), int(r["kind"])): r for r in rows}
    assert all(int(by[(p, R.SNV)]["alt_rank"]) == alt[p] for p in HOM_SNVS + HET_SNVS)
    assert int(by[(DEL_ANCHOR, R.DEL)]["length"]) == DEL_LEN and R.letters_of(by[(INS_ANCHOR, R.INS)]["letters"], 2) == "CT"
    assert {0, 16} == {int(f) for f in rec["flag"]}


# ------------------------------------------------------------------------------------------------ the ABI
def test_symbols_sizes_and_python_names():
    L = capi.lib()
    names = [n for n in capi.EXPORTED if n.startswith("flx_variants_")]
    header = open(os.path.join(ROOT, "include", "floxer_amd.h")).read()
    assert set(names) == {n for n in re.findall(r"\b(flx_[a-z0-9_]+)\s*\(", header) if n.startswith("flx_variants_")}
    for name in names:
        getattr(L, name)
    assert {"flx_variants_create", "flx_variants_create_for_text", "flx_variants_free", "flx_variants_add_records", "flx_variants_add_run", "flx_variants_add_run_resident",
            "flx_variants_finish", "flx_variants_num_rows", "flx_variants_copy_rows", "flx_variants_num_alleles", "flx_variants_copy_alleles", "flx_variants_geometry",
            "flx_variants_host"} <= set(names) and len(names) == 14
    assert C.sizeof(capi.VariantsOptions) == 48 and C.sizeof(capi.Variant) == 72 and C.sizeof(capi.VariantAllele) == 32
    assert F.VARIANT_DTYPE.itemsize == 72 and F.VARIANT_ALLELE_DTYPE.itemsize == 32 and F.VARIANT_KINDS == ("SNV", "DEL", "INS")
    for dtype, struct in ((F.VARIANT_DTYPE, capi.Variant), (F.VARIANT_ALLELE_DTYPE, capi.VariantAllele)):
        assert [dtype.fields[n][1] for n in dtype.names] == [getattr(struct, f[0]).offset for f in struct._fields_]
    o = F.variants_options(count_secondary=True, min_mapq=7, min_depth=5, min_qual=1500, max_del=30, cost_match=1, cost_mismatch=3, cost_het=2, prior_het=4, prior_hom=5)
    assert (o.count_secondary, o.min_mapq, o.min_depth, o.min_qual, o.max_del, o.cost_match, o.cost_mismatch, o.cost_het, o.prior_het, o.prior_hom, list(o.reserved)) == \
        (1, 7, 5, 1500, 30, 1, 3, 2, 4, 5, [0, 0])
    cap, waves, longest, max_del = F.variants_geometry()
    assert cap >= 1 and waves == 4 and longest == 32 and max_del == 50
    for name in ("variants", "variants_options", "variants_host", "variants_geometry", "VARIANT_KINDS"):
        assert hasattr(F, name)
    for method in ("add_records", "add", "finish", "rows", "alleles", "close"):
        assert callable(getattr(F.variants, method))
    with pytest.raises(F.FloxerError):                                   # no device: the host form is variants_host
        F.variants(text=[np.ones(5, dtype=np.uint8)], device=-1)


def test_refusals_of_the_host_rule():
    rng = np.random.default_rng(9)
    text = R.random_text(rng, 60)
    rec, words = R.records_of([(0, 0, 3, 0, [R.word("=", 20), R.word("I", 2), R.word("X", 3), R.word("D", 2), R.word("=", 1)])] * 6)
    rec["read"] = 0
    reads = [np.array([1] * 20 + [2, 3] + [4, 4, 4] + [1], dtype=np.uint8)]
    bad = capi.VariantsOptions()
    bad.reserved[1] = 1
    refused = (bad, F.variants_options(cost_het=1574), F.variants_options(cost_het=1575), F.variants_options(cost_match=325), F.variants_options(cost_match=400),
               F.variants_options(cost_mismatch=325), F.variants_options(cost_match=5, cost_het=5, cost_mismatch=9), F.variants_options(max_del=1 << 28),
               F.variants_options(prior_het=(1 << 20) + 1))
    for o in refused:
        with pytest.raises(F.FloxerError):
            F.variants_host(text, [60], rec, words, reads, o)
        with pytest.raises(F.FloxerError):
            F.variants_genotype(1, 1, 1, o)
    for o in (F.variants_options(cost_match=324), F.variants_options(cost_het=1573), F.variants_options(max_del=(1 << 28) - 1), F.variants_options(prior_hom=1 << 20)):
        F.variants_host(text, [60], rec, words, reads, o)
    with pytest.raises(F.FloxerError, match="rank above 5"):
        F.variants_host(np.full(60, 6, dtype=np.uint8), [60], rec, words, reads)
    # everything pileup_plan refuses: past the end, a sequence that is not there, an M word, no reference-consuming column, no word
    for rows in ([(0, 0, 50, 0, [R.word("=", 11)])], [(0, 1, 0, 0, [R.word("=", 1)])], [(0, 0, 0, 0, [R.word("M", 5)])], [(0, 0, 0, 0, [R.word("S", 5), R.word("I", 1)])],
                 [(0, 0, 0, 0, [])]):
        rec2, words2, reads2 = R.records_with_reads(rng, [(0, 0, 3, 0, [R.word("=", 20)])] * 2 + rows)
        with pytest.raises(F.FloxerError):
            F.variants_host(text, [60], rec2, words2, reads2)
    rec2, words2, reads2 = R.records_with_reads(rng, [(0, 0, 3, 0, [R.word("=", 20)])] * 2)
    with pytest.raises(F.FloxerError):                                   # the query-consuming lengths and the read disagree
        F.variants_host(text, [60], rec2, words2, [reads2[0], reads2[1][:-1]])
    rec2["read"][1] = 2
    with pytest.raises(F.FloxerError, match="read_index"):
        F.variants_host(text, [60], rec2, words2, reads2)
    rows, al = F.variants_host(text, [60], rec, words, reads, F.variants_options(min_depth=1))
    assert [(int(a["pos"]), int(a["kind"]), int(a["length"]), int(a["count"])) for a in al] == [(22, R.INS, 2, 6), (25, R.DEL, 2, 6)]
    assert {(22, R.INS), (25, R.DEL)} <= {(int(r["pos"]), int(r["kind"])) for r in rows}


# ------------------------------------------------------------------------------------------------ the tool's parser
def tool(*args):
    env = dict(os.environ, FLX_VARIANTS_PARSE_ONLY="1")                  # the parser alone: no device is touched, no file is opened
    return subprocess.run([TOOL] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def parsed(*args):
    r = tool(*args)
    assert r.returncode == 0 and r.stdout == b"" and b"CLI PARSER ERROR" not in r.stderr, (args, r.stderr)
    return dict(l.split("=", 1) for l in r.stderr.decode().splitlines())


def test_tool_parser_and_cost_derivation(tmp_path):
    ref, reads = os.path.join(GOLDEN, "reference.fasta"), os.path.join(GOLDEN, "queries.fastq")
    vcf = str(tmp_path / "calls.vcf")
    base = ["--reference", ref, "--queries", reads, "--output", vcf]
    h = subprocess.run([TOOL, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0 and h.stdout == b""
    lines = h.stderr.decode().splitlines()
    options = ("reference", "queries", "output", "query-errors", "error-probability", "device", "min-depth", "min-qual", "max-deletion", "heterozygosity", "read-error",
               "secondary", "min-mapq", "realign-affine", "batch-reads", "sample")
    for name in options:
        assert len([l for l in lines if re.search(rf"^\s+(-\w, )?--{name}(\s|$)", l)]) == 1, name
    assert len(lines) == 1 + len(options) and lines[0].startswith("floxer_variants")
    costs = lambda d: tuple(int(d[k]) for k in ("cost-match", "cost-mismatch", "cost-het"))       # noqa: E731
    priors = lambda d: (int(d["prior-het"]), int(d["prior-hom"]))                                # noqa: E731
    d = parsed(*base, "--error-probability", "0.08")
    assert costs(d) == (36, 1574, 325) and priors(d) == (3000, 3301)      # --read-error defaults to --error-probability, the heterozygosity to 0.001
    assert (d["min-depth"], d["min-qual"], d["max-deletion"], d["secondary"], d["min-mapq"], d["batch-reads"], d["output"], d["sample"]) == ("0", "0", "0", "0", "0", "16384", vcf, "SAMPLE")
    assert costs(parsed(*base, "-p", "0.08", "--read-error", "0.01")) == (4, 2477, 304)
    assert costs(parsed(*base, "-p", "0.01")) == (4, 2477, 304)
    assert costs(parsed(*base, "-p", "0.05", "--read-error", "0.15")) == (71, 1301, 347)
    assert costs(parsed(*base, "-e", "3")) == (36, 1574, 325)             # neither given: 0.08
    assert costs(parsed(*base, "-p", "0.05", "--read-error", "0.00001")) == (1, 5477, 301)  # -1000 log10(0.99999) rounds to 0, the library's "default": the tool says 1
    assert priors(parsed(*base, "-p", "0.08", "--heterozygosity", "0.001")) == (3000, 3301)
    assert priors(parsed(*base, "-p", "0.08", "--heterozygosity=0.01")) == (2000, 2301)
    d = parsed(*base, "-p", "0.05", "--min-depth", "7", "--min-qual", "20", "--max-deletion", "30", "--secondary", "--min-mapq", "5", "--realign-affine", "--batch-reads", "9",
               "--sample", "NA12878", "--device", "1")
    assert (d["min-depth"], d["min-qual"], d["max-deletion"], d["secondary"], d["min-mapq"], d["realign-affine"], d["batch-reads"], d["sample"], d["device"]) == \
        ("7", "2000", "30", "1", "5", "1", "9", "NA12878", "1")
    assert parsed(*base, "-p", "0.05", "--min-qual", "8.3")["min-qual"] == "830"
    good = (["-e", "2"], ["-p", "0.00001", "--min-mapq", "254", "--batch-reads", "16777216"], ["-p", "0.99999", "--read-error", "0.5"], ["-e", "4096"],
            ["-p", "0.05", "--max-deletion", "268435455", "--min-depth", "1000000", "--device", "1023", "--heterozygosity", "0.5", "--min-qual", "0.01"])
    for extra in good:
        parsed(*base, *extra)
    bad = ([], ["-e", "1"], ["-e", "4097"], ["-p", "0.000001"], ["-p", "1"], ["-p", "x"], ["-e", "-1"], ["-p", "0.05", "--device", "1024"], ["-p", "0.05", "--min-depth", "0"],
           ["-p", "0.05", "--min-depth", "1000001"], ["-p", "0.05", "--min-qual", "0"], ["-p", "0.05", "--min-qual", "10001"], ["-p", "0.05", "--max-deletion", "0"],
           ["-p", "0.05", "--max-deletion", "268435456"], ["-p", "0.05", "--heterozygosity", "0"], ["-p", "0.05", "--heterozygosity", "0.51"], ["-p", "0.05", "--read-error", "0"],
           ["-p", "0.05", "--read-error", "0.51"], ["-p", "0.05", "--min-mapq", "0"], ["-p", "0.05", "--min-mapq", "255"], ["-p", "0.05", "--batch-reads", "0"],
           ["-p", "0.05", "--batch-reads", "16777217"], ["-p", "0.05", "--sample", "two words"], ["-p", "0.05", "--sample", ""], ["-p", "0.05", "--min-depth"], ["-p", "0.05", "--sam"],
           ["-p", "0.05", "--changes", str(tmp_path / "changes.tsv")], ["-p", "0.05", "stray"])
    for extra in bad:
        r = tool(*base, *extra)
        assert r.returncode == 255 and r.stderr.startswith(b"[CLI PARSER ERROR]\n") and r.stdout == b"", (extra, r.stderr)
    for args, what in ((["--queries", reads, "--output", vcf, "-p", "0.05"], b"-r/--reference is required"), (["--reference", ref, "--output", vcf, "-p", "0.05"], b"-q/--queries is required"),
                       (["--reference", ref, "--queries", reads, "-p", "0.05"], b"-o/--output is required"),
                       (["--reference", ref, "--queries", reads, "--output", str(tmp_path / "calls.bcf"), "-p", "0.05"], b"[vcf]"),
                       (["--reference", ref, "--queries", reads, "--output", str(tmp_path / "calls.vcf.gz"), "-p", "0.05"], b"[vcf]"),
                       (["--reference", reads, "--queries", reads, "--output", vcf, "-p", "0.05"], b"-r/--reference"),
                       (["--reference", ref, "--queries", ref, "--output", vcf, "-p", "0.05"], b"-q/--queries"),
                       (["--reference", str(tmp_path / "none.fa"), "--queries", reads, "--output", vcf, "-p", "0.05"], b"does not exist"),
                       (base, b"Either a fixed number of errors"), (base + ["-e", "1"], b"PEX tree leaves")):
        r = tool(*args)
        assert r.returncode == 255 and r.stderr.startswith(b"[CLI PARSER ERROR]\n") and what in r.stderr, (args, r.stderr)
    assert os.listdir(tmp_path) == []


def test_rule_header_against_a_column_walk_under_sanitizers(tmp_path):
    """tests/variants_check.cpp: flx_variants.hpp on random records, built with ASan + UBSan; nothing is preloaded"""
    exe = str(tmp_path / "variants_check")
    src = os.path.join(ROOT, "tests", "variants_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
