"""The variant-calling rule (flx_variants, include/floxer_amd.h) in plain numpy and Python, for the tests: the counts are
pileup_ref.counts', the alleles come from a walk over the I and D words of the counted records, the SNV candidates and their genotypes
are vectorised over the positions, the indel candidates go anchor by anchor; next to the call a naive position-by-position loop with
the scalar genotype that the reference itself is checked against.

text: the uint8 ranks of the unpadded concatenation of the sequences; records, words, lengths, reads: as in pileup_ref. The results are
(rows, alleles): structured arrays of floxer_amd.VARIANT_DTYPE and VARIANT_ALLELE_DTYPE."""
import numpy as np

import floxer_amd as F
import pileup_ref as P
from pileup_ref import REC, records_of, records_with_reads, span, starts_of, word  # noqa: F401 (shared with the tests)

DEFAULTS = dict(min_depth=4, min_qual=2000, max_del=50, cost_match=36, cost_mismatch=1574, cost_het=325, prior_het=3000, prior_hom=3301)
SNV, DEL, INS = 0, 1, 2
KEY_DEL, KEY_INS = 0, 1                                                  # the kinds inside a key: deletions sort in front of insertions
RR, RA, AA = 0, 1, 2
MAX_INS = 32
U32 = (1 << 32) - 1
VOID = ((1 << 64) - 1, (1 << 64) - 1)


def options(count_secondary=False, min_mapq=0, min_depth=0, min_qual=0, max_del=0, cost_match=0, cost_mismatch=0, cost_het=0, prior_het=0, prior_hom=0):
    return dict(count_secondary=count_secondary, min_mapq=min_mapq, min_depth=min_depth, min_qual=min_qual, max_del=max_del, cost_match=cost_match,
                cost_mismatch=cost_mismatch, cost_het=cost_het, prior_het=prior_het, prior_hom=prior_hom)


def c_options(o):
    return F.variants_options(**o)


def model(o):
    """the eight numbers of the rule with the defaults taken for 0"""
    return {k: int(o[k]) or DEFAULTS[k] for k in DEFAULTS}


def pack(letters):
    """ranks 1..4 -> the key's lo: letter k at bits 63 - 2k and 62 - 2k"""
    lo = 0
    for k, r in enumerate(letters):
        lo |= (int(r) - 1) << (62 - 2 * k)
    return lo


def letters_of(lo, length):
    return "".join("ACGT"[(int(lo) >> (62 - 2 * k)) & 3] for k in range(int(length)))


def key_of(anchor, kind, length, letters, max_del):
    """(hi, lo) of an event behind `anchor` (None: no column precedes it), or the void key"""
    if anchor is None or length < 1:
        return VOID
    if kind == KEY_DEL:
        return VOID if length > max_del else (int(anchor) << 32 | KEY_DEL << 28 | length, 0)
    letters = [int(x) for x in letters]
    if length > MAX_INS or any(not 1 <= x <= 4 for x in letters):
        return VOID
    return int(anchor) << 32 | KEY_INS << 28 | length, pack(letters)


def events(lengths, records, words, reads, o):
    """the allele key (anchor, kind, length, lo) of every I and D word of every counted record that yields one, in record and word order"""
    starts = starts_of(lengths)
    max_del = model(o)["max_del"]
    out = []
    for rec in records:
        if not P.record_counts(rec, o):
            continue
        ws = [(int(w) & 15, int(w) >> 4) for w in words[int(rec["coff"]): int(rec["coff"]) + int(rec["clen"])]]
        if not any(op in (1, 2) for op, _ in ws):
            continue
        seq = P.oriented(reads[int(rec["read"])], rec["flag"])
        origin = int(starts[int(rec["ref"])]) + int(rec["pos"])
        p, row = origin, 0
        for op, ln in ws:
            if op in (1, 2):
                anchor = p - 1 if p > origin else None
                hi, lo = key_of(anchor, KEY_INS if op == 1 else KEY_DEL, ln, seq[row: row + ln] if op == 1 and ln <= MAX_INS else [], max_del)
                if (hi, lo) != VOID:
                    out.append((hi >> 32, hi >> 28 & 15, hi & ((1 << 28) - 1), lo))
            if op in (7, 8, 2):
                p += ln
            if op in (7, 8, 1, 4):
                row += ln
    return out


def alleles_of(lengths, evs, times=1):
    """the events grouped: a structured array of floxer_amd.VARIANT_ALLELE_DTYPE in key order, every count multiplied by `times`"""
    starts = starts_of(lengths)
    count = {}
    for e in evs:
        count[e] = count.get(e, 0) + times
    keys = sorted(count)
    out = np.zeros(len(keys), dtype=F.VARIANT_ALLELE_DTYPE)
    for i, (a, kind, ln, lo) in enumerate(keys):
        ref = int(np.searchsorted(starts, a, side="right")) - 1
        out[i] = (ref, a - int(starts[ref]), INS if kind == KEY_INS else DEL, ln, count[(a, kind, ln, lo)], 0, lo)
    return out


def winners(lengths, al):
    """{anchor in the concatenation: (index of its winning allele, events)}: the largest count, the first in key order among equals"""
    starts = starts_of(lengths)
    win = {}
    for i, a in enumerate(al):
        p = int(starts[int(a["ref"])]) + int(a["pos"])
        if p not in win:
            win[p] = (i, int(a["count"]))
        else:
            w, ev = win[p]
            win[p] = (i if int(a["count"]) > int(al[w]["count"]) else w, ev + int(a["count"]))
    return win


def genotype(ref_n, alt_n, oth, m):
    """the scalar rule in Python integers -> dict(gt, gq, qual, pl, L)"""
    ref_n, alt_n, oth = int(ref_n), int(alt_n), int(oth)
    L = [ref_n * m["cost_match"] + (alt_n + oth) * m["cost_mismatch"], (ref_n + alt_n) * m["cost_het"] + oth * m["cost_mismatch"],
         alt_n * m["cost_match"] + (ref_n + oth) * m["cost_mismatch"]]
    Q = [L[0], L[1] + m["prior_het"], L[2] + m["prior_hom"]]
    gt = min(range(3), key=lambda g: (Q[g], g))
    ordered = sorted(Q)
    return dict(gt=gt, gq=min((ordered[1] - ordered[0]) // 100, 99), qual=min(max(Q[0] - min(Q[1], Q[2]), 0), U32), pl=[min((x - min(L)) // 100, U32) for x in L], L=L)


def makes_row(g, cov, m):
    return g["gt"] != RR and cov >= m["min_depth"] and g["qual"] >= m["min_qual"]


def row_of(ref, pos, kind, ref_rank, alt_rank, length, ref_n, alt_n, cov, g, letters):
    return (ref, pos, kind, ref_rank, alt_rank, length, min(ref_n, U32), min(alt_n, U32), min(cov, U32), g["gt"], g["gq"], g["qual"], g["pl"], 0, letters)


def call(text, lengths, cnt, al, o):
    """the SNV candidates of all positions at once (int64: the tests' counts times a cost stay far below 2^63), the indel candidates anchor
    by anchor -> rows"""
    starts = starts_of(lengths)
    total = int(starts[-1])
    m = model(o)
    c = np.asarray(cnt, dtype=np.int64)
    R = np.asarray(text, dtype=np.int64)
    at = np.arange(total)
    cov = c[P.DEPTH] + c[P.DEL]
    n = np.zeros((5, total), dtype=np.int64)
    n[1:5] = c[P.A:P.T + 1]
    letter = (R >= 1) & (R <= 4)
    n[R[letter], at[letter]] += (c[P.DEPTH] - c[P.A:P.T + 1].sum(axis=0))[letter]
    ref_n = n[np.where(letter, R, 0), at]
    others = n.copy()
    others[0] = -1
    others[np.where(letter, R, 0), at] = -1
    alt = np.argmax(others, axis=0)                                       # (the first of the largest: the smallest rank)
    alt_n = others[alt, at]
    cand = letter & (alt_n > 0)
    oth = cov - ref_n - alt_n
    mm, xx, hh = m["cost_match"], m["cost_mismatch"], m["cost_het"]
    L = np.stack([ref_n * mm + (alt_n + oth) * xx, (ref_n + alt_n) * hh + oth * xx, alt_n * mm + (ref_n + oth) * xx])
    Q = L + np.array([[0], [m["prior_het"]], [m["prior_hom"]]], dtype=np.int64)
    gt = np.argmin(Q, axis=0)                                             # (the first of the smallest: RR, RA, AA)
    qs = np.sort(Q, axis=0)
    gq = np.minimum((qs[1] - qs[0]) // 100, 99)
    qual = np.clip(Q[0] - np.minimum(Q[1], Q[2]), 0, U32)
    pl = np.minimum((L - L.min(axis=0)) // 100, U32)
    stands = cand & (gt != RR) & (cov >= m["min_depth"]) & (qual >= m["min_qual"])
    sp = at[stands]
    win = winners(lengths, al)
    indel_rows = []
    for p in sorted(win):
        i, ev = win[p]
        a = al[i]
        cv, k = int(cov[p]), int(a["count"])
        g = genotype(max(cv - ev, 0), k, ev - k, m)
        if makes_row(g, cv, m):
            r = int(np.searchsorted(starts, p, side="right")) - 1
            indel_rows.append((p, row_of(r, p - int(starts[r]), int(a["kind"]), int(R[p]), 0, int(a["length"]), max(cv - ev, 0), k, cv, g,
                                         int(a["letters"]) if int(a["kind"]) == INS else 0)))
    rows = np.zeros(len(sp) + len(indel_rows), dtype=F.VARIANT_DTYPE)
    order = np.zeros(len(rows), dtype=np.int64)
    k = len(sp)
    ref = np.searchsorted(starts, sp, side="right") - 1
    rows["ref"][:k], rows["pos"][:k], rows["kind"][:k] = ref, sp - starts[ref], SNV
    rows["ref_rank"][:k], rows["alt_rank"][:k], rows["length"][:k] = R[sp], alt[sp], 1
    rows["ref_count"][:k], rows["alt_count"][:k], rows["cov"][:k] = ref_n[sp], alt_n[sp], cov[sp]
    rows["gt"][:k], rows["gq"][:k], rows["qual"][:k], rows["pl"][:k] = gt[sp], gq[sp], qual[sp], pl[:, sp].T
    order[:k] = sp * 2
    for j, (p, row) in enumerate(indel_rows):
        rows[k + j] = row
        order[k + j] = p * 2 + 1
    return rows[np.argsort(order, kind="stable")]


def call_naive(text, lengths, cnt, al, o):
    """one position at a time, as the rule is written"""
    starts = starts_of(lengths)
    m = model(o)
    win = winners(lengths, al)
    rows = []
    for r in range(len(lengths)):
        for p in range(int(starts[r]), int(starts[r + 1])):
            v = [int(cnt[k][p]) for k in range(7)]
            R, cov = int(text[p]), v[P.DEPTH] + v[P.DEL]
            if 1 <= R <= 4:
                n = {1: v[P.A], 2: v[P.C], 3: v[P.G], 4: v[P.T]}
                n[R] += v[P.DEPTH] - v[P.A] - v[P.C] - v[P.G] - v[P.T]
                top = max(n[k] for k in n if k != R)
                alt = min(k for k in n if k != R and n[k] == top)
                if top > 0:
                    g = genotype(n[R], n[alt], cov - n[R] - n[alt], m)
                    if makes_row(g, cov, m):
                        rows.append(row_of(r, p - int(starts[r]), SNV, R, alt, 1, n[R], n[alt], cov, g, 0))
            if p in win:
                i, ev = win[p]
                a = al[i]
                k = int(a["count"])
                g = genotype(max(cov - ev, 0), k, ev - k, m)
                if makes_row(g, cov, m):
                    rows.append(row_of(r, p - int(starts[r]), int(a["kind"]), R, 0, int(a["length"]), max(cov - ev, 0), k, cov, g, int(a["letters"]) if int(a["kind"]) == INS else 0))
    return np.array(rows, dtype=F.VARIANT_DTYPE) if rows else np.zeros(0, dtype=F.VARIANT_DTYPE)


def variants(text, lengths, records, words, reads, o, times=1):
    """the whole rule -> (rows, alleles); times: every record counts that often"""
    cnt = P.counts(lengths, records, words, reads, o).astype(np.int64) * times
    al = alleles_of(lengths, events(lengths, records, words, reads, o), times)
    return call(text, lengths, cnt, al, o), al


def random_text(rng, n):
    """n ranks, mostly A C G T, with ranks 0 and 5 among them"""
    return rng.choice(np.arange(6, dtype=np.uint8), size=int(n), p=[0.02, 0.235, 0.235, 0.235, 0.235, 0.04])


def vcf_lines(rows, names, chroms):
    """the data lines of the tool's VCF for these rows; chroms: the rank arrays of the sequences"""
    out = []
    for v in rows:
        text = chroms[int(v["ref"])]
        pos, length = int(v["pos"]), int(v["length"])
        ref = "NACGTN"[int(text[pos])]
        alt = ref
        if int(v["kind"]) == SNV:
            alt = "NACGT"[int(v["alt_rank"])]
        elif int(v["kind"]) == DEL:
            ref += "".join("NACGTN"[int(x)] for x in text[pos + 1: pos + 1 + length])
        else:
            alt += letters_of(v["letters"], length)
        q = int(v["qual"])
        out.append(f"{names[int(v['ref'])]}\t{pos + 1}\t.\t{ref}\t{alt}\t{q // 100}.{q % 100:02d}\t.\tDP={int(v['cov'])}\tGT:GQ:DP:AD:PL\t{'0/1' if int(v['gt']) == RA else '1/1'}:"
                   f"{int(v['gq'])}:{int(v['cov'])}:{int(v['ref_count'])},{int(v['alt_count'])}:{int(v['pl'][0])},{int(v['pl'][1])},{int(v['pl'][2])}\n")
    return out
