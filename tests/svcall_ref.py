"""The structural-variant calling rule (floxer_amd/csrc/flx_svcall.hpp) in plain numpy and Python: the spans of the counted records, the
count of a cluster by brute force over all spans (no sort, no window, no max_span), the genotype and the rows. Every expected value of
the svcall tests comes from here. Clusters are tests/sv_ref.py's tuples (type, side_a, side_b,
support, ref_a, ref_b, pos_a_min, pos_a_max, q_min, q_median, q_max) or a structured array of F.SV_CLUSTER_DTYPE."""
import numpy as np

import floxer_amd as F
import sv_ref as S

DEL, INS, BND = S.DEL, S.INS, S.BND
DEFAULT_COSTS = (36, 1574, 325, 3000, 3301)
COST_NAMES = ("cost_match", "cost_mismatch", "cost_het", "prior_het", "prior_hom")
U32 = 0xFFFFFFFF


def options(count_secondary=False, min_mapq=0, flank=0, min_depth=0, min_qual=0, cost_match=0, cost_mismatch=0, cost_het=0, prior_het=0, prior_hom=0):
    return dict(count_secondary=count_secondary, min_mapq=min_mapq, flank=flank, min_depth=min_depth, min_qual=min_qual, cost_match=cost_match,
                cost_mismatch=cost_mismatch, cost_het=cost_het, prior_het=prior_het, prior_hom=prior_hom)


def c_options(o):
    return F.svcall_options(**o)


def model(o):
    """(flank, min_depth, min_qual, m, x, h, prior_het, prior_hom) with the defaults taken for 0"""
    return (o["flank"] or 50, o["min_depth"] or 4, o["min_qual"] or 2000) + tuple(o[n] or d for n, d in zip(COST_NAMES, DEFAULT_COSTS))


def cluster_tuples(clusters):
    if isinstance(clusters, np.ndarray):
        return [tuple(int(c[n]) for n in ("type", "side_a", "side_b", "support", "ref_a", "ref_b", "pos_a_min", "pos_a_max", "q_min", "q_median", "q_max")) for c in clusters]
    return [tuple(int(x) for x in c) for c in clusters]


def spans(records, words, o):
    """(ref, rs, re) of every counted record, in the records' order"""
    out = []
    for r in records:
        if not S.counts(r, o):
            continue
        off, n = int(r["coff"]), int(r["clen"])
        cols = sum(int(w) >> 4 for w in words[off: off + n] if (int(w) & 15) in (7, 8, 2))
        out.append((int(r["ref"]), int(r["pos"]), int(r["pos"]) + cols))
    return out


def genotype(ref_n, alt_n, o):
    """(gt, gq, qual, pl0, pl1, pl2) of flx_variants' rule with oth = 0"""
    _, _, _, m, x, h, prior_het, prior_hom = model(o)
    L = [ref_n * m + alt_n * x, (ref_n + alt_n) * h, alt_n * m + ref_n * x]
    Q = [L[0], L[1] + prior_het, L[2] + prior_hom]
    gt = 0
    for g in (1, 2):
        if Q[g] < Q[gt]:
            gt = g
    second = min(Q[g] for g in range(3) if g != gt)
    gq = min((second - Q[gt]) // 100, 99)
    alt_q = min(Q[1], Q[2])
    qual = min(Q[0] - alt_q, U32) if Q[0] > alt_q else 0
    return (gt, gq, qual) + tuple(min((l - min(L)) // 100, U32) for l in L)


def bounds(c, n_r, flank):
    t, _, _, _, _, _, pmin, pmax, _, _, qmax = c
    lo = pmin
    hi = pmax + qmax if t == DEL else pmax + 1
    return (lo - flank if lo >= flank else 0), min(hi + flank, n_r)


def rows(span_list, clusters, lengths, o):
    """one tuple per DEL / INS cluster, in F.SVCALL_ROW_DTYPE's field order with pl flattened; the count walks every span"""
    flank, min_depth, min_qual = model(o)[:3]
    out = []
    all_spans = np.asarray(list(span_list), dtype=np.int64).reshape(-1, 3)
    for i, c in enumerate(cluster_tuples(clusters)):
        t, _, _, support, ref, _, pmin, pmax, qmin, qmed, qmax = c
        if t == BND:
            continue
        lo2, hi2 = bounds(c, int(lengths[ref]), flank)
        span_n = int(np.count_nonzero((all_spans[:, 0] == ref) & (all_spans[:, 1] <= lo2) & (all_spans[:, 2] >= hi2)))      # every span is asked
        alt_n = support
        ref_n = span_n - alt_n if span_n > alt_n else 0
        g = genotype(ref_n, alt_n, o)
        ok = 1 if g[0] != 0 and ref_n + alt_n >= min_depth and g[2] >= min_qual else 0
        out.append((i, t, ref, pmin, pmax, qmin, qmed, qmax, alt_n, ref_n, span_n) + g + (ok,))
    return out


def row_array(rws):
    out = np.zeros(len(rws), dtype=F.SVCALL_ROW_DTYPE)
    for i, r in enumerate(rws):
        out[i] = r[:14] + (list(r[14:17]), r[17])
    return out


def row_tuples(arr):
    return [tuple(int(r[n]) for n in ("cluster", "type", "ref", "pos_a_min", "pos_a_max", "q_min", "q_median", "q_max", "alt_n", "ref_n", "span_n", "gt", "gq", "qual"))
            + tuple(int(x) for x in r["pl"]) + (int(r["pass"]),) for r in arr]


def expected(records, words, clusters, lengths, o):
    return row_array(rows(spans(records, words, o), clusters, lengths, o))


def random_clusters(rng, lengths, n, with_bnd=True):
    """valid clusters of all three types over the sequences, some at position 0 and some at their sequence's end"""
    out = []
    for _ in range(n):
        t = int(rng.integers(0, 3 if with_bnd else 2))
        ref = int(rng.integers(0, len(lengths)))
        n_r = int(lengths[ref])
        qmin = int(rng.integers(1, 120))
        qmed = qmin + int(rng.integers(0, 40))
        qmax = qmed + int(rng.integers(0, 40))
        room = n_r - qmax if t == DEL else n_r - 1
        if t == BND:
            other = int(rng.integers(0, len(lengths)))
            out.append((BND, int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(1, 9)), min(ref, other), max(ref, other), 3, 9, 1, 4, 8))
            continue
        if room < 0:
            continue
        mode = int(rng.integers(0, 6))
        pmax = room if mode == 0 else int(rng.integers(0, room + 1))
        pmin = 0 if mode == 1 else int(rng.integers(max(0, pmax - 150), pmax + 1))
        out.append((t, 0, 0, int(rng.integers(1, 12)), ref, ref, pmin, pmax, qmin, qmed, qmax))
    return out
