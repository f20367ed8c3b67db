"""The allele-pileup rule (flx_pileup, include/floxer_amd.h) in plain numpy, for the tests: difference arrays for DEPTH and DEL plus
np.add.at for the letters and the insertion anchors, then the site table; next to each a naive column-by-column loop that the
reference itself is checked against.

records, words, lengths: as in coverage_ref; reads: a list of uint8 rank arrays indexed by the records' `read`; counts are (7, total)
uint32 in the order DEPTH, DEL, A, C, G, T, INS over the unpadded concatenation of the sequences."""
import numpy as np

import floxer_amd as F
from coverage_ref import REC, counts as record_counts, random_records, records_across, records_of, span, starts_of, word  # noqa: F401 (shared with the tests)

DEPTH, DEL, A, C, G, T, INS = range(7)
COMPLEMENT = np.array([0, 4, 3, 2, 1, 5], dtype=np.uint8)
DEFAULTS = dict(min_depth=4, min_count=2, min_permille=200)


def options(count_secondary=False, min_mapq=0, min_depth=0, min_count=0, min_permille=0):
    return dict(count_secondary=count_secondary, min_mapq=min_mapq, min_depth=min_depth, min_count=min_count, min_permille=min_permille)


def c_options(o):
    return F.pileup_options(**o)


def oriented(read, flag):
    """the read as SEQ has it: as given, or its reverse complement for flag bit 16"""
    read = np.asarray(read, dtype=np.uint8)
    return COMPLEMENT[read[::-1]] if int(flag) & 16 else read


def query_length(ws):
    return sum(int(w) >> 4 for w in ws if int(w) & 15 in (7, 8, 1, 4))


def counts(lengths, records, words, reads, o):
    """difference arrays and scattered adds, then cumsum"""
    starts = starts_of(lengths)
    total = int(starts[-1])
    diff = np.zeros((2, total + 1), dtype=np.int64)
    planes = np.zeros((7, total), dtype=np.int64)
    words = np.asarray(words, dtype=np.uint32)
    for rec in records:
        if not record_counts(rec, o):
            continue
        w = words[int(rec["coff"]): int(rec["coff"]) + int(rec["clen"])].astype(np.int64)
        op, ln = w & 15, w >> 4
        cols = np.where(np.isin(op, (7, 8, 2)), ln, 0)
        rows = np.where(np.isin(op, (7, 8, 1, 4)), ln, 0)
        origin = int(starts[int(rec["ref"])]) + int(rec["pos"])
        first = origin + np.concatenate([[0], np.cumsum(cols)[:-1]])
        first_row = np.concatenate([[0], np.cumsum(rows)[:-1]])
        for plane, sel in ((0, (op == 7) | (op == 8)), (1, op == 2)):
            np.add.at(diff[plane], first[sel], 1)
            np.add.at(diff[plane], (first + ln)[sel], -1)
        x = op == 8
        if x.any():
            seq = oriented(reads[int(rec["read"])], rec["flag"])
            within = np.arange(int(ln[x].sum())) - np.repeat(np.cumsum(ln[x]) - ln[x], ln[x])
            pos = np.repeat(first[x], ln[x]) + within
            letter = seq[np.repeat(first_row[x], ln[x]) + within].astype(np.int64)
            keep = (letter >= 1) & (letter <= 4)
            np.add.at(planes, (A + letter[keep] - 1, pos[keep]), 1)
        i = op == 1
        np.add.at(planes[INS], np.where(first[i] > origin, first[i] - 1, first[i]), 1)
    planes[DEPTH] = np.cumsum(diff[0][:-1])
    planes[DEL] = np.cumsum(diff[1][:-1])
    return planes.astype(np.uint32)


def counts_naive(lengths, records, words, reads, o):
    """one column at a time"""
    starts = starts_of(lengths)
    out = np.zeros((7, int(starts[-1])), dtype=np.uint32)
    for rec in records:
        if not record_counts(rec, o):
            continue
        seq = oriented(reads[int(rec["read"])], rec["flag"])
        p = int(starts[int(rec["ref"])]) + int(rec["pos"])
        row, last = 0, None                                              # last: the preceding reference-consuming column
        ws = [(int(w) & 15, int(w) >> 4) for w in words[int(rec["coff"]): int(rec["coff"]) + int(rec["clen"])]]
        for op, ln in ws:
            if op == 1:
                out[INS][last if last is not None else p] += 1           # (no column yet: the cursor is the record's first column)
                row += ln
            elif op == 4:
                row += ln
            else:
                for _ in range(ln):
                    if op == 2:
                        out[DEL][p] += 1
                    else:
                        out[DEPTH][p] += 1
                        if op == 8 and 1 <= int(seq[row]) <= 4:
                            out[A + int(seq[row]) - 1][p] += 1
                        row += 1
                    last = p
                    p += 1
    return out


def thresholds(o):
    return tuple(int(o[k]) or DEFAULTS[k] for k in ("min_depth", "min_count", "min_permille"))


def sites(lengths, cnt, o):
    """the site table of a (7, total) count array: a structured array of floxer_amd.SITE_DTYPE in position order"""
    starts = starts_of(lengths)
    min_depth, min_count, min_permille = thresholds(o)
    c = np.asarray(cnt, dtype=np.int64)
    cov = c[DEPTH] + c[DEL]
    best = c[1:].max(axis=0)
    at = np.nonzero((cov >= min_depth) & (best >= min_count) & (best * 1000 >= min_permille * cov))[0]
    ref = np.searchsorted(starts, at, side="right") - 1
    out = np.zeros(len(at), dtype=F.SITE_DTYPE)
    out["ref"], out["pos"], out["depth"], out["del"], out["ins"] = ref, at - starts[ref], c[DEPTH][at], c[DEL][at], c[INS][at]
    out["alt"] = c[A:T + 1, at].T
    return out


def sites_naive(lengths, cnt, o):
    starts = starts_of(lengths)
    min_depth, min_count, min_permille = thresholds(o)
    rows = []
    for r in range(len(lengths)):
        for p in range(int(starts[r]), int(starts[r + 1])):
            v = [int(cnt[k][p]) for k in range(7)]
            cov, best = v[DEPTH] + v[DEL], max(v[1:])
            if cov >= min_depth and best >= min_count and best * 1000 >= min_permille * cov:
                rows.append((r, p - int(starts[r]), v[DEPTH], v[DEL], v[INS], v[A:T + 1], 0))
    return np.array(rows, dtype=F.SITE_DTYPE) if rows else np.zeros(0, dtype=F.SITE_DTYPE)


# ---- inputs
def random_read(rng, n):
    """n ranks, mostly A C G T, with ranks 0 and 5 among them"""
    return rng.choice(np.arange(6, dtype=np.uint8), size=int(n), p=[0.05, 0.2125, 0.2125, 0.2125, 0.2125, 0.1])


def attach_reads(rng, records, words):
    """one read per record, of exactly the record's query length; the records' `read` is set to its index. Returns the list of reads."""
    reads = []
    for i in range(len(records)):
        ws = words[int(records[i]["coff"]): int(records[i]["coff"]) + int(records[i]["clen"])]
        records[i]["read"] = i
        reads.append(random_read(rng, query_length(ws)))
    return reads


def records_with_reads(rng, rows):
    """rows as coverage_ref.records_of takes them -> (records, words, reads)"""
    rec, words = records_of(rows)
    return rec, words, attach_reads(rng, rec, words)
