"""The depth-of-coverage rule (flx_coverage, include/floxer_amd.h) in plain numpy, for the tests: a difference array from each counted
record's CIGAR, then cumsum, runs and windows; next to it a naive column-by-column loop that the reference itself is checked against.

records: a numpy array of floxer_amd's record dtype (read, flag, ref, pos, nm, coff, clen, res); words: the uint32 CIGAR pool (len << 4 |
op; I=1 D=2 S=4 '='=7 X=8); lengths: the reference lengths; depth is indexed by position in their unpadded concatenation."""
import numpy as np

import floxer_amd as F

REC = F._REC_DTYPE
CONSUMES = (7, 8, 2)


def options(count_deletions=False, count_secondary=False, min_mapq=0, report_zero=False):
    return dict(count_deletions=count_deletions, count_secondary=count_secondary, min_mapq=min_mapq, report_zero=report_zero)


def c_options(o):
    return F.coverage_options(**o)


def counts(rec, o):
    if rec["flag"] & 4:
        return False
    if rec["flag"] & 256 and not o["count_secondary"]:
        return False
    if o["min_mapq"] > 0 and rec["res"] < o["min_mapq"]:
        return False
    return True


def starts_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])


def depth(lengths, records, words, o):
    """difference array, then cumsum"""
    starts = starts_of(lengths)
    diff = np.zeros(int(starts[-1]) + 1, dtype=np.int64)
    words = np.asarray(words, dtype=np.uint32)
    for rec in records:
        if not counts(rec, o):
            continue
        w = words[int(rec["coff"]): int(rec["coff"]) + int(rec["clen"])].astype(np.int64)
        op, ln = w & 15, w >> 4
        cols = np.where(np.isin(op, CONSUMES), ln, 0)
        first = int(starts[int(rec["ref"])]) + int(rec["pos"]) + np.concatenate([[0], np.cumsum(cols)[:-1]])
        counted = (op == 7) | (op == 8) | ((op == 2) & bool(o["count_deletions"]))
        np.add.at(diff, first[counted], 1)
        np.add.at(diff, (first + ln)[counted], -1)
    return np.cumsum(diff[:-1]).astype(np.uint32)


def depth_naive(lengths, records, words, o):
    """one column at a time"""
    starts = starts_of(lengths)
    out = np.zeros(int(starts[-1]), dtype=np.uint32)
    for rec in records:
        if not counts(rec, o):
            continue
        p = int(starts[int(rec["ref"])]) + int(rec["pos"])
        for w in words[int(rec["coff"]): int(rec["coff"]) + int(rec["clen"])]:
            op, ln = int(w) & 15, int(w) >> 4
            for _ in range(ln):
                if op in (7, 8):
                    out[p] += 1
                    p += 1
                elif op == 2:
                    if o["count_deletions"]:
                        out[p] += 1
                    p += 1
    return out


def runs(lengths, d, report_zero=False):
    """maximal stretches of equal depth inside one sequence: a structured array of floxer_amd.RUN_DTYPE"""
    starts = starts_of(lengths)
    d = np.asarray(d, dtype=np.int64)
    head = np.ones(len(d), dtype=bool)
    head[1:] = d[1:] != d[:-1]
    head[starts[:-1]] = True                                             # a run never crosses a sequence boundary
    at = np.nonzero(head)[0]
    end = np.concatenate([at[1:], [len(d)]])
    ref = np.searchsorted(starts, at, side="right") - 1
    keep = np.ones(len(at), dtype=bool) if report_zero else d[at] > 0
    out = np.zeros(int(keep.sum()), dtype=F.RUN_DTYPE)
    out["ref"], out["depth"], out["start"], out["end"] = ref[keep], d[at][keep], (at - starts[ref])[keep], (end - starts[ref])[keep]
    return out


def runs_naive(lengths, d, report_zero=False):
    starts = starts_of(lengths)
    out = []
    for r in range(len(lengths)):
        seg = [int(x) for x in d[int(starts[r]): int(starts[r + 1])]]
        a = 0
        for p in range(1, len(seg) + 1):
            if p == len(seg) or seg[p] != seg[a]:
                if seg[a] or report_zero:
                    out.append((r, seg[a], a, p))
                a = p
    return np.array(out, dtype=F.RUN_DTYPE)


def windows(lengths, d, w=0):
    """per sequence and [k w, min((k + 1) w, len)): a structured array of floxer_amd.WINDOW_DTYPE; w = 0: one window per sequence"""
    starts = starts_of(lengths)
    parts = []
    for r in range(len(lengths)):
        seg = np.asarray(d[int(starts[r]): int(starts[r + 1])], dtype=np.uint64)
        size = int(w) if w else len(seg)
        edges = np.arange(0, len(seg), size)
        out = np.zeros(len(edges), dtype=F.WINDOW_DTYPE)
        out["ref"], out["start"], out["end"] = r, edges, np.minimum(edges + size, len(seg))
        out["depth_sum"], out["max_depth"] = np.add.reduceat(seg, edges), np.maximum.reduceat(seg, edges)
        out["covered"] = np.add.reduceat((seg > 0).astype(np.uint64), edges)
        parts.append(out)
    return np.concatenate(parts)


def windows_naive(lengths, d, w=0):
    starts = starts_of(lengths)
    out = []
    for r in range(len(lengths)):
        seg = [int(x) for x in d[int(starts[r]): int(starts[r + 1])]]
        size = int(w) if w else len(seg)
        for a in range(0, len(seg), size):
            part = seg[a: a + size]
            out.append((r, max(part), a, a + len(part), sum(part), sum(1 for x in part if x)))
    return np.array(out, dtype=F.WINDOW_DTYPE)


# ---- inputs
def word(op, ln):
    return (int(ln) << 4) | "MIDNSHP=X".index(op)


def records_of(rows, pool_offset=0):
    """rows: (flag, ref, pos, mapq, [words]) -> (records, words); every record gets its own words"""
    rec = np.zeros(len(rows), dtype=REC)
    words = []
    for i, (flag, ref, pos, mapq, ws) in enumerate(rows):
        rec[i] = (i, flag, ref, pos, 0, pool_offset + len(words), len(ws), mapq)
        words += list(ws)
    return rec, np.array(words, dtype=np.uint32)


def span(ws):
    return sum(int(w) >> 4 for w in ws if int(w) & 15 in CONSUMES)


def random_words(rng, n_words, max_len=12, clips=True):
    """n_words CIGAR words: = runs with X, I and D between them, optionally soft clips at the ends; never a zero length"""
    body = n_words - (2 if clips and n_words >= 3 else 0)
    ws = []
    for t in range(body):
        op = "=" if t % 2 == 0 else "XID"[int(rng.integers(0, 3))]
        ws.append(word(op, int(rng.integers(1, max_len + 1))))
    if body < n_words:
        ws = [word("S", int(rng.integers(1, 50)))] + ws + [word("S", int(rng.integers(1, 50)))]
    return ws


def joined(parts):
    """(records, words) pairs, each over its own pool -> one pair over the pools' concatenation"""
    recs, pools, at = [], [], 0
    for rec, words in parts:
        rec = rec.copy()
        rec["coff"] += at
        at += len(words)
        recs.append(rec)
        pools.append(words)
    return np.concatenate(recs), np.concatenate(pools)


def records_across(rng, at, tail):
    """records on one sequence of at + tail positions (tail >= 3) whose array is handled in pieces of `at` entries. First, each of them
    twice in a row (so that the even and the odd records both hold them): records on position 0, on the positions either side of index
    `at`, one across it with an X, an I and a D there, and on the last position. Behind them random records: 300 anywhere, 150 within 300
    positions of the start, 150 within 300 positions in front of index `at` up to the end."""
    rows = [(0, 0, 0, 0, [word("X", 2), word("=", 8)]),
            (16, 0, at - 3, 0, [word("=", 2), word("X", 1), word("I", 2), word("X", 1), word("D", 1), word("=", 1)]),     # X on at - 1 and on at, D on at + 1
            (0, 0, at - 1, 0, [word("X", 1)]), (0, 0, at, 0, [word("X", 1)]), (0, 0, at + tail - 1, 0, [word("X", 1)]),
            (16, 0, at - 1000, 0, [word("=", 1000 + tail - 1), word("I", 1), word("X", 1)])]                                # ends with the sequence
    near = random_records(rng, [300 + tail], 150, max_words=12)
    near[0]["pos"] += at - 300
    return joined([records_of([row for row in rows for _ in range(2)]), random_records(rng, [at + tail], 300, max_words=40),
                   random_records(rng, [300], 150, max_words=12), near])


def random_records(rng, lengths, n, max_words=9):
    """n records of every flag and mapping quality, placed so that they fit their sequences"""
    rows = []
    while len(rows) < n:
        ws = random_words(rng, int(rng.integers(1, max_words + 1)), clips=bool(rng.integers(0, 2)))
        ref = int(rng.integers(0, len(lengths)))
        if span(ws) > lengths[ref]:
            continue
        flag = int(rng.choice([0, 16, 256, 272, 2048, 2064, 4]))
        rows.append((flag, ref, int(rng.integers(0, lengths[ref] - span(ws) + 1)), int(rng.choice([0, 3, 60])), ws))
    return records_of(rows)
