"""The structural-variant signature rule in plain Python, written from the rule's text (include/floxer_amd.h) and independent of
floxer_amd/csrc/flx_sv.hpp: tuples, sorted() and loops, no ordering tricks. The expected value of tests/test_sv_host.py and
tests/test_sv_gpu.py.

A signature is the tuple (type, side_a, side_b, ref_a, ref_b, pos_a, q); that tuple's order is the key order."""
import numpy as np

import floxer_amd as F

OPS = {"M": 0, "I": 1, "D": 2, "N": 3, "S": 4, "H": 5, "P": 6, "=": 7, "X": 8}
DEL, INS, BND = 0, 1, 2
L, R = 0, 1
REC_DTYPE = F._REC_DTYPE


def word(op, n):
    return (int(n) << 4) | OPS[op]


def options(min_length=0, max_distance=0, min_support=0, count_secondary=False, min_mapq=0):
    return dict(min_length=min_length, max_distance=max_distance, min_support=min_support, count_secondary=count_secondary, min_mapq=min_mapq)


def c_options(o, initial_capacity=0):
    return F.sv_options(initial_capacity=initial_capacity, **o)


def thresholds(o):
    return o["min_length"] or 50, o["max_distance"] or 100, o["min_support"] or 2


def records_of(rows):
    """rows: (flag, ref, pos, read, mapq, [words]) -> (records, word pool); every row gets its own words"""
    rec = np.zeros(len(rows), dtype=REC_DTYPE)
    pool = []
    for i, (flag, ref, pos, read, mapq, ws) in enumerate(rows):
        rec[i] = (read, flag, ref, pos, 0, len(pool), len(ws), mapq)
        pool.extend(ws)
    return rec, np.array(pool, dtype=np.uint32)


def query_rows(ws):
    """the letters a word list consumes of its read"""
    return sum(w >> 4 for w in ws if (w & 15) in (7, 8, 1, 4))


def counts(r, o):
    flag = int(r["flag"])
    if flag & 4:
        return False
    if (flag & 256) and not o["count_secondary"]:
        return False
    if o["min_mapq"] > 0 and int(r["res"]) < o["min_mapq"]:
        return False
    return True


def signatures(records, words, read_lengths, o):
    """every signature of the records, sorted: a list of tuples"""
    min_length = thresholds(o)[0]
    out = []
    groups = []                                                          # lists of (query_start, index, ref, rs, re, reverse)
    prev_read = None
    for i, r in enumerate(records):
        read = int(r["read"])
        if prev_read is None or read != prev_read:
            groups.append([])
        prev_read = read
        if not counts(r, o):
            continue
        ws = [int(w) for w in words[int(r["coff"]): int(r["coff"]) + int(r["clen"])]]
        ref, pos = int(r["ref"]), int(r["pos"])
        p = pos
        for w in ws:
            op, n = w & 15, w >> 4
            if op == 2 and n >= min_length:
                out.append((DEL, 0, 0, ref, ref, p, n))
            if op == 1 and n >= min_length:
                out.append((INS, 0, 0, ref, ref, p - 1 if p > pos else p, n))
            if op in (7, 8, 2):
                p += n
        if int(r["flag"]) & 256:
            continue
        lead = 0
        for w in ws:
            if w & 15 != 4:
                break
            lead += w >> 4
        trail = 0
        for w in reversed(ws):
            if w & 15 != 4:
                break
            trail += w >> 4
        reverse = bool(int(r["flag"]) & 16)
        groups[-1].append((trail if reverse else lead, i, ref, pos, p, reverse))
    for g in groups:
        g = sorted(g)                                                    # by (query_start, index)
        for a, b in zip(g, g[1:]):
            end_a = (a[2], a[3], L) if a[5] else (a[2], a[4] - 1, R)
            end_b = (b[2], b[4] - 1, R) if b[5] else (b[2], b[3], L)
            lo, hi = sorted([end_a, end_b])
            out.append((BND, lo[2], hi[2], lo[0], hi[0], lo[1], hi[1]))
    return sorted(out)


def clusters(sigs, o):
    """the clusters of a list of signature tuples in any order: tuples (type, side_a, side_b, support, ref_a, ref_b, pos_a_min, pos_a_max,
    q_min, q_median, q_max)"""
    _, max_distance, min_support = thresholds(o)
    sigs = sorted(sigs)
    coarse = []
    for s in sigs:
        if coarse and coarse[-1][-1][:5] == s[:5] and s[5] - coarse[-1][-1][5] <= max_distance:
            coarse[-1].append(s)
        else:
            coarse.append([s])
    out = []
    for group in coarse:
        members = sorted(group, key=lambda s: (s[6], s[5]))
        fine = []
        for s in members:
            if fine and s[6] - fine[-1][-1][6] <= max_distance:
                fine[-1].append(s)
            else:
                fine.append([s])
        for c in fine:
            if len(c) < min_support:
                continue
            qs = [s[6] for s in c]
            ps = [s[5] for s in c]
            out.append(c[0][:3] + (len(c),) + c[0][3:5] + (min(ps), max(ps), qs[0], qs[(len(c) - 1) // 2], qs[-1]))
    return out


def signature_array(sigs):
    out = np.zeros(len(sigs), dtype=F.SV_SIGNATURE_DTYPE)
    for i, (t, sa, sb, ra, rb, p, q) in enumerate(sigs):
        out[i] = (t, sa, sb, 0, ra, rb, p, q)
    return out


def cluster_array(cl):
    out = np.zeros(len(cl), dtype=F.SV_CLUSTER_DTYPE)
    for i, c in enumerate(cl):
        out[i] = c + (0,)
    return out


def signature_tuples(arr):
    return [(int(s["type"]), int(s["side_a"]), int(s["side_b"]), int(s["ref_a"]), int(s["ref_b"]), int(s["pos_a"]), int(s["q"])) for s in arr]


def tsv_lines(cl, names):
    """the CLI's output of a cluster array: one line per cluster"""
    lines = []
    for c in cl:
        t = int(c["type"])
        side = (lambda s: "LR"[int(s)]) if t == BND else (lambda s: ".")
        one = 1 if t == BND else 0                                       # q is a 1-based position for BND and a length otherwise
        lines.append("\t".join(str(x) for x in (F.SV_TYPES[t], names[int(c["ref_a"])], int(c["pos_a_min"]) + 1, int(c["pos_a_max"]) + 1, side(c["side_a"]),
                                                   names[int(c["ref_b"])], int(c["q_min"]) + one, int(c["q_median"]) + one, int(c["q_max"]) + one, side(c["side_b"]),
                                                   int(c["support"]))))
    return lines


def random_records(rng, lengths, n_reads, min_length=50, max_words=9):
    """reads of one to five neighbouring records with valid words: long and short D and I words, clips at the ends only, all the flags.
    Returns (records, words, read_lengths)."""
    rows, read_lengths = [], []
    assert min(lengths) >= 800                                           # (a read fits every sequence)
    for read in range(n_reads):
        n_rec = int(rng.integers(1, 6))
        read_len = int(rng.integers(400, 800))
        read_lengths.append(read_len)
        for k in range(n_rec):
            flag = int(rng.choice([0, 16, 2048, 2064, 256, 272, 4])) if k else int(rng.choice([0, 16, 4]))
            if flag == 4:
                rows.append((4, -1, 0, read, 0, []))
                continue
            ref = int(rng.integers(0, len(lengths)))
            ws = []
            left = read_len
            lead = int(rng.integers(0, 3)) * int(rng.integers(1, 80))
            if lead:
                ws.append(word("S", lead))
                left -= lead
            trail = int(rng.integers(0, 3)) * int(rng.integers(1, 80))
            left -= trail
            span = 0
            first = True
            for _ in range(int(rng.integers(0, max_words))):
                op = "=XID"[int(rng.integers(0, 4))]
                n = int(rng.choice([1, 3, min_length - 1, min_length, min_length + 30]))
                if op in "=XI" and n >= left - 1:
                    continue
                if op in "=XD" and span + n >= lengths[ref] - 1:
                    continue
                ws.append(word(op, n))
                if op in "=XI":
                    left -= n
                if op in "=XD":
                    span += n
                first = False
            ws.append(word("=" if first or rng.integers(0, 2) else "X", left))           # (left >= 1; the span may not fit: checked below)
            span += left
            if trail:
                ws.append(word("S", trail))
            if span > lengths[ref]:
                ws = [word("=", read_len)]
                span = read_len
            pos = int(rng.integers(0, lengths[ref] - span + 1))
            rows.append((flag, ref, pos, read, int(rng.integers(0, 61)), ws))
    rec, words = records_of(rows)
    return rec, words, read_lengths
