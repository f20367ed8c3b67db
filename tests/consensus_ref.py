"""The consensus rule (flx_consensus, include/floxer_amd.h) in plain numpy, for the tests: the counts are pileup_ref.counts', the alleles
come from a walk over the I words of the counted records, the call is vectorised over the positions, the letters are placed by a
cumulative sum; next to the call a naive position-by-position loop that the reference itself is checked against.

text: the uint8 ranks of the unpadded concatenation of the sequences; records, words, lengths, reads: as in pileup_ref. The results are
(letters, changes, alleles): a list of str per sequence and structured arrays of floxer_amd.CHANGE_DTYPE and ALLELE_DTYPE."""
import numpy as np

import floxer_amd as F
import pileup_ref as P
from pileup_ref import REC, records_of, records_with_reads, span, starts_of, word  # noqa: F401 (shared with the tests)

DEFAULTS = dict(min_depth=3, min_count=2, min_permille=500)
SUB, DEL, INS = 0, 1, 2
MAX_INS = 32
LETTERS = np.frombuffer(b"NACGTN", dtype=np.uint8)


def options(count_secondary=False, min_mapq=0, min_depth=0, min_count=0, min_permille=0, mask_low_depth=False):
    return dict(count_secondary=count_secondary, min_mapq=min_mapq, min_depth=min_depth, min_count=min_count, min_permille=min_permille,
                mask_low_depth=mask_low_depth)


def c_options(o):
    return F.consensus_options(**o)


def thresholds(o):
    return tuple(int(o[k]) or DEFAULTS[k] for k in ("min_depth", "min_count", "min_permille"))


def pack(letters):
    """ranks 1..4 -> the key's lo: letter k at bits 63 - 2k and 62 - 2k"""
    lo = 0
    for k, r in enumerate(letters):
        lo |= (int(r) - 1) << (62 - 2 * k)
    return lo


def unpack(lo, length):
    return [((int(lo) >> (62 - 2 * k)) & 3) + 1 for k in range(int(length))]


def key_of(anchor, letters):
    """(hi, lo) of an insertion behind `anchor` (None: no column precedes it), or the void key"""
    letters = [int(x) for x in letters]
    if anchor is None or not 1 <= len(letters) <= MAX_INS or any(not 1 <= x <= 4 for x in letters):
        return (1 << 64) - 1, (1 << 64) - 1
    return int(anchor) << 8 | len(letters), pack(letters)


def events(lengths, records, words, reads, o):
    """the allele key (anchor, length, lo) of every I word of every counted record that yields one, in record and word order"""
    starts = starts_of(lengths)
    out = []
    for rec in records:
        if not P.record_counts(rec, o):
            continue
        ws = [(int(w) & 15, int(w) >> 4) for w in words[int(rec["coff"]): int(rec["coff"]) + int(rec["clen"])]]
        if not any(op == 1 for op, _ in ws):
            continue
        seq = P.oriented(reads[int(rec["read"])], rec["flag"])
        origin = int(starts[int(rec["ref"])]) + int(rec["pos"])
        p, row = origin, 0
        for op, ln in ws:
            if op == 1:
                hi, lo = key_of(p - 1 if p > origin else None, seq[row: row + ln] if ln <= MAX_INS else [0])
                if hi != (1 << 64) - 1:
                    out.append((hi >> 8, hi & 255, lo))
            if op in (7, 8, 2):
                p += ln
            if op in (7, 8, 1, 4):
                row += ln
    return out


def alleles_of(lengths, evs, times=1):
    """the events grouped: a structured array of floxer_amd.ALLELE_DTYPE in key order, every count multiplied by `times`"""
    starts = starts_of(lengths)
    count = {}
    for e in evs:
        count[e] = count.get(e, 0) + times
    keys = sorted(count)
    out = np.zeros(len(keys), dtype=F.ALLELE_DTYPE)
    for i, (a, ln, lo) in enumerate(keys):
        ref = int(np.searchsorted(starts, a, side="right")) - 1
        out[i] = (ref, a - int(starts[ref]), ln, count[(a, ln, lo)], lo)
    return out


def winners(lengths, al):
    """{anchor in the concatenation: index of its winning allele}: the largest count, the first in key order among equals"""
    starts = starts_of(lengths)
    win = {}
    for i, a in enumerate(al):
        p = int(starts[int(a["ref"])]) + int(a["pos"])
        if p not in win or int(a["count"]) > int(al[win[p]]["count"]):
            win[p] = i
    return win


def call(text, lengths, cnt, al, o):
    """the call over all positions at once -> (letters, changes)"""
    starts = starts_of(lengths)
    total = int(starts[-1])
    min_depth, min_count, min_permille = thresholds(o)
    c = np.asarray(cnt, dtype=np.int64)
    R = np.asarray(text, dtype=np.int64)
    at = np.arange(total)
    cov = c[P.DEPTH] + c[P.DEL]
    n = np.zeros((6, total), dtype=np.int64)
    n[1:5] = c[P.A:P.T + 1]
    n[5] = c[P.DEL]
    letter = (R >= 1) & (R <= 4)
    n[R[letter], at[letter]] += (c[P.DEPTH] - c[P.A:P.T + 1].sum(axis=0))[letter]
    best = np.argmax(n[1:], axis=0) + 1                                   # (the first of the largest: A, C, G, T, DEL)
    tied_with_r = letter & (n[np.where(letter, R, 1), at] == n[best, at])
    best = np.where(tied_with_r, R, best)
    nb = n[best, at]
    called = cov >= min_depth
    is_r = letter & (best == R)                                           # (R = 5 is the letter N, best = 5 the deletion)
    stands = called & ~is_r & (nb >= min_count) & (nb * 1000 >= min_permille * cov)
    emit = np.where(letter, R, 5)
    if o["mask_low_depth"]:
        emit = np.where(called, emit, 5)
    emit = np.where(stands, np.where(best == 5, 0, best), emit)
    ins_len = np.zeros(total, dtype=np.int64)
    ins_rows = []
    for p, i in sorted(winners(lengths, al).items()):
        k = int(al[i]["count"])
        if called[p] and k >= min_count and k * 1000 >= min_permille * int(cov[p]):
            ins_len[p] = int(al[i]["length"])
            ins_rows.append((p, i))
    # the letters
    out_len = (emit > 0).astype(np.int64) + ins_len
    end = np.cumsum(out_len)
    begin = end - out_len
    pool = np.zeros(int(end[-1]) if total else 0, dtype=np.uint8)
    own = emit > 0
    pool[begin[own]] = LETTERS[emit[own]]
    for p, i in ins_rows:
        first = int(begin[p]) + (1 if emit[p] > 0 else 0)
        pool[first: first + int(ins_len[p])] = LETTERS[unpack(al[i]["letters"], al[i]["length"])]
    text_out = pool.tobytes().decode("ascii")
    bounds = [int(begin[int(s)]) if int(s) < total else int(end[-1]) for s in starts[:-1]] + [int(end[-1])]
    letters = [text_out[bounds[r]: bounds[r + 1]] for r in range(len(lengths))]
    # the changes: SUB or DEL in front of the INS of the same position
    rows = np.zeros(int(stands.sum()) + len(ins_rows), dtype=F.CHANGE_DTYPE)
    order = np.zeros(len(rows), dtype=np.int64)
    sp = at[stands]
    k = len(sp)
    ref = np.searchsorted(starts, sp, side="right") - 1
    rows["ref"][:k], rows["pos"][:k] = ref, sp - starts[ref]
    rows["kind"][:k] = np.where(best[sp] == 5, DEL, SUB)
    rows["ref_rank"][:k], rows["alt_rank"][:k] = R[sp], np.where(best[sp] == 5, 0, best[sp])
    rows["length"][:k], rows["count"][:k], rows["cov"][:k] = 1, nb[sp], cov[sp]
    order[:k] = sp * 2
    for j, (p, i) in enumerate(ins_rows):
        r = int(np.searchsorted(starts, p, side="right")) - 1
        rows[k + j] = (r, p - int(starts[r]), INS, int(R[p]), 0, int(al[i]["length"]), int(al[i]["count"]), int(cov[p]), int(al[i]["letters"]))
        order[k + j] = p * 2 + 1
    return letters, rows[np.argsort(order, kind="stable")]


def call_naive(text, lengths, cnt, al, o):
    """one position at a time, as the rule is written"""
    starts = starts_of(lengths)
    min_depth, min_count, min_permille = thresholds(o)
    win = winners(lengths, al)
    letters, rows = [], []
    for r in range(len(lengths)):
        s = []
        for p in range(int(starts[r]), int(starts[r + 1])):
            v = [int(cnt[k][p]) for k in range(7)]
            R, cov = int(text[p]), v[P.DEPTH] + v[P.DEL]
            own = "NACGTN"[R]
            if cov < min_depth:
                s.append("N" if o["mask_low_depth"] else own)
                continue
            n = {1: v[P.A], 2: v[P.C], 3: v[P.G], 4: v[P.T], 5: v[P.DEL]}
            if 1 <= R <= 4:
                n[R] += v[P.DEPTH] - v[P.A] - v[P.C] - v[P.G] - v[P.T]
            top = max(n.values())
            best = R if 1 <= R <= 4 and n[R] == top else min(k for k in n if n[k] == top)
            if not (1 <= R <= 4 and best == R) and n[best] >= min_count and n[best] * 1000 >= min_permille * cov:
                rows.append((r, p - int(starts[r]), DEL if best == 5 else SUB, R, 0 if best == 5 else best, 1, n[best], cov, 0))
                s.append("" if best == 5 else "NACGT"[best])
            else:
                s.append(own)
            if p in win:
                a = al[win[p]]
                if int(a["count"]) >= min_count and int(a["count"]) * 1000 >= min_permille * cov:
                    rows.append((r, p - int(starts[r]), INS, R, 0, int(a["length"]), int(a["count"]), cov, int(a["letters"])))
                    s.append("".join("NACGT"[x] for x in unpack(a["letters"], a["length"])))
        letters.append("".join(s))
    return letters, np.array(rows, dtype=F.CHANGE_DTYPE) if rows else np.zeros(0, dtype=F.CHANGE_DTYPE)


def consensus(text, lengths, records, words, reads, o, times=1):
    """the whole rule -> (letters, changes, alleles); times: every record counts that often"""
    cnt = P.counts(lengths, records, words, reads, o).astype(np.int64) * times
    al = alleles_of(lengths, events(lengths, records, words, reads, o), times)
    letters, changes = call(text, lengths, cnt, al, o)
    return letters, changes, al


def random_text(rng, n):
    """n ranks, mostly A C G T, with ranks 0 and 5 among them"""
    return rng.choice(np.arange(6, dtype=np.uint8), size=int(n), p=[0.02, 0.235, 0.235, 0.235, 0.235, 0.04])
