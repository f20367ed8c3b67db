"""The error-profile rule (flx_errprof, include/floxer_amd.h) in plain numpy, for the tests: every word's columns and rows expanded into
index arrays and counted with np.add.at, the homopolymer runs read off slices of the text; next to it a naive loop that walks every
column and every position of a run on its own, which the reference itself is checked against; and the text form of a table as the CLI
writes it.

text: the uint8 ranks (0..5) of the unpadded concatenation of the sequences; lengths: their lengths; records, words: as in coverage_ref;
reads: a list of uint8 rank arrays indexed by the records' `read`. A table is a dict of uint64 arrays by the names of SECTIONS."""
import numpy as np

import floxer_amd as F
from coverage_ref import REC, counts as record_counts, random_words, records_of, span, starts_of, word  # noqa: F401 (shared with the tests)
from pileup_ref import attach_reads, oriented, query_length, random_read, records_with_reads  # noqa: F401

SECTIONS = (("PAIR_EQ", 36), ("PAIR_X", 36), ("INS_LEN", 64), ("DEL_LEN", 64), ("INS_LETTER", 6), ("DEL_LETTER", 6), ("HP_DEL", 34), ("HP_INS", 34),
            ("POS_MATCH", 100), ("POS_MISMATCH", 100), ("POS_INS", 100), ("POS_CLIP", 100), ("POS_DEL", 100), ("EQ_RUN", 256), ("IDENTITY", 101), ("TOTALS", 8))
TOTALS = ("records", "matches", "mismatches", "ins_events", "ins_bases", "del_events", "del_bases", "clip_bases")
LETTERS = ".ACGTN"


def options(count_secondary=False, min_mapq=0):
    return dict(count_secondary=count_secondary, min_mapq=min_mapq)


def c_options(o, flush_threshold=0):
    return F.errprof_options(flush_threshold=flush_threshold, **o)


def empty():
    return {name: np.zeros(n, dtype=np.uint64) for name, n in SECTIONS}


def same(a, b):
    """the entries in which two tables differ: [(section, index, a's, b's)]"""
    assert set(a) == set(b) == {name for name, _ in SECTIONS}
    return [(name, int(i), int(a[name][i]), int(b[name][i])) for name, _ in SECTIONS for i in np.nonzero(np.asarray(a[name]) != np.asarray(b[name]))[0]]


def times(t, n):
    return {k: v * np.uint64(n) for k, v in t.items()}


def plus(a, b):
    return {k: a[k] + b[k] for k in a}


def _expand(first, ln):
    """the members of the stretches [first[i], first[i] + ln[i])"""
    if len(ln) == 0:
        return np.zeros(0, dtype=np.int64)
    within = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
    return np.repeat(first, ln) + within


def _run(stretch, a):
    """leading entries of `stretch` equal to a"""
    differ = np.nonzero(stretch != a)[0]
    return int(differ[0]) if len(differ) else len(stretch)


def table(text, lengths, records, words, reads, o, into=None):
    """index arrays and np.add.at"""
    text = np.asarray(text, dtype=np.uint8)
    starts = starts_of(lengths)
    words = np.asarray(words, dtype=np.uint32)
    T = {k: v.astype(np.int64) for k, v in (into if into is not None else empty()).items()}
    for rec in records:
        if not record_counts(rec, o):
            continue
        w = words[int(rec["coff"]): int(rec["coff"]) + int(rec["clen"])].astype(np.int64)
        op, ln = w & 15, w >> 4
        seq = oriented(reads[int(rec["read"])], rec["flag"]).astype(np.int64)
        n, reverse = len(seq), bool(int(rec["flag"]) & 16)
        s0, s1 = int(starts[int(rec["ref"])]), int(starts[int(rec["ref"]) + 1])
        cols = np.where(np.isin(op, (7, 8, 2)), ln, 0)
        rows = np.where(np.isin(op, (7, 8, 1, 4)), ln, 0)
        first = s0 + int(rec["pos"]) + np.cumsum(cols) - cols
        first_row = np.cumsum(rows) - rows

        def bins(r):
            r = np.asarray(r, dtype=np.int64)
            return ((n - 1 - r) if reverse else r) * 100 // n
        for code, name in ((7, "PAIR_EQ"), (8, "PAIR_X")):
            sel = op == code
            t, q = text[_expand(first[sel], ln[sel])].astype(np.int64), seq[_expand(first_row[sel], ln[sel])]
            np.add.at(T[name], t * 6 + q, 1)
        for code, name in ((7, "POS_MATCH"), (8, "POS_MISMATCH"), (1, "POS_INS"), (4, "POS_CLIP")):
            sel = op == code
            if sel.any():
                np.add.at(T[name], bins(_expand(first_row[sel], ln[sel])), 1)
        ins, dele = op == 1, op == 2
        np.add.at(T["INS_LEN"], np.minimum(ln[ins], 64) - 1, 1)
        np.add.at(T["DEL_LEN"], np.minimum(ln[dele], 64) - 1, 1)
        np.add.at(T["EQ_RUN"], np.minimum(ln[op == 7], 256) - 1, 1)
        np.add.at(T["INS_LETTER"], seq[_expand(first_row[ins], ln[ins])], 1)
        np.add.at(T["DEL_LETTER"], text[_expand(first[dele], ln[dele])].astype(np.int64), 1)
        if dele.any():
            np.add.at(T["POS_DEL"], bins(np.minimum(first_row[dele], n - 1)) if n else np.zeros(int(dele.sum()), dtype=np.int64), 1)
        for p, r, L in zip(first[ins], first_row[ins], ln[ins]):
            p, r, L = int(p), int(r), int(L)
            a = int(seq[r])
            if not 1 <= a <= 4 or (seq[r: r + L] != a).any():
                T["HP_INS"][33] += 1
            else:
                left = _run(text[max(s0, p - 32): p][::-1], a)
                right = _run(text[p: min(s1, p + 32)], a)
                T["HP_INS"][min(32, left + right)] += 1
        for p, L in zip(first[dele], ln[dele]):
            p, L = int(p), int(L)
            a = int(text[p])
            if not 1 <= a <= 4 or (text[p: p + L] != a).any():
                T["HP_DEL"][33] += 1
            else:
                left = _run(text[max(s0, p - 32): p][::-1], a)
                right = _run(text[p + L: min(s1, p + L + 32)], a)
                T["HP_DEL"][min(32, left + L + right)] += 1
        m, x, ib, db = int(ln[op == 7].sum()), int(ln[op == 8].sum()), int(ln[ins].sum()), int(ln[dele].sum())
        T["IDENTITY"][m * 100 // (m + x + ib + db)] += 1
        T["TOTALS"] += np.array([1, m, x, int(ins.sum()), ib, int(dele.sum()), db, int(ln[op == 4].sum())], dtype=np.int64)
    return {k: v.astype(np.uint64) for k, v in T.items()}


def table_naive(text, lengths, records, words, reads, o):
    """one column, one row, one position of a run at a time"""
    starts = starts_of(lengths)
    T = {name: [0] * n for name, n in SECTIONS}
    for rec in records:
        if not record_counts(rec, o):
            continue
        seq = [int(c) for c in oriented(reads[int(rec["read"])], rec["flag"])]
        n, reverse = len(seq), bool(int(rec["flag"]) & 16)
        s0, s1 = int(starts[int(rec["ref"])]), int(starts[int(rec["ref"]) + 1])
        p, r = s0 + int(rec["pos"]), 0
        tot = dict.fromkeys(TOTALS, 0)
        tot["records"] = 1

        def pos_bin(row):
            return ((n - 1 - row) if reverse else row) * 100 // n if n else 0

        def run(at, step, a):
            k = 0
            while k < 32 and s0 <= at < s1 and int(text[at]) == a:
                k, at = k + 1, at + step
            return k
        for wd in words[int(rec["coff"]): int(rec["coff"]) + int(rec["clen"])]:
            op, L = int(wd) & 15, int(wd) >> 4
            if op in (7, 8):
                for _ in range(L):
                    T["PAIR_EQ" if op == 7 else "PAIR_X"][int(text[p]) * 6 + seq[r]] += 1
                    T["POS_MATCH" if op == 7 else "POS_MISMATCH"][pos_bin(r)] += 1
                    p, r = p + 1, r + 1
                tot["matches" if op == 7 else "mismatches"] += L
                if op == 7:
                    T["EQ_RUN"][min(L, 256) - 1] += 1
            elif op == 1:
                letters = seq[r: r + L]
                a = letters[0]
                T["INS_LEN"][min(L, 64) - 1] += 1
                mixed = not 1 <= a <= 4
                for c in letters:
                    T["INS_LETTER"][c] += 1
                    T["POS_INS"][pos_bin(r)] += 1
                    mixed = mixed or c != a
                    r += 1
                T["HP_INS"][33 if mixed else min(32, run(p - 1, -1, a) + run(p, 1, a))] += 1
                tot["ins_events"] += 1
                tot["ins_bases"] += L
            elif op == 2:
                a = int(text[p])
                T["DEL_LEN"][min(L, 64) - 1] += 1
                T["POS_DEL"][pos_bin(min(r, n - 1))] += 1
                mixed = not 1 <= a <= 4
                for k in range(L):
                    T["DEL_LETTER"][int(text[p + k])] += 1
                    mixed = mixed or int(text[p + k]) != a
                T["HP_DEL"][33 if mixed else min(32, run(p - 1, -1, a) + L + run(p + L, 1, a))] += 1
                p += L
                tot["del_events"] += 1
                tot["del_bases"] += L
            elif op == 4:
                for _ in range(L):
                    T["POS_CLIP"][pos_bin(r)] += 1
                    r += 1
                tot["clip_bases"] += L
        T["IDENTITY"][tot["matches"] * 100 // (tot["matches"] + tot["mismatches"] + tot["ins_bases"] + tot["del_bases"])] += 1
        for i, k in enumerate(TOTALS):
            T["TOTALS"][i] += tot[k]
    return {k: np.array(v, dtype=np.uint64) for k, v in T.items()}


def tsv(T):
    """the text of a table as --error-profile writes it"""
    out = []

    def numbered(name, first, last=None, before_last=None):
        v = T[name]
        keys = [str(first + i) for i in range(len(v))]
        if last:
            keys[-1] = last
        if before_last:
            keys[-2] = before_last
        out.extend(f"{name}\t{k}\t{int(c)}" for k, c in zip(keys, v))
    for name in ("PAIR_EQ", "PAIR_X"):
        out.extend(f"{name}\t{LETTERS[a]}\t{LETTERS[b]}\t{int(T[name][a * 6 + b])}" for a in range(6) for b in range(6))
    numbered("INS_LEN", 1, "64+")
    numbered("DEL_LEN", 1, "64+")
    for name in ("INS_LETTER", "DEL_LETTER"):
        out.extend(f"{name}\t{LETTERS[a]}\t{int(T[name][a])}" for a in range(6))
    numbered("HP_DEL", 0, "mixed", "32+")
    numbered("HP_INS", 0, "mixed", "32+")
    for name in ("POS_MATCH", "POS_MISMATCH", "POS_INS", "POS_CLIP", "POS_DEL"):
        numbered(name, 0)
    numbered("EQ_RUN", 1, "256+")
    numbered("IDENTITY", 0)
    out.extend(f"TOTALS\t{k}\t{int(c)}" for k, c in zip(TOTALS, T["TOTALS"]))
    tot = {k: int(c) for k, c in zip(TOTALS, T["TOTALS"])}
    columns = tot["matches"] + tot["mismatches"] + tot["ins_bases"] + tot["del_bases"]

    def ppm(v):
        return v * 10 ** 6 // columns if columns else 0
    unequal = sum(int(T["PAIR_EQ"][a * 6 + b]) for a in range(6) for b in range(6) if a != b)
    out += [f"summary\tcolumns\t{columns}", f"summary\terror_rate_ppm\t{ppm(tot['mismatches'] + tot['ins_bases'] + tot['del_bases'])}",
            f"summary\tmismatch_ppm\t{ppm(tot['mismatches'])}", f"summary\tinsertion_ppm\t{ppm(tot['ins_bases'])}",
            f"summary\tdeletion_ppm\t{ppm(tot['del_bases'])}", f"summary\teq_columns_unequal\t{unequal}"]
    return ("\n".join(out) + "\n").encode()


# ---- inputs
def random_text(rng, lengths):
    """the concatenation of len(lengths) sequences: letters in runs of 1..40 (so that every homopolymer bin is met), with ranks 0 and 5 among
    them; a sequence often ends and the next begins with the same letter"""
    out = []
    for n in lengths:
        seq = []
        while len(seq) < n:
            a = int(rng.choice([0, 1, 2, 3, 4, 5], p=[0.02, 0.235, 0.235, 0.235, 0.235, 0.04]))
            seq += [a] * int(rng.choice([1, 1, 1, 2, 3, 5, 8, 31, 32, 33, 40]))
        out.append(np.array(seq[:n], dtype=np.uint8))
    for i in range(1, len(out)):
        if i % 2 and out[i - 1][-1] in (1, 2, 3, 4):
            out[i][: min(3, len(out[i]))] = out[i - 1][-1]
    return np.concatenate(out)


def random_records(rng, lengths, n, max_words=9, max_len=12):
    """n records of every flag and mapping quality, placed so that they fit their sequences (coverage_ref's, with longer words now and then)"""
    rows = []
    while len(rows) < n:
        ws = random_words(rng, int(rng.integers(1, max_words + 1)), max_len=max_len if rng.integers(0, 4) else 5 * max_len, clips=bool(rng.integers(0, 2)))
        ref = int(rng.integers(0, len(lengths)))
        if span(ws) > lengths[ref] or span(ws) == 0:
            continue
        flag = int(rng.choice([0, 16, 256, 272, 2048, 2064, 4]))
        rows.append((flag, ref, int(rng.integers(0, lengths[ref] - span(ws) + 1)), int(rng.choice([0, 3, 60])), ws))
    return records_of(rows)


def fitted_reads(rng, text, lengths, records, words, fraction=0.7):
    """one read per record of the record's query length; with probability `fraction` per = column the read's letter is the reference's (so that
    PAIR_EQ has a diagonal and inserted runs meet equal neighbours), otherwise random. The records' `read` is set."""
    starts = starts_of(lengths)
    reads = attach_reads(rng, records, words)
    for i, rec in enumerate(records):
        seq = oriented(reads[i], rec["flag"]).copy()
        p, r = int(starts[int(rec["ref"])]) + int(rec["pos"]), 0
        for wd in words[int(rec["coff"]): int(rec["coff"]) + int(rec["clen"])]:
            op, L = int(wd) & 15, int(wd) >> 4
            if op == 7:
                keep = rng.random(L) < fraction
                seq[r: r + L][keep] = text[p: p + L][keep]
            if op == 1 and rng.random() < 0.6 and p < len(text):
                seq[r: r + L] = text[p] if rng.random() < 0.5 or p == 0 else text[p - 1]
            if op in (7, 8, 2):
                p += L
            if op in (7, 8, 1, 4):
                r += L
        reads[i] = oriented(seq, rec["flag"])                             # (orienting twice gives the read as given)
    return reads
