"""The PAF rule (flx_paf, include/floxer_amd.h) and the PAF line in plain Python, for the tests; written from the rule's text.

records: a numpy array of floxer_amd's record dtype (read, flag, ref, pos, nm, coff, clen, res); words: the uint32 CIGAR pool (len << 4 |
op; I=1 D=2 S=4 '='=7 X=8); read_lengths: one entry per read; ref_lens: the reference lengths. A summary is a tuple in the order of
floxer_amd.PAF_SUMMARY_DTYPE: query_start, query_end, ref_end, matches, mismatches, ins_bases, del_bases, gap_opens."""
import numpy as np

import floxer_amd as F

REC = F._REC_DTYPE
OPS = "MIDNSHP=X"
FLAGS = (0, 16, 256, 272, 2048, 2064, 4)
LIMIT = 1 << 31


class Refused(Exception):
    pass


def word(op, n):
    return (int(n) << 4) | OPS.index(op)


def records_of(rows):
    """rows: (flag, ref, pos, read, nm, [words], mapq=0) -> (records, word pool)"""
    rec = np.zeros(len(rows), dtype=REC)
    pool = []
    for i, row in enumerate(rows):
        flag, ref, pos, read, nm, ws = row[:6]
        rec[i] = (read, flag, ref, pos, nm, len(pool), len(ws), row[6] if len(row) > 6 else 0)
        pool.extend(int(w) for w in ws)
    return rec, np.array(pool, dtype=np.uint32)


def mapped(rec):
    return not int(rec["flag"]) & 4 and int(rec["ref"]) >= 0


def summary(rec, words, read_lengths, ref_lens, n_words=None):
    """one record's summary; Refused with the reason for a record the rule refuses"""
    if not mapped(rec):
        return (0,) * 8
    n_words = len(words) if n_words is None else n_words
    if int(rec["ref"]) >= len(ref_lens):
        raise Refused("reference_id")
    if int(rec["pos"]) < 0:
        raise Refused("negative position")
    if int(rec["clen"]) == 0:
        raise Refused("no words")
    if int(rec["coff"]) + int(rec["clen"]) > n_words:
        raise Refused("words outside the pool")
    ws = [(int(w) & 15, int(w) >> 4) for w in words[int(rec["coff"]): int(rec["coff"]) + int(rec["clen"])]]
    if any(op not in (7, 8, 1, 2, 4) for op, _ in ws):
        raise Refused("op")
    if any(ln == 0 for _, ln in ws):
        raise Refused("zero length")
    non_s = [i for i, (op, _) in enumerate(ws) if op != 4]
    if not non_s:
        raise Refused("no reference-consuming column")
    if any(op == 4 for op, _ in ws[non_s[0]: non_s[-1] + 1]):
        raise Refused("interior clip")
    lead = sum(ln for _, ln in ws[: non_s[0]])
    trail = sum(ln for _, ln in ws[non_s[-1] + 1:])
    eq, x, ins, dele = (sum(ln for op, ln in ws if op == o) for o in (7, 8, 1, 2))
    gap_opens = sum(1 for i, (op, _) in enumerate(ws) if op in (1, 2) and (i == 0 or ws[i - 1][0] != op))
    if max(lead, trail, eq, x, ins, dele, gap_opens, lead + eq + x + ins + trail, eq + x + dele) >= LIMIT:
        raise Refused("2^31")
    if int(rec["pos"]) + eq + x + dele > int(ref_lens[int(rec["ref"])]):
        raise Refused("behind its sequence")
    if int(rec["read"]) >= len(read_lengths):
        raise Refused("read_index")
    n = int(read_lengths[int(rec["read"])])
    if lead + eq + x + ins + trail != n:
        raise Refused("read length")
    if eq + x + dele == 0:
        raise Refused("no reference-consuming column")
    if int(rec["flag"]) & 16:
        q0, q1 = trail, n - lead
    else:
        q0, q1 = lead, n - trail
    return (q0, q1, int(rec["pos"]) + eq + x + dele, eq, x, ins, dele, gap_opens)


def summarize(records, words, read_lengths, ref_lens):
    out = np.zeros(len(records), dtype=F.PAF_SUMMARY_DTYPE)
    for i, rec in enumerate(records):
        out[i] = summary(rec, words, read_lengths, ref_lens)
    return out


def divergence(num, den):
    """de:f with four decimals, in integers"""
    t = (20000 * num + den) // (2 * den)
    return "%d.%04d" % (t // 10000, t % 10000)


def options(write_cigar=False, write_unmapped=False, mapq_from_records=False, skip_secondary=False):
    return dict(write_cigar=write_cigar, write_unmapped=write_unmapped, mapq_from_records=mapq_from_records, skip_secondary=skip_secondary)


def c_options(o):
    return F.paf_options(**o)


def line(qname, qlen, rec, ws, s, ref_ids, ref_lens, o, score=None, cs=None):
    """the line of one record (str, with its line end), or '' when the record produces none"""
    if not mapped(rec):
        return "\t".join([qname, str(qlen), "0", "0", "*", "*", "0", "0", "0", "0", "0", "0"]) + "\n" if o["write_unmapped"] else ""
    flag = int(rec["flag"])
    if flag & 256 and o["skip_secondary"]:
        return ""
    q0, q1, ref_end, eq, x, ins, dele, gap_opens = (int(v) for v in s)
    cols = [qname, str(qlen), str(q0), str(q1), "-" if flag & 16 else "+", ref_ids[int(rec["ref"])], str(int(ref_lens[int(rec["ref"])])), str(int(rec["pos"])),
            str(ref_end), str(eq), str(eq + x + ins + dele), str(int(rec["res"])) if o["mapq_from_records"] else "255"]
    cols.append("tp:A:S" if flag & 256 else "tp:A:P")
    cols.append("NM:i:%d" % int(rec["nm"]))
    if score is not None:
        cols.append("AS:i:%d" % int(score))
    cols.append("de:f:" + divergence(x + gap_opens, eq + x + gap_opens))
    if o["write_cigar"]:
        cols.append("cg:Z:" + "".join("%d%s" % (int(w) >> 4, OPS[int(w) & 15]) for w in ws))
    if cs:
        cols.append("cs:Z:" + (cs.decode() if isinstance(cs, bytes) else cs))
    return "\t".join(cols) + "\n"


def lines(read_ids, read_lengths, records, words, summaries, ref_ids, ref_lens, o, scores=None, cs=None):
    """the bytes of one write call; cs: a list of bytes / None per record"""
    out = []
    for i, rec in enumerate(records):
        ws = words[int(rec["coff"]): int(rec["coff"]) + int(rec["clen"])]
        out.append(line(read_ids[int(rec["read"])], int(read_lengths[int(rec["read"])]), rec, ws, summaries[i], ref_ids, ref_lens, o,
                        None if scores is None else scores[i], None if cs is None else cs[i]))
    return "".join(out).encode()


def random_valid(rng, ref_lens, n_reads, max_words=12, max_len=30):
    """n_reads reads with one record of every kind in turn, valid by construction: clips only at the ends, at least one reference column,
    the span inside the sequence, the read as long as its words say. Returns (records, words, read_lengths)."""
    rows, read_lengths = [], []
    for r in range(n_reads):
        flag = FLAGS[r % len(FLAGS)]
        if flag == 4:
            read_lengths.append(int(rng.integers(1, 200)))
            rows.append((4, -1, 0, r, 0, []))
            continue
        ref = int(rng.integers(0, len(ref_lens)))
        ws = []
        for _ in range(int(rng.integers(1, max_words + 1))):
            ws.append(("=XID"[int(rng.integers(0, 4))], int(rng.integers(1, max_len + 1))))
        if rng.integers(0, 2):                                           # (neighbours with one op are allowed: the rule takes any words)
            ws.insert(int(rng.integers(0, len(ws) + 1)), ("=", int(rng.integers(1, max_len + 1))))
        if not any(op in "=XD" for op, _ in ws):
            ws.append(("X", 1))
        span = sum(ln for op, ln in ws if op in "=XD")
        while span > ref_lens[ref]:                                      # drop reference columns until the record fits
            k = next(i for i, (op, _) in enumerate(ws) if op in "=XD")
            span -= ws[k][1]
            del ws[k]
        if span == 0:
            ws.append(("=", 1))
            span = 1
        if rng.integers(0, 2):
            ws.insert(0, ("S", int(rng.integers(1, 40))))
        if rng.integers(0, 2):
            ws.append(("S", int(rng.integers(1, 40))))
        pos = int(rng.integers(0, ref_lens[ref] - span + 1))
        read_lengths.append(sum(ln for op, ln in ws if op in "=XIS"))
        nm = sum(ln for op, ln in ws if op in "XID")
        rows.append((flag, ref, pos, r, nm, [word(op, ln) for op, ln in ws], int(rng.integers(0, 61))))
    rec, words = records_of(rows)
    return rec, words, np.array(read_lengths, dtype=np.uint64)


def from_sam(text, ref_ids, ref_lens, o):
    """the PAF bytes of a SAM text (header lines skipped), from QNAME, FLAG, RNAME, POS, MAPQ, CIGAR, the length of SEQ (a secondary
    record has none: its read's length is that of the same QNAME's record with SEQ), NM and cs alone"""
    fields = [l.split("\t") for l in text.splitlines() if l and not l.startswith("@")]
    qlen = {}
    for f in fields:
        if f[9] != "*":
            qlen[f[0]] = len(f[9])
    out = []
    for f in fields:
        flag = int(f[1])
        tags = {t[:2]: t[5:] for t in f[11:]}
        if flag & 4:
            rec, ws = np.zeros(1, dtype=REC)[0], []
            rec["flag"], rec["ref"] = 4, -1
            out.append(line(f[0], qlen[f[0]], rec, ws, (0,) * 8, ref_ids, ref_lens, o))
            continue
        ws, num = [], ""
        for ch in f[5]:
            if ch.isdigit():
                num += ch
            else:
                ws.append(word(ch, int(num)))
                num = ""
        rec, words = records_of([(flag, ref_ids.index(f[2]), int(f[3]) - 1, 0, int(tags["NM"]), ws, int(f[4]))])
        s = summary(rec[0], words, [qlen[f[0]]], ref_lens)
        out.append(line(f[0], qlen[f[0]], rec[0], ws, s, ref_ids, ref_lens, o, int(tags["AS"]) if "AS" in tags else None, tags.get("cs")))
    return "".join(out).encode()
