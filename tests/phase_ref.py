"""The phasing rule (flx_phase, include/floxer_amd.h) in plain numpy and Python, for the tests. Two forms that check each other: `phase`
finds the word of every anchor by a search over the words' first columns and runs links, chain, tags and votes over arrays; `phase_naive`
expands every record into its columns, each with the insertions and deletions directly behind it, and follows the rule's text site by
site and record by record. Next to them what the tool floxer_phase makes of a VCF: `vcf_sites`, `vcf_lines` and `tag_lines`.

sites: a structured array of floxer_amd.PHASE_SITE_DTYPE; records, words, lengths, reads: as in pileup_ref. The results are
(results, tags): structured arrays of floxer_amd.PHASE_RESULT_DTYPE and PHASE_TAG_DTYPE, the tags in the order of the counted records."""
import numpy as np

import floxer_amd as F
import pileup_ref as P
from pileup_ref import records_of, records_with_reads, span, starts_of, word  # noqa: F401 (shared with the tests)

SNV, DEL, INS = 0, 1, 2
REF, ALT, NONE = 0, 1, 2
NO_SET = (1 << 32) - 1
DEFAULTS = dict(min_link=2, min_margin=1, refine_rounds=1)


def options(count_secondary=False, min_mapq=0, min_link=0, min_margin=0, refine_rounds=0, skip_refine=False):
    return dict(count_secondary=count_secondary, min_mapq=min_mapq, min_link=min_link, min_margin=min_margin, refine_rounds=refine_rounds, skip_refine=skip_refine)


def c_options(o):
    return F.phase_options(**o)


def model(o):
    """(min_link, min_margin, rounds) with the defaults taken for 0"""
    return int(o["min_link"]) or 2, int(o["min_margin"]) or 1, 0 if o["skip_refine"] else int(o["refine_rounds"]) or 1


def pack(letters):
    lo = 0
    for k, r in enumerate(letters):
        lo |= (int(r) - 1) << (62 - 2 * k)
    return lo


def unpack(lo, length):
    return tuple(((int(lo) >> (62 - 2 * k)) & 3) + 1 for k in range(int(length)))


def sites_of(rows):
    """rows: (ref, pos, kind, alt_rank, length, letters as ranks) -> PHASE_SITE_DTYPE"""
    out = np.zeros(len(rows), dtype=F.PHASE_SITE_DTYPE)
    for i, (ref, pos, kind, alt, length, letters) in enumerate(rows):
        out[i] = (ref, pos, kind, alt, length, 0, pack(letters))
    return out


def anchors_of(lengths, sites):
    return starts_of(lengths)[sites["ref"].astype(np.int64)] + sites["pos"].astype(np.int64)


def counted(records, o):
    return [rec for rec in records if P.record_counts(rec, o)]


def words_of(rec, words):
    return [(int(w) & 15, int(w) >> 4) for w in words[int(rec["coff"]): int(rec["coff"]) + int(rec["clen"])]]


# ------------------------------------------------------------------------------------------------ the observations, by words
def word_key(op, anchor, ln, seq, row):
    """(anchor, kind, length, letters) of an I or D word behind a column, or None when it is no allele"""
    if op == 2:
        return (anchor, DEL, ln, ())
    letters = tuple(int(x) for x in seq[row: row + ln]) if ln <= 32 else ()
    if ln > 32 or any(not 1 <= x <= 4 for x in letters):
        return None
    return (anchor, INS, ln, letters)


def observe(lengths, sites, rec, words, reads):
    """(first, obs): the record's first site and one observation per slot"""
    starts = starts_of(lengths)
    anchors = anchors_of(lengths, sites)
    ws = words_of(rec, words)
    op = np.array([w[0] for w in ws])
    ln = np.array([w[1] for w in ws])
    cols = np.where(np.isin(op, (7, 8, 2)), ln, 0)
    rows = np.where(np.isin(op, (7, 8, 1, 4)), ln, 0)
    origin = int(starts[int(rec["ref"])]) + int(rec["pos"])
    col0 = origin + np.cumsum(cols) - cols
    row0 = np.cumsum(rows) - rows
    end = origin + int(cols.sum())
    first, last = int(np.searchsorted(anchors, origin, side="left")), int(np.searchsorted(anchors, end, side="left"))
    seq = P.oriented(reads[int(rec["read"])], rec["flag"])
    owners = np.nonzero(cols)[0]
    obs = np.full(last - first, NONE, dtype=np.uint8)
    for k in range(last - first):
        s = sites[first + k]
        a = int(anchors[first + k])
        t = int(owners[np.searchsorted(col0[owners], a, side="right") - 1])
        if int(s["kind"]) == SNV:
            if op[t] == 7:
                obs[k] = REF
            elif op[t] == 8 and int(seq[int(row0[t]) + a - int(col0[t])]) == int(s["alt_rank"]):
                obs[k] = ALT
            continue
        want = (a, int(s["kind"]), int(s["length"]), unpack(s["letters"], s["length"]) if int(s["kind"]) == INS else ())
        behind = []
        if a == int(col0[t]) + int(ln[t]) - 1:
            p, row = a + 1, int(row0[t]) + int(rows[t])
            for u in range(t + 1, len(ws)):
                if op[u] not in (1, 2):
                    break
                behind.append(word_key(int(op[u]), p - 1, int(ln[u]), seq, row))
                if op[u] == 1:
                    row += int(ln[u])
                else:
                    p += int(ln[u])
        if want in behind:
            obs[k] = ALT
        elif not behind and op[t] in (7, 8) and a + 1 < end:
            obs[k] = REF
    return first, obs


def phase(lengths, sites, records, words, reads, o, add_of=None):
    """the whole rule -> (results, tags); add_of: the add serial of every counted record (default 0)"""
    min_link, min_margin, rounds = model(o)
    n = len(sites)
    recs = counted(records, o)
    seen = [observe(lengths, sites, rec, words, reads) for rec in recs]
    cis, trans = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for first, obs in seen:
        if len(obs) < 2:
            continue
        both = (obs[:-1] < NONE) & (obs[1:] < NONE)
        at = first + np.nonzero(both)[0]
        equal = obs[:-1][both] == obs[1:][both]
        np.add.at(cis, at[equal], 1)
        np.add.at(trans, at[~equal], 1)
    joined = np.zeros(n, dtype=bool)                                     # joined[i]: site i is connected to site i - 1
    if n > 1:
        joined[1:] = (sites["ref"][1:] == sites["ref"][:-1]) & (np.abs(cis[:-1] - trans[:-1]) >= min_link)
    flips = np.zeros(n, dtype=np.int64)
    if n > 1:
        flips[1:] = joined[1:] & (trans[:-1] > cis[:-1])
    at = np.arange(n)
    set_id = np.maximum.accumulate(np.where(joined, 0, at)) if n else at
    F_ = np.cumsum(flips)
    p = (F_ - F_[set_id]) & 1 if n else flips
    size = np.bincount(set_id, minlength=n)[set_id] if n else at
    phased = size > 1
    tags = np.zeros(len(recs), dtype=F.PHASE_TAG_DTYPE)
    keep, swap = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)

    def tag_all():
        for j, (first, obs) in enumerate(seen):
            idx = first + np.arange(len(obs))
            use = phased[idx] & (obs < NONE)
            hap, ps, h1, h2 = 0, NO_SET, 0, 0
            if use.any():
                ids, counts = np.unique(set_id[idx][use], return_counts=True)
                ps = int(ids[np.argmax(counts)])                           # (the first of the largest: the smallest set id, the record's first run)
                mine = use & (set_id[idx] == ps)
                x = obs[mine].astype(np.int64) ^ p[idx][mine]
                h1, h2 = int((x == 1).sum()), int((x == 0).sum())
                hap = 1 if h1 - h2 >= min_margin else 2 if h2 - h1 >= min_margin else 0
            tags[j] = (0 if add_of is None else int(add_of[j]), int(recs[j]["read"]), hap, ps, h1, h2, len(obs), 0)

    tag_all()
    for _ in range(rounds):
        keep[:], swap[:] = 0, 0
        for j, (first, obs) in enumerate(seen):
            if int(tags[j]["hap"]) == 0:
                continue
            idx = first + np.arange(len(obs))
            mine = phased[idx] & (obs < NONE) & (set_id[idx] == int(tags[j]["phase_set"]))
            agrees = (obs[mine].astype(np.int64) ^ p[idx][mine]) == (1 if int(tags[j]["hap"]) == 1 else 0)
            np.add.at(keep, idx[mine][agrees], 1)
            np.add.at(swap, idx[mine][~agrees], 1)
        p = np.where(swap > keep, p ^ 1, p)
        tag_all()
    out = np.zeros(n, dtype=F.PHASE_RESULT_DTYPE)
    out["phase_set"], out["phased"], out["phase"], out["cis"], out["trans"], out["keep"], out["swap"] = set_id, phased, p, cis, trans, keep, swap
    return out, tags


# ------------------------------------------------------------------------------------------------ the naive form
def columns_of(origin, ws, seq):
    """every reference-consuming column of a record: [position, op, oriented letter or None, the I and D events directly behind it]"""
    out, open_runs = [], []
    p, row = origin, 0
    for op, ln in ws:
        if op in (1, 2):
            key = word_key(op, p - 1, ln, seq, row) if p > origin else None
            for c in open_runs:
                c[3].append(key)
        else:
            open_runs = []
        if op in (7, 8, 2):
            for k in range(ln):
                out.append([p + k, op, int(seq[row + k]) if op != 2 else None, []])
            open_runs.append(out[-1])
            p += ln
        if op in (7, 8, 1, 4):
            row += ln
    return out


def phase_naive(lengths, sites, records, words, reads, o, add_of=None):
    min_link, min_margin, rounds = model(o)
    starts = starts_of(lengths)
    n = len(sites)
    anchor = [int(starts[int(s["ref"])]) + int(s["pos"]) for s in sites]
    recs = counted(records, o)
    seen = []                                                            # per record: {site index: observation}
    for rec in recs:
        origin = int(starts[int(rec["ref"])]) + int(rec["pos"])
        cols = columns_of(origin, words_of(rec, words), P.oriented(reads[int(rec["read"])], rec["flag"]))
        end = origin + len(cols)
        mine = {}
        for i in range(n):
            if not origin <= anchor[i] < end:
                continue
            _, op, letter, behind = cols[anchor[i] - origin]
            s = sites[i]
            if int(s["kind"]) == SNV:
                mine[i] = REF if op == 7 else ALT if op == 8 and letter == int(s["alt_rank"]) else NONE
            else:
                want = (anchor[i], int(s["kind"]), int(s["length"]), unpack(s["letters"], s["length"]) if int(s["kind"]) == INS else ())
                mine[i] = ALT if want in behind else REF if not behind and op in (7, 8) and anchor[i] + 1 < end else NONE
        seen.append(mine)
    cis, trans = [0] * n, [0] * n
    for mine in seen:
        for i in mine:
            if i + 1 in mine and mine[i] != NONE and mine[i + 1] != NONE:
                if mine[i] == mine[i + 1]:
                    cis[i] += 1
                else:
                    trans[i] += 1
    set_id, p = list(range(n)), [0] * n
    for i in range(1, n):
        if int(sites[i]["ref"]) == int(sites[i - 1]["ref"]) and abs(cis[i - 1] - trans[i - 1]) >= min_link:
            set_id[i] = set_id[i - 1]
            p[i] = p[i - 1] ^ (1 if trans[i - 1] > cis[i - 1] else 0)
    phased = [set_id.count(set_id[i]) > 1 for i in range(n)] if n < 3000 else None
    if phased is None:
        size = {}
        for s in set_id:
            size[s] = size.get(s, 0) + 1
        phased = [size[set_id[i]] > 1 for i in range(n)]
    tags = np.zeros(len(recs), dtype=F.PHASE_TAG_DTYPE)
    keep, swap = [0] * n, [0] * n

    def tag_all():
        for j, mine in enumerate(seen):
            runs = {}                                                    # set id -> [observations, h1, h2], in the record's order
            for i in sorted(mine):
                if phased[i] and mine[i] != NONE:
                    r = runs.setdefault(set_id[i], [0, 0, 0])
                    r[0] += 1
                    r[1 if mine[i] ^ p[i] == 1 else 2] += 1
            hap, ps, h1, h2 = 0, NO_SET, 0, 0
            for sid in sorted(runs):
                if runs[sid][0] > (runs[ps][0] if ps != NO_SET else 0):
                    ps = sid
            if ps != NO_SET:
                _, h1, h2 = runs[ps]
                hap = 1 if h1 - h2 >= min_margin else 2 if h2 - h1 >= min_margin else 0
            tags[j] = (0 if add_of is None else int(add_of[j]), int(recs[j]["read"]), hap, ps, h1, h2, len(mine), 0)

    tag_all()
    for _ in range(rounds):
        keep, swap = [0] * n, [0] * n
        for j, mine in enumerate(seen):
            hap, ps = int(tags[j]["hap"]), int(tags[j]["phase_set"])
            for i in mine:
                if hap and phased[i] and set_id[i] == ps and mine[i] != NONE:
                    if (mine[i] ^ p[i]) == (1 if hap == 1 else 0):
                        keep[i] += 1
                    else:
                        swap[i] += 1
        p = [p[i] ^ 1 if swap[i] > keep[i] else p[i] for i in range(n)]
        tag_all()
    out = np.zeros(n, dtype=F.PHASE_RESULT_DTYPE)
    for i in range(n):
        out[i] = (set_id[i], phased[i], p[i], cis[i], trans[i], keep[i], swap[i], 0)
    return out, tags


# ------------------------------------------------------------------------------------------------ the tool's files
PS_HEADER = '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set">\n'


def vcf_sites(lines, names):
    """the lines of a VCF that are sites -> (line indices, sites): biallelic, plain A C G T, an SNV or an anchored indel with an insertion
    of at most 32 letters, GT 0/1 or 1/0 in the first sample"""
    at, rows = [], []
    for i, line in enumerate(lines):
        col = line.rstrip("\r\n").split("\t")
        if line.startswith("#") or len(col) < 10:
            continue
        ref, alt = col[3], col[4]
        if not ref or not alt or set(ref + alt) - set("ACGT"):
            continue
        fmt, sample = col[8].split(":"), col[9].split(":")
        if "GT" not in fmt or fmt.index("GT") >= len(sample) or sample[fmt.index("GT")] not in ("0/1", "1/0"):
            continue
        rank = lambda c: "ACGT".index(c) + 1                              # noqa: E731
        if len(ref) == 1 and len(alt) == 1 and ref != alt:
            row = (SNV, rank(alt), 1, ())
        elif len(ref) == 1 and 1 < len(alt) <= 33 and alt[0] == ref:
            row = (INS, 0, len(alt) - 1, [rank(c) for c in alt[1:]])
        elif len(alt) == 1 and len(ref) > 1 and ref[0] == alt:
            row = (DEL, 0, len(ref) - 1, ())
        else:
            continue
        at.append(i)
        rows.append((names.index(col[0]), int(col[1]) - 1) + row)
    return at, sites_of(rows)


def vcf_lines(lines, names, results):
    """the tool's output for the input lines and the results of their sites"""
    at, sites = vcf_sites(lines, names)
    assert len(results) == len(at)
    out = []
    for i, line in enumerate(lines):
        if line.startswith("#CHROM") and not any(l.startswith("##FORMAT=<ID=PS,") for l in lines):
            out.append(PS_HEADER)
        if i not in at:
            out.append(line)
            continue
        r = results[at.index(i)]
        body = line.rstrip("\r\n")
        col = body.split("\t")
        fmt = col[8].split(":")
        if "PS" not in fmt:
            fmt.append("PS")
        ps, gt = fmt.index("PS"), fmt.index("GT")
        col[8] = ":".join(fmt)
        for c in range(9, len(col)):
            v = col[c].split(":")
            v += ["."] * (ps + 1 - len(v))
            v[ps] = str(int(sites[int(r["phase_set"])]["pos"]) + 1) if c == 9 and int(r["phased"]) else "."
            if c == 9 and int(r["phased"]):
                v[gt] = "0|1" if int(r["phase"]) else "1|0"
            col[c] = ":".join(v)
        out.append("\t".join(col) + line[len(body):])
    return out


def tag_lines(names, tags, batch_reads, sites):
    """the tool's --haplotags table: one line per read in input order; tags[k]: add = the batch, read = the index in it"""
    first = {}
    for t in tags:
        first.setdefault(int(t["add"]) * batch_reads + int(t["read"]), t)
    out = []
    for r, name in enumerate(names):
        t = first.get(r)
        if t is None:
            out.append(f"{name}\t.\t.\t0\t0\t0\n")
            continue
        ps = "." if int(t["phase_set"]) == NO_SET else str(int(sites[int(t["phase_set"])]["pos"]) + 1)
        out.append(f"{name}\t{int(t['hap']) or '.'}\t{ps}\t{int(t['h1'])}\t{int(t['h2'])}\t{int(t['n_slots'])}\n")
    return out
