"""The coordinate order of records in plain numpy, for the tests of flx_sort: the key and its order (np.lexsort on hi, lo), a record's
end, reg2bin / reg2bins of SAMv1 5.3, and readers of BGZF, BAM and BAI on zlib and struct. Nothing here calls the library."""
import struct
import zlib

import numpy as np

REC_DTYPE = np.dtype([("read", "<u8"), ("flag", "<u4"), ("ref", "<i4"), ("pos", "<i4"), ("nm", "<u4"), ("coff", "<u8"), ("clen", "<u4"), ("res", "<u4")])
ENTRY_DTYPE = np.dtype([("ordinal", "<u8"), ("ref", "<i4"), ("pos", "<i4"), ("end", "<u4"), ("flag", "<u4")])
OPS = {"I": 1, "D": 2, "S": 4, "=": 7, "X": 8}
CONSUMES = (2, 7, 8)
UNPLACED = 0xFFFFFFFF


def word(op, n):
    return (int(n) << 4) | OPS[op]


def records_of(rows):
    """rows: (flag, ref, pos, [words]) -> the record array and the word pool (every record's words stored once, in row order)"""
    rec = np.zeros(len(rows), dtype=REC_DTYPE)
    pool = []
    for i, (flag, ref, pos, words) in enumerate(rows):
        rec[i] = (i, flag, ref, pos, 0, len(pool), len(words), 0)
        pool.extend(words)
    return rec, np.array(pool, dtype=np.uint32)


def unplaced(rec):
    return ((rec["flag"] & 4) != 0) | (rec["ref"] < 0)


def spans(rec, words):
    """the reference columns of every record's words"""
    words = np.asarray(words, dtype=np.uint64)
    cols = np.where(np.isin(words & 15, CONSUMES), words >> 4, 0).astype(np.uint64)
    cum = np.concatenate([[0], np.cumsum(cols, dtype=np.uint64)])
    a = rec["coff"].astype(np.int64)
    return (cum[a + rec["clen"].astype(np.int64)] - cum[a]).astype(np.uint64)


def ends(rec, words):
    """position + max(1, span) for a mapped record; position + 1 for an unplaced one (as uint32)"""
    un = unplaced(rec)
    pos = rec["pos"].astype(np.int64) & 0xFFFFFFFF
    e = np.where(un, pos + 1, pos + np.maximum(1, spans(rec, words).astype(np.int64)))
    return (e & 0xFFFFFFFF).astype(np.uint32)


def keys(rec, ordinals):
    un = unplaced(rec)
    ref = np.where(un, UNPLACED, rec["ref"].astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    hi = (ref << np.uint64(32)) | (rec["pos"].astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    lo = (((rec["flag"].astype(np.uint64) >> np.uint64(4)) & np.uint64(1)) << np.uint64(63)) | np.asarray(ordinals, dtype=np.uint64)
    return hi, lo


def order(rec, ordinals):
    """the records' indices in key order"""
    hi, lo = keys(rec, ordinals)
    return np.lexsort((lo, hi))


def entries(rec, words, ordinals):
    """what flx_sort_host and a finished object give: the entries in key order"""
    o = order(rec, ordinals)
    out = np.zeros(len(rec), dtype=ENTRY_DTYPE)
    out["ordinal"] = np.asarray(ordinals, dtype=np.uint64)[o]
    out["ref"] = np.where(unplaced(rec), -1, rec["ref"])[o]
    out["pos"] = rec["pos"][o]
    out["end"] = ends(rec, words)[o]
    out["flag"] = rec["flag"][o]
    return out


def random_records(rng, n, n_refs=3, max_pos=1000, max_words=4, unplaced_share=0.1):
    rows = []
    for _ in range(n):
        ops = "=XIDS"
        words = [word(ops[int(rng.integers(0, 5))], int(rng.integers(1, 30))) for _ in range(int(rng.integers(0, max_words + 1)))]
        if rng.random() < unplaced_share:
            rows.append((4, -1, 0, []))
        else:
            rows.append((int(rng.choice([0, 16, 256, 272, 2048, 2064])), int(rng.integers(0, n_refs)), int(rng.integers(0, max_pos)), words))
    return records_of(rows)


# ------------------------------------------------------------------------------------------------ bins (SAMv1 5.3)
def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


# ------------------------------------------------------------------------------------------------ BGZF, BAM, BAI
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_members(data):
    """[(file offset, compressed size, payload)] of every BGZF member; every member is checked as a gzip member of its own"""
    out = []
    at = 0
    while at < len(data):
        assert data[at: at + 4] == b"\x1f\x8b\x08\x04", at
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        extra = data[at + 12: at + 12 + xlen]
        bsize = None
        e = 0
        while e < len(extra):
            si1, si2, slen = extra[e], extra[e + 1], struct.unpack_from("<H", extra, e + 2)[0]
            if (si1, si2) == (66, 67):
                bsize = struct.unpack_from("<H", extra, e + 4)[0] + 1
            e += 4 + slen
        assert bsize is not None, at
        member = data[at: at + bsize]
        d = zlib.decompressobj(31)                     # gzip framing: header, crc32 and isize are checked
        payload = d.decompress(member) + d.flush()
        assert d.eof and d.unused_data == b"", at
        out.append((at, bsize, payload))
        at += bsize
    return out


class Bam:
    """A BAM file read whole: header text, references, and every record with its bytes, fields and virtual offsets."""

    def __init__(self, path):
        with open(path, "rb") as f:
            self.data = f.read()
        self.members = bgzf_members(self.data)
        self.has_eof = len(self.members) > 0 and self.data.endswith(EOF_BLOCK)
        stream = b"".join(m[2] for m in self.members)
        self.stream = stream
        self._mstarts = np.cumsum([0] + [len(m[2]) for m in self.members])[:-1]
        self._coffs = [m[0] for m in self.members]
        assert stream[:4] == b"BAM\x01"
        l_text = struct.unpack_from("<i", stream, 4)[0]
        self.text = stream[8: 8 + l_text].decode()
        at = 8 + l_text
        n_ref = struct.unpack_from("<i", stream, at)[0]
        at += 4
        self.refs = []
        for _ in range(n_ref):
            l_name = struct.unpack_from("<i", stream, at)[0]
            name = stream[at + 4: at + 4 + l_name - 1].decode()
            self.refs.append((name, struct.unpack_from("<i", stream, at + 4 + l_name)[0]))
            at += 8 + l_name
        self.records = []                              # dicts: bytes, ref, pos, end, bin, flag, name, vstart, vend
        while at < len(stream):
            size = struct.unpack_from("<i", stream, at)[0]
            body = stream[at + 4: at + 4 + size]
            ref, pos, l_name, mapq, bin_, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", body, 0)
            name = body[32: 32 + l_name - 1].decode()
            cig = struct.unpack_from("<%dI" % n_cigar, body, 32 + l_name)
            span = sum(c >> 4 for c in cig if (c & 15) in (0, 2, 3, 7, 8))
            un = ref < 0 or (flag & 4) != 0
            self.records.append(dict(bytes=stream[at: at + 4 + size], ref=ref, pos=pos, end=pos + (1 if un else max(1, span)), bin=bin_, flag=flag, name=name,
                                     mapq=mapq, vstart=self.voffset(at), vend=self.voffset(at + 4 + size)))
            at += 4 + size
        assert at == len(stream)

    def voffset(self, u):
        """the virtual offset of uncompressed offset u: a byte at a member's end is the next member's first"""
        m = int(np.searchsorted(self._mstarts, u, side="right")) - 1
        return (self._coffs[m] << 16) | (u - int(self._mstarts[m]))


class Bai:
    def __init__(self, path):
        with open(path, "rb") as f:
            d = f.read()
        assert d[:4] == b"BAI\x01"
        n_ref = struct.unpack_from("<i", d, 4)[0]
        at = 8
        self.refs = []                                 # per reference: {"bins": {bin: [(beg, end)]}, "pseudo": (first, last, mapped, unmapped) | None, "linear": [..]}
        for _ in range(n_ref):
            n_bin = struct.unpack_from("<i", d, at)[0]
            at += 4
            bins, pseudo = {}, None
            for _ in range(n_bin):
                b, n_chunk = struct.unpack_from("<Ii", d, at)
                at += 8
                chunks = [struct.unpack_from("<QQ", d, at + 16 * c) for c in range(n_chunk)]
                at += 16 * n_chunk
                if b == 37450:
                    assert n_chunk == 2
                    pseudo = (chunks[0][0], chunks[0][1], chunks[1][0], chunks[1][1])
                else:
                    assert b not in bins
                    bins[b] = chunks
            n_intv = struct.unpack_from("<i", d, at)[0]
            at += 4
            linear = list(struct.unpack_from("<%dQ" % n_intv, d, at))
            at += 8 * n_intv
            self.refs.append(dict(bins=bins, pseudo=pseudo, linear=linear))
        self.n_no_coor = struct.unpack_from("<Q", d, at)[0] if at < len(d) else None
        at += 8
        assert at == len(d)

    def query(self, bam, ref, beg, end):
        """the records of [beg, end) of a reference, found through the bins, the chunks and the linear index's lower bound"""
        r = self.refs[ref]
        w = beg >> 14
        low = r["linear"][w] if w < len(r["linear"]) else (r["linear"][-1] if r["linear"] else 0)
        by_start = {rec["vstart"]: i for i, rec in enumerate(bam.records)}
        found = set()
        for b in reg2bins(beg, end):
            for cb, ce in r["bins"].get(b, []):
                if ce <= low:
                    continue
                i = by_start[cb]
                while i < len(bam.records) and bam.records[i]["vstart"] < ce:
                    rec = bam.records[i]
                    if rec["ref"] == ref and rec["pos"] < end and rec["end"] > beg:
                        found.add(i)
                    i += 1
        return found
