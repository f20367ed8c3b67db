"""Output options without a GPU: flx_select_records (the rule the pipeline applies to every read's records) against a plain-Python
restatement of it on random record sets, and the CLI's new flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC_DTYPE = np.dtype([("read", "<u8"), ("flag", "<u4"), ("ref", "<i4"), ("pos", "<i4"), ("nm", "<u4"), ("coff", "<u8"),
                      ("clen", "<u4"), ("res", "<u4")])


def restate(rows, drop_duplicates, max_alignments):
    """the rule of flx_output_options in plain Python. rows: [(read, flag, ref, pos, nm, cigar words tuple)] of whole reads, each
    read's records contiguous and in output order. Returns the keep mask."""
    keep = [True] * len(rows)
    i = 0
    while i < len(rows):
        j = i
        while j < len(rows) and rows[j][0] == rows[i][0]:
            j += 1
        mapped = [t for t in range(i, j) if not rows[t][1] & 4]
        if drop_duplicates:
            seen = set()
            for t in mapped:
                _, flag, ref, pos, nm, cig = rows[t]
                key = (ref, flag & 16, pos, nm, tuple(cig))
                if key in seen:
                    keep[t] = False
                seen.add(key)
        if max_alignments:
            left = sorted((t for t in mapped if keep[t]), key=lambda t: (rows[t][4], t))
            for t in left[max_alignments:]:
                keep[t] = False
        i = j
    return keep


def to_run(rows, rng, shuffle_pool=True):
    """RunResult of rows; every record's CIGAR gets words of its own at a random place in the pool (equal CIGARs at different
    offsets), except that some records reuse the previous record's words (one offset, as union members do)"""
    pieces, offs = [], []
    at = 0
    prev = None
    for r in rows:
        cig = list(r[5])
        if prev is not None and prev[0] == cig and cig and rng.random() < 0.3:
            offs.append(prev[1])
            continue
        if shuffle_pool and rng.random() < 0.5:
            pad = [int(x) for x in rng.integers(0, 1 << 20, size=int(rng.integers(1, 4)))]
            pieces += pad
            at += len(pad)
        offs.append(at if cig else int(rng.integers(0, 4)) * int(rng.random() < 0.5))
        pieces += cig
        prev = (cig, at)
        at += len(cig)
    raw = np.zeros(len(rows), dtype=REC_DTYPE)
    for k, r in enumerate(rows):
        raw[k] = (r[0], r[1], r[2], r[3], r[4], offs[k], len(r[5]), 0)
    return F.RunResult(raw, np.array(pieces, dtype=np.uint32), np.zeros(0, np.uint8))


def random_read(rng, read, n_refs, with_cigar=True):
    """a read's records as the pipeline forms them: alignments by reference id, the first of the best NM the primary"""
    if rng.random() < 0.12:
        return [(read, 4, -1, 0, 0, ())]
    base = []
    for _ in range(int(rng.integers(1, 8))):
        cig = tuple(int(rng.integers(1, 40)) << 4 | int(rng.choice([1, 2, 7, 8])) for _ in range(int(rng.integers(1, 6)))) if with_cigar else ()
        base.append([int(rng.integers(0, n_refs)), int(rng.integers(0, 2)) * 16, int(rng.integers(0, 5000)), int(rng.integers(0, 6)), cig])
    als = []
    for _ in range(int(rng.integers(1, 30))):
        a = list(base[int(rng.integers(0, len(base)))])
        kind = rng.integers(0, 8)
        if kind == 0:
            a[1] ^= 16                                   # strand only
        elif kind == 1:
            a[2] += int(rng.choice([-1, 1]))             # start only
        elif kind == 2:
            a[3] += 1                                    # NM only
        elif kind == 3 and a[4]:
            c = list(a[4])                               # one CIGAR word only
            p = int(rng.integers(0, len(c)))
            c[p] += 16
            a[4] = tuple(c)
        elif kind == 4:
            a[0] = (a[0] + 1) % n_refs                   # reference only (NM ties across references)
        als.append(a)                                    # else: an exact copy
    als.sort(key=lambda a: a[0])                         # per reference, stable: verification order within one
    best = min(a[3] for a in als)
    out, primary = [], False
    for ref, strand, pos, nm, cig in als:
        flag = strand
        if not primary and nm == best:
            primary = True
        else:
            flag |= 256
        out.append((read, flag, ref, pos, nm, cig))
    return out


def random_rows(rng, n_reads, n_refs=3, with_cigar=True):
    rows = []
    for read in range(n_reads):
        rows += random_read(rng, read, n_refs, with_cigar)
    return rows


@pytest.mark.parametrize("drop,cap", [(True, 0), (False, 1), (False, 2), (False, 3), (True, 1), (True, 2), (True, 5), (True, 1000),
                                      (False, 1000), (False, 0)])
@pytest.mark.parametrize("with_cigar", [True, False])
def test_select_records_matches_the_restatement(drop, cap, with_cigar):
    rng = np.random.default_rng(1000 * cap + 10 * drop + with_cigar)
    for trial in range(6):
        rows = random_rows(rng, 60, n_refs=1 + trial % 3, with_cigar=with_cigar)
        run = to_run(rows, rng)
        assert [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), tuple(int(w) for w in run.cigars[r[5]: r[5] + r[6]]))
                for r in run.rows] == rows                                                # the run holds the rows
        got = F.select_records(run, F.output_options(drop_duplicates=drop, max_alignments=cap))
        exp = restate(rows, drop, cap)
        assert got.tolist() == exp
        # every read keeps its primary (or its unmapped record), and keeps no more than the cap
        reads = sorted({r[0] for r in rows})
        for read in reads:
            idx = [k for k, r in enumerate(rows) if r[0] == read]
            lead = [k for k in idx if not rows[k][1] & 256]
            assert len(lead) == 1 and got[lead[0]]
            if cap:
                assert sum(got[k] for k in idx) <= cap
        if drop:
            kept = [(r[0], r[1] & 16, r[2], r[3], r[4], r[5]) for r, k in zip(rows, got) if k and not r[1] & 4]
            assert len(kept) == len(set(kept))


def test_select_records_edge_cases():
    rng = np.random.default_rng(5)
    # one read, equal CIGAR contents at different offsets, and a record that differs in each key field by itself
    c = (10 << 4 | 7, 2 << 4 | 8, 30 << 4 | 7)
    rows = [(0, 0, 0, 100, 2, c), (0, 256, 0, 100, 2, c), (0, 256 | 16, 0, 100, 2, c), (0, 256, 0, 101, 2, c), (0, 256, 0, 100, 3, c),
            (0, 256, 0, 100, 2, c[:2] + (31 << 4 | 7,)), (0, 256, 1, 100, 2, c), (0, 256, 1, 100, 2, c)]
    run = to_run(rows, rng)
    assert F.select_records(run, F.output_options(drop_duplicates=True)).tolist() == [True, False, True, True, True, True, True, False]
    # the cap keeps the smallest (NM, index): NM ties across references go by output order
    assert F.select_records(run, F.output_options(max_alignments=2)).tolist() == [True, True, False, False, False, False, False, False]
    assert F.select_records(run, F.output_options(drop_duplicates=True, max_alignments=3)).tolist() == \
        [True, False, True, True, False, False, False, False]
    # a read with only its unmapped record, empty CIGARs, N = 1 and N larger than the count
    rows = [(0, 4, -1, 0, 0, ()), (1, 0, 0, 7, 0, ()), (1, 256 | 16, 2, 7, 1, ()), (1, 256 | 16, 2, 7, 1, ()), (2, 4, -1, 0, 0, ())]
    run = to_run(rows, rng)
    for drop, cap in [(True, 0), (False, 1), (True, 1), (False, 9), (True, 9)]:
        assert F.select_records(run, F.output_options(drop, cap)).tolist() == restate(rows, drop, cap), (drop, cap)
    assert F.select_records(run, F.output_options(True, 1)).tolist() == [True, True, False, False, True]
    # no options and a zeroed struct keep everything; an empty array is fine
    L = capi.lib()
    keep = np.zeros(len(run.raw), np.uint8)
    raw = np.ascontiguousarray(run.raw)
    capi.check(L.flx_select_records(raw.ctypes.data_as(C.POINTER(capi.Record)), len(raw), capi.ptr(run.cigars, capi.u32p), None,
                                    capi.ptr(keep, capi.u8p)))
    assert keep.tolist() == [1] * len(raw)
    assert F.select_records(run, F.output_options()).tolist() == [True] * len(raw)
    assert F.select_records(to_run([], rng), F.output_options(True, 1)).tolist() == []


def test_output_options_reserved_fields_and_bad_values():
    rng = np.random.default_rng(6)
    run = to_run([(0, 0, 0, 1, 0, (5 << 4 | 7,))], rng)
    o = F.output_options(True, 1)
    o.reserved2[1] = 1
    with pytest.raises(F.FloxerError):
        F.select_records(run, o)
    with pytest.raises(F.FloxerError):
        F.output_options(max_alignments=-1)


def test_cli_accepts_the_output_flags_and_rejects_bad_caps(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    base = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"),
            "--output", str(tmp_path / "o.sam"), "-e", "2"]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert h.returncode == 0 and b"--drop-duplicate-alignments" in h.stderr and b"--max-alignments <value>" in h.stderr
    env = dict(os.environ, FLX_CLI_PARSE_ONLY="1")          # the options are parsed, then only the reader runs (no GPU)
    for extra in (["--drop-duplicate-alignments"], ["-D"], ["--max-alignments", "3"], ["-N", "1"], ["--max-alignments=2"],
                  ["-D", "-N", "5"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and r.stdout == b"" and b"CLI PARSER ERROR" not in r.stderr, (extra, r.stderr)
    for extra in (["--max-alignments", "0"], ["--max-alignments", "x"], ["-N", "-1"], ["-N"], ["--max-alignments", "3k"]):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and r.stdout == b"" and b"CLI PARSER ERROR" in r.stderr, extra
