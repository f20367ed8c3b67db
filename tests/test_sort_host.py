"""The coordinate order of records without a GPU: flx_sort_host and a sort object on device -1 against the plain-numpy rule of
tests/sort_ref.py, every refusal, the sorted BAM writer (flx_sam_open_sorted on device -1) against the unsorted writer's records, the BAI
index read back with sort_ref's own reader and queried region by region, the CLI's parser errors, and tests/sort_check.cpp: the rule
header under ASan + UBSan."""
import ctypes as C
import gzip
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import sort_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the rule
def host_and_object(n_refs, rec, words, adds):
    """flx_sort_host and the host object (adds: [(indices, first_ordinal)]) against the reference; returns the entries"""
    ordinals = np.zeros(len(rec), dtype=np.uint64)
    for idx, first in adds:
        ordinals[idx] = first + np.arange(len(idx), dtype=np.uint64)
    want = R.entries(rec, words, ordinals)
    got = F.sort_host(n_refs, rec, words, ordinals)
    assert got.dtype == want.dtype and (got == want).all()
    s = F.record_sorter(n_refs, device=-1)
    for idx, first in adds:
        order = s.add_records(rec[idx], words, first)
        assert (np.asarray(idx)[order] == np.asarray(idx)[R.order(rec[idx], first + np.arange(len(idx), dtype=np.uint64))]).all()
    assert len(s) == len(rec)
    s.finish()
    assert (s.entries() == want).all()
    if len(rec) > 4:
        assert (s.entries(1, 4) == want[1:4]).all()
    s.close()
    return want


def test_all_keys_equal_only_ordinals_decide():
    rec, words = R.records_of([(0, 1, 500, [R.word("=", 5)])] * 50)
    rng = np.random.default_rng(1)
    idx = rng.permutation(50)
    want = host_and_object(2, rec, words, [(idx[:20], 7 << 32), (idx[20:], 3 << 32)])
    assert (np.diff(want["ordinal"].astype(np.int64)) > 0).all() and int(want["ordinal"][0]) == 3 << 32


def test_strand_and_top_byte_alone():
    top = 1 << 24
    rows = [(16, 1, 9, []), (0, 1, 9, []), (272, 1, 9, []), (256, 1, 9, []), (0, 1 | top, 9, []), (16, 1, 9, []), (0, 1, 9, []), (2064, 1 | top, 9, []), (2048, 1 | top, 9, [])]
    rec, words = R.records_of(rows)
    want = host_and_object(top + 2, rec, words, [(np.arange(len(rows)), 0)])
    assert want["ordinal"].tolist() == [1, 3, 6, 0, 2, 5, 4, 8, 7]          # forward before reverse whatever the ordinals; the top byte above all


def test_unplaced_last_in_ordinal_order():
    rows = [(4, -1, 0, []), (0, 0, 5, []), (4, 1, 3, []), (20, -1, 0, []), (0, -1, 7, []), (16, 1, 0, [])]
    rec, words = R.records_of(rows)
    want = host_and_object(2, rec, words, [(np.arange(6), 100)])
    assert want["ref"].tolist() == [0, 1, -1, -1, -1, -1]
    # among the unplaced: position, then strand, then ordinal; a flag-4 record that names a reference is unplaced all the same
    assert want["ordinal"].tolist() == [101, 105, 100, 103, 102, 104]


def test_positions_at_the_extremes_and_ends():
    longest = (1 << 28) - 1
    far = [R.word("D", longest)] * 8 + [R.word("=", (1 << 31) - 2 - 8 * longest)]
    rows = [(0, 0, (1 << 31) - 2, []), (0, 0, 0, []), (16, 0, 0, far), (0, 0, 1, far), (0, 0, 7, [R.word("S", 3), R.word("I", 2)]),
            (0, 0, 7, [R.word("S", 3), R.word("=", 4), R.word("I", 2), R.word("X", 1), R.word("D", 6), R.word("S", 9)])]
    rec, words = R.records_of(rows)
    want = host_and_object(1, rec, words, [(np.arange(len(rows)), 0)])
    assert want["pos"].tolist() == [0, 0, 1, 7, 7, (1 << 31) - 2]
    assert want["end"].tolist() == [1, (1 << 31) - 2, (1 << 31) - 1, 8, 18, (1 << 31) - 1]


def test_ordinals_above_32_bits_and_shuffled_adds():
    rng = np.random.default_rng(5)
    rec, words = R.random_records(rng, 700, max_pos=30)
    idx = rng.permutation(700)
    cuts = [0, 1, 64, 65, 300, 700]
    firsts = [(1 << 63) - 2, 9 << 32, (1 << 62) + 5, 1 << 32, 0]
    adds = [(idx[cuts[k]: cuts[k + 1]], firsts[k]) for k in range(5)]
    a = host_and_object(3, rec, words, adds)
    b = host_and_object(3, rec, words, adds[::-1])
    assert (a == b).all() and int(a["ordinal"].max()) == (1 << 63) - 2


def test_refusals_leave_the_object_as_it_was():
    rec, words = R.records_of([(0, 0, 5, [R.word("=", 4)]), (16, 1, 9, [R.word("=", 2), R.word("D", 1)]), (4, -1, 0, [])])
    ords = np.arange(3, dtype=np.uint64)
    s = F.record_sorter(2, device=-1)
    s.add_records(rec, words, 1 << 32)

    def refused(r, w, first, match, host_ordinals=ords):
        with pytest.raises(F.FloxerError, match=match):
            s.add_records(r, w, first)
        assert len(s) == 3
        if host_ordinals is not None:
            with pytest.raises(F.FloxerError, match=match):
                F.sort_host(2, r, w, host_ordinals)
    bad = rec.copy(); bad["ref"][0] = 2
    refused(bad, words, 2 << 32, "reference_id")
    bad = rec.copy(); bad["pos"][1] = -1
    refused(bad, words, 2 << 32, "negative")
    refused(rec, np.array([R.word("=", 4), 3 << 4 | 0, R.word("D", 1)], dtype=np.uint32), 2 << 32, "op other")
    refused(rec, np.array([R.word("=", 4), 3 << 4 | 3, R.word("D", 1)], dtype=np.uint32), 2 << 32, "op other")
    refused(rec, np.array([R.word("=", 4), 0 << 4 | 7, R.word("D", 1)], dtype=np.uint32), 2 << 32, "length 0")
    refused(rec, words[:2], 2 << 32, "outside the pool")
    bad = rec.copy(); bad["coff"][1] = (1 << 64) - 1
    refused(bad, words, 2 << 32, "outside the pool")
    bad = rec.copy(); bad["pos"][0] = (1 << 31) - 4
    refused(bad, words, 2 << 32, "2\\^31")
    refused(rec, words, 1 << 63, "2\\^63", host_ordinals=np.array([0, 1 << 63, 2], dtype=np.uint64))
    refused(rec, words, (1 << 63) - 2, "2\\^63", host_ordinals=None)
    refused(rec, words, 1 << 32, "added before", host_ordinals=None)
    s.finish()
    assert (s.entries() == R.entries(rec, words, (1 << 32) + ords)).all()
    with pytest.raises(F.FloxerError, match="finished"):
        s.add_records(rec, words, 5 << 32)
    with pytest.raises(F.FloxerError, match="finished"):
        s.finish()
    s.close()


def test_abi_and_geometry():
    L = capi.lib()
    names = [n for n in capi.EXPORTED if n.startswith("flx_sort")]
    assert len(names) == 9 and "flx_sam_open_sorted" in capi.EXPORTED
    for name in names + ["flx_sam_open_sorted"]:
        getattr(L, name)
    assert C.sizeof(capi.SortOptions) == 32 and C.sizeof(capi.SortEntry) == 24 and F.SORT_ENTRY_DTYPE.itemsize == 24 and F.SORT_ENTRY_DTYPE == R.ENTRY_DTYPE
    tile, bits, cap, scan = F.sort_geometry()
    assert bits == 8 and tile % 256 == 0 and cap >= 64 and scan >= 256
    for bad in (F.sort_options(tile_keys=100),):
        with pytest.raises(F.FloxerError, match="tile_keys"):
            F.record_sorter(2, device=-1, options=bad)
    with pytest.raises(F.FloxerError):
        F.record_sorter(2, device=-2)
    s = F.record_sorter(2, device=-1)
    with pytest.raises(F.FloxerError, match="finish"):
        s.entries()
    s.finish()
    assert len(s.entries()) == 0
    s.close()


def test_rule_header_under_sanitizers(tmp_path):
    """tests/sort_check.cpp: flx_sort.hpp alone, built with ASan + UBSan"""
    exe = str(tmp_path / "sort_check")
    src = os.path.join(ROOT, "tests", "sort_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


def test_reference_bins():
    assert R.reg2bin(0, 1) == 4681 and R.reg2bin(16383, 16385) == 585 and R.reg2bin(0, 1 << 29) == 0
    rng = np.random.default_rng(2)
    for _ in range(500):
        a = int(rng.integers(0, 1 << 29))
        b = min(1 << 29, a + 1 + int(rng.integers(0, 1 << int(rng.integers(1, 28)))))
        bins = R.reg2bins(a, b)
        assert R.reg2bin(a, b) in bins and len(set(bins)) == len(bins)
        inner = int(rng.integers(a, b))
        assert R.reg2bin(inner, inner + 1) in bins                        # a record inside the region lies in one of its bins


# ------------------------------------------------------------------------------------------------ the sorted writer
REF_NAMES = [b"chrA", b"chrB", b"chrEmpty", b"chrD"]
REF_LENS = [(1 << 27) + 5000, 5_000_000, 77_000, 40_000]
EDGES = [0, 16383, 16384, 16385, (1 << 17) - 1, 1 << 17, (1 << 20) - 2, 1 << 20, (1 << 26) - 1, 1 << 26, (1 << 26) + 1]


def dataset():
    """reads with one to six records each (a read's records contiguous), many of them on the windows' and bins' boundaries, on both
    strands, some sharing one CIGAR array, some unmapped; about 350 KB of BAM, several BGZF blocks"""
    rng = np.random.default_rng(17)
    n_reads = 420
    lens = rng.integers(90, 260, size=n_reads)
    pool = rng.integers(1, 5, size=int(lens.sum()), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ids = [f"read{i:04d}".encode() for i in range(n_reads)]
    quals = [bytes(rng.integers(35, 70, size=int(n), dtype=np.uint8)) if i % 7 else b"" for i, n in enumerate(lens)]
    rows, words = [], []
    for i in range(n_reads):
        if i % 11 == 3:
            rows.append((i, 4, -1, 0, 0, 0, 0, 0))
            continue
        n = int(lens[i])
        cigars = []
        for _ in range(2):                                                # two CIGAR arrays per read, shared by its records
            gap = int(rng.choice([0, 0, 3, 20_000, 140_000]))
            cig = [R.word("S", 5), R.word("=", n // 2 - 5), R.word("X", 1)] + ([R.word("D", gap)] if gap else []) + [R.word("I", 2), R.word("=", n - n // 2 - 3)]
            cigars.append((len(words), len(cig)))
            words.extend(cig)
        for k in range(int(rng.integers(1, 7))):
            ref = int(rng.choice([0, 0, 0, 1, 1, 3]))
            if rng.random() < 0.6 and ref == 0:
                pos = int(rng.choice(EDGES)) + int(rng.integers(-2, 3))
                pos = max(0, pos - (n // 2 if rng.random() < 0.5 else 0))
            elif rng.random() < 0.3:
                pos = 1000                                                # many records at one place: strand and written order decide
            else:
                pos = int(rng.integers(0, REF_LENS[ref] - 200_000 if ref < 2 else 30_000))
            flag = (0 if k == 0 else 256) | (16 if rng.random() < 0.5 else 0)
            off, ln = cigars[int(rng.integers(0, 2)) if k else 0]
            rows.append((i, flag, ref, pos, int(rng.integers(0, 9)), off, ln, int(rng.integers(0, 61))))
    rec = np.array(rows, dtype=R.REC_DTYPE)
    return dict(ids=ids, quals=quals, pool=pool, offs=offs, rec=rec, words=np.array(words, dtype=np.uint32), n_reads=n_reads)


@pytest.fixture(scope="module")
def data():
    return dataset()


def write(data, path, sorted_=True, calls=1, threads=1, index=False, device=-1, ref_lens=REF_LENS, spill=None, mapq=True):
    """the dataset through flx_sam_open_sorted (or flx_sam_open), in `calls` write calls cut at read boundaries; returns (rc of open, rcs of the writes, rc of close)"""
    L = capi.lib()
    n_refs = len(REF_NAMES)
    ref_ids = (C.c_char_p * n_refs)(*REF_NAMES)
    lens = np.array(ref_lens, dtype=np.uint64)
    ids = (C.c_char_p * data["n_reads"])(*data["ids"])
    quals = (C.c_char_p * data["n_reads"])(*data["quals"])
    w = C.c_void_p()
    spill = spill or path + ".spill"
    if sorted_:
        rc = L.flx_sam_open_sorted(path.encode(), spill.encode(), device, int(index), ref_ids, capi.ptr(lens, capi.u64p), n_refs, C.byref(w))
    else:
        rc = L.flx_sam_open(path.encode(), ref_ids, capi.ptr(lens, capi.u64p), n_refs, C.byref(w))
    if rc:
        return rc, [], None
    capi.check(L.flx_sam_set_threads(w, threads))
    capi.check(L.flx_sam_set_mapq(w, int(mapq)))
    rec = data["rec"]
    read_cuts = [data["n_reads"] * k // calls for k in range(calls + 1)]
    cuts = np.searchsorted(rec["read"], read_cuts, side="left")
    cuts[-1] = len(rec)
    rcs = []
    for k in range(calls):
        part = np.ascontiguousarray(rec[cuts[k]: cuts[k + 1]])
        rcs.append(L.flx_sam_write(w, ids, capi.ptr(data["pool"], capi.u8p), capi.ptr(data["offs"], capi.u64p), quals,
                                   part.ctypes.data_as(C.POINTER(capi.Record)), len(part), capi.ptr(data["words"], capi.u32p)))
    return 0, rcs, L.flx_sam_close(w)


def record_key(r):
    un = r["ref"] < 0 or r["flag"] & 4
    return (0xFFFFFFFF if un else r["ref"], r["pos"] & 0xFFFFFFFF, (r["flag"] >> 4) & 1)


@pytest.fixture(scope="module")
def files(data, tmp_path_factory):
    d = tmp_path_factory.mktemp("sorted")
    paths = {k: str(d / f"{k}.bam") for k in ("plain", "one", "three", "seven", "threads8", "indexed")}
    assert write(data, paths["plain"], sorted_=False) == (0, [0], 0)
    assert write(data, paths["one"]) == (0, [0], 0)
    assert write(data, paths["three"], calls=3) == (0, [0] * 3, 0)
    assert write(data, paths["seven"], calls=7) == (0, [0] * 7, 0)
    assert write(data, paths["threads8"], calls=3, threads=8) == (0, [0] * 3, 0)
    assert write(data, paths["indexed"], calls=3, threads=3, index=True) == (0, [0] * 3, 0)
    for p in paths.values():
        assert not os.path.exists(p + ".spill")                          # gone after close
    return paths


def test_calls_do_not_change_the_stream(files):
    one = R.Bam(files["one"])
    assert len(one.members) > 4 and len(one.records) > 1000
    for other in ("three", "seven"):
        assert R.Bam(files[other]).stream == one.stream, other


def test_threads_do_not_change_the_file(files):
    a, b, c = (open(files[k], "rb").read() for k in ("three", "threads8", "indexed"))
    assert a == b == c
    assert not os.path.exists(files["three"] + ".bai") and os.path.exists(files["indexed"] + ".bai")


def test_sorted_against_unsorted(files, data):
    plain, got = R.Bam(files["plain"]), R.Bam(files["seven"])
    assert len(plain.records) == len(data["rec"]) == len(got.records)
    assert Counter(r["bytes"] for r in plain.records) == Counter(r["bytes"] for r in got.records)
    want = sorted(plain.records, key=record_key)                          # (stable: equal keys keep the written order)
    assert [r["bytes"] for r in got.records] == [r["bytes"] for r in want]
    keys = [record_key(r) for r in got.records]
    assert keys == sorted(keys) and len(set(keys)) < len(keys) and any(k[0] == 0xFFFFFFFF for k in keys)
    assert plain.text.startswith("@HD\tVN:1.6\n@SQ") and got.text.startswith("@HD\tVN:1.6\tSO:coordinate\n@SQ")
    assert got.text.split("\n", 1)[1] == plain.text.split("\n", 1)[1] and got.refs == plain.refs == [(n.decode(), l) for n, l in zip(REF_NAMES, REF_LENS)]
    assert got.has_eof and plain.has_eof
    with gzip.open(files["seven"], "rb") as f:                            # every member passes Python's gzip
        assert f.read() == got.stream
    # the order is the library's own as well: entries of the records with the writer's ordinals (one call: k = 0)
    rec = data["rec"]
    assert [(r["ref"], r["pos"], r["flag"]) for r in R.Bam(files["one"]).records] == [(int(a), int(b), int(c)) for a, b, c in
                                                                                  zip(*(F.sort_host(4, rec, data["words"], np.arange(len(rec)))[k] for k in ("ref", "pos", "flag")))]


def test_spill_is_removed_after_failures(data, tmp_path):
    spill = str(tmp_path / "spill.tmp")
    # an output that cannot be created: refused at open, and the spill file made just before is gone
    rc, _, _ = write(data, str(tmp_path / "no_such_dir" / "o.bam"), spill=spill)
    assert rc == -6 and not os.path.exists(spill)
    # a spill file that cannot be created
    rc, _, _ = write(data, str(tmp_path / "o.bam"), spill=str(tmp_path / "no_such_dir" / "spill.tmp"))
    assert rc == -6 and "spill" in capi.lib().flx_last_error().decode()
    # a record that cannot be written (a read name of 300 characters): the write fails, close reports it and removes the spill file
    broken = dict(data, ids=[b"x" * 300] + data["ids"][1:])
    rc, rcs, rc_close = write(broken, str(tmp_path / "o.bam"), spill=spill, calls=2)
    assert rc == 0 and rcs[0] == -1 and rcs[1] != 0 and rc_close != 0 and not os.path.exists(spill)
    # not a .bam
    rc, _, _ = write(data, str(tmp_path / "o.sam"), spill=spill)
    assert rc == -1 and not os.path.exists(spill)


def test_index_limit(data, tmp_path):
    lens = list(REF_LENS)
    lens[2] = (1 << 29) + 1
    rc, _, _ = write(data, str(tmp_path / "big.bam"), index=True, ref_lens=lens)
    assert rc == -1
    msg = capi.lib().flx_last_error().decode()
    assert "chrEmpty" in msg and "2^29" in msg and not os.path.exists(str(tmp_path / "big.bam.spill"))
    assert write(data, str(tmp_path / "big.bam"), index=False, ref_lens=lens) == (0, [0], 0)
    lens[2] = 1 << 29
    assert write(data, str(tmp_path / "fits.bam"), index=True, ref_lens=lens) == (0, [0], 0)


# ------------------------------------------------------------------------------------------------ the index
def check_index_structure(bam, bai):
    assert len(bai.refs) == len(bam.refs)
    by_start = {r["vstart"]: i for i, r in enumerate(bam.records)}
    placed = [r for r in bam.records if not (r["ref"] < 0 or r["flag"] & 4)]
    assert bai.n_no_coor == len(bam.records) - len(placed)
    for ref, idx in enumerate(bai.refs):
        mine = [r for r in placed if r["ref"] == ref]
        if not mine:
            assert idx["bins"] == {} and idx["pseudo"] is None and idx["linear"] == []
            continue
        seen = 0
        for b, chunks in idx["bins"].items():
            assert chunks and all(beg < end for beg, end in chunks), b   # non-empty
            assert all(chunks[k][1] <= chunks[k + 1][0] for k in range(len(chunks) - 1)), b      # ordered
            for beg, end in chunks:
                i = by_start[beg]
                while i < len(bam.records) and bam.records[i]["vstart"] < end:
                    assert bam.records[i]["bin"] == b and bam.records[i]["ref"] == ref
                    assert R.reg2bin(bam.records[i]["pos"], bam.records[i]["end"]) == b
                    seen += 1
                    i += 1
                assert bam.records[i - 1]["vend"] == end                  # the first byte behind the chunk's last record
        assert seen == len(mine)                                          # every record in exactly one chunk
        assert idx["pseudo"] == (mine[0]["vstart"], mine[-1]["vend"], len(mine), 0)
        lin = idx["linear"]
        assert len(lin) == ((max(r["end"] for r in mine) - 1) >> 14) + 1 and all(a <= b for a, b in zip(lin, lin[1:]))
        want, before = [], 0
        for w in range(len(lin)):
            over = [r["vstart"] for r in mine if r["pos"] < (w + 1) << 14 and r["end"] > w << 14]
            before = min(over) if over else before
            want.append(before)
        assert lin == want
    return placed


def check_region_queries(bam, bai, seed, n_random=200, min_hits=1000):
    rng = np.random.default_rng(seed)
    regions = []
    for ref, (_, length) in enumerate(bam.refs):
        for e in EDGES + [16384 * 3, (1 << 20) + (1 << 14)]:
            if e < length:
                regions += [(ref, max(0, e - 1), e), (ref, e, e + 1), (ref, max(0, e - 1), e + 1), (ref, e, min(length, e + 16384)), (ref, max(0, e - 20_000), min(length, e + 20_000))]
        regions.append((ref, 0, length))
    while len(regions) < n_random + 60:
        ref = int(rng.integers(0, len(bam.refs)))
        length = bam.refs[ref][1]
        a = int(rng.integers(0, length)) if rng.random() < 0.5 else min(length - 1, max(0, int(rng.choice(EDGES)) + int(rng.integers(-300, 300))))
        b = min(length, a + 1 + int(rng.integers(0, 1 << int(rng.integers(1, 22)))))
        regions.append((ref, a, b))
    hits = 0
    for ref, a, b in regions:
        brute = {i for i, r in enumerate(bam.records) if r["ref"] == ref and not r["flag"] & 4 and r["pos"] < b and r["end"] > a}
        assert bai.query(bam, ref, a, b) == brute, (ref, a, b)
        hits += len(brute)
    assert hits >= min_hits and len(regions) >= 200


def test_index_structure_and_region_queries(files):
    bam, bai = R.Bam(files["indexed"]), R.Bai(files["indexed"] + ".bai")
    placed = check_index_structure(bam, bai)
    assert bai.n_no_coor > 10 and len(placed) > 1000 and bai.refs[2]["bins"] == {} and len(bai.refs[0]["bins"]) > 20
    assert {0, 1, 9, 73, 585, 4681} & set(bai.refs[0]["bins"]) and len(bai.refs[0]["linear"]) > 4096
    assert any(len(c) > 1 for c in bai.refs[0]["bins"].values())          # a bin left and entered again: two chunks
    check_region_queries(bam, bai, 3)


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_sort_flags(tmp_path):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    g = os.path.join(ROOT, "tests", "golden")
    base = [exe, "--reference", os.path.join(g, "reference.fasta"), "--queries", os.path.join(g, "queries.fastq"), "-e", "2"]
    h = subprocess.run([exe, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    text = (h.stdout + h.stderr).decode()
    for opt in ("--sort-by-coordinate", "--bam-index", "--sort-tmp"):
        assert opt in text and "not floxer's" in [l for l in text.splitlines() if opt in l][0]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")                      # (parser errors come before any device is opened)
    bam, sam = str(tmp_path / "o.bam"), str(tmp_path / "o.sam")
    for extra, needle in ((["--output", bam, "--bam-index"], b"--sort-by-coordinate"),
                          (["--output", bam, "--sort-tmp", str(tmp_path)], b"--sort-by-coordinate"),
                          (["--output", sam, "--sort-by-coordinate"], b".bam"),
                          (["--output", sam, "--sort-by-coordinate", "--bam-index"], b".bam"),
                          (["--output", bam, "--sort-by-coordinate", "--sort-tmp"], b"sort-tmp")):
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode != 0 and b"CLI PARSER ERROR" in r.stderr and needle in r.stderr, (extra, r.stderr)
    assert not os.path.exists(bam) and not os.path.exists(sam)
