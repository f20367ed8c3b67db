"""The coordinate order of records on the GPU (flx_sort: kernels sort_keys_add, sort_census, sort_histogram, the table's scan,
sort_scatter, sort_entries; runs and the Python class). Every device result must equal flx_sort_host's on the same records, words and
ordinals, exactly; test_sort_host.py holds flx_sort_host against the plain-numpy rule of tests/sort_ref.py. The sizes come from
sort_geometry() and sit on the kernels' boundaries: a wave, a block's step of its tile, a tile, the scan tile of the digit table."""
import os
import subprocess
import threading
from collections import Counter

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import sort_ref as R

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 256                                                               # a block's threads: tile_keys is a multiple


def synthetic(rng, n, n_refs=5, max_pos=1 << 20, words_per=2, one_ref=False, one_pos=False):
    """n records without the per-row Python loop: flags of both strands, a share of unplaced records, a few words each"""
    rec = np.zeros(n, dtype=R.REC_DTYPE)
    rec["read"] = np.arange(n)
    rec["flag"] = rng.choice(np.array([0, 16, 256, 272, 2048, 2064], dtype=np.uint32), size=n)
    rec["ref"] = 2 if one_ref else rng.integers(0, n_refs, size=n)
    rec["pos"] = 77 if one_pos else rng.integers(0, max_pos, size=n)
    un = rng.random(n) < 0.05
    rec["flag"][un] = 4
    rec["ref"][un] = -1
    rec["pos"][un] = 0
    ops = np.array([R.OPS[c] for c in "=XIDS"], dtype=np.uint32)
    words = (rng.integers(1, 50, size=max(1, n * words_per)).astype(np.uint32) << 4) | rng.choice(ops, size=max(1, n * words_per))
    rec["coff"] = np.arange(n) * words_per
    rec["clen"] = np.where(un, 0, words_per)
    return rec, words


def on_device(n_refs, rec, words, adds, options=None, threads=0):
    """adds: [(indices into rec, first_ordinal)]; returns (entries, the out_order of every add, the ordinals the adds gave)"""
    ordinals = np.zeros(len(rec), dtype=np.uint64)
    for idx, first in adds:
        ordinals[idx] = first + np.arange(len(idx), dtype=np.uint64)
    s = F.record_sorter(n_refs, options=options)
    try:
        orders = [None] * len(adds)

        def work(k):
            idx, first = adds[k]
            orders[k] = s.add_records(rec[idx], words, first)
        if threads:
            pool = [threading.Thread(target=lambda t=t: [work(k) for k in range(t, len(adds), threads)]) for t in range(threads)]
            for t in pool:
                t.start()
            for t in pool:
                t.join()
        else:
            for k in range(len(adds)):
                work(k)
        assert len(s) == sum(len(idx) for idx, _ in adds)
        s.finish()
        got = s.entries()
        if len(got) > 10:                                                 # a stretch in the middle is the same stretch
            a, b = len(got) // 3, len(got) // 3 + 7
            assert (s.entries(a, b) == got[a:b]).all() and len(s.entries(b, b)) == 0
    finally:
        s.close()
    return got, orders, ordinals


def check(n_refs, rec, words, adds, options=None, threads=0):
    got, orders, ordinals = on_device(n_refs, rec, words, adds, options, threads)
    want = F.sort_host(n_refs, rec, words, ordinals)
    assert got.dtype == want.dtype and len(got) == len(want)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    for (idx, first), order in zip(adds, orders):                        # every add's own order: the host's entries of the add alone name it
        part = F.sort_host(n_refs, rec[idx], words, first + np.arange(len(idx), dtype=np.uint64))
        assert order.dtype == np.uint32 and len(order) == len(idx)
        assert (first + order.astype(np.uint64) == part["ordinal"]).all()
    return got


def one_add(n):
    return [(np.arange(n), 5 << 32)]


# ------------------------------------------------------------------------------------------------ sizes
def sizes():
    tile, bits, cap, scan = F.sort_geometry()
    assert bits == 8 and tile % BLOCK == 0 and scan * scan // 256 >= 17
    tiles_past_scan = scan // 256 + 1                                     # the tile x digit table outgrows one scan tile
    return [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, tile - 1, tile, tile + 1, 3 * tile + 1, tiles_past_scan * tile + 5]


@gpu
@pytest.mark.parametrize("which", range(13))
def test_sizes(which):
    n = sizes()[which]
    rec, words = synthetic(np.random.default_rng(which), n)
    got = check(5, rec, words, one_add(n))
    if n > 1000:
        assert (got["ref"] == -1).any() and (got["flag"] & 16 != 0).any() and len(set(got["ref"].tolist())) == 6


@gpu
@pytest.mark.parametrize("tile_keys,n_tiles", [(256, 17), (256, 300), (512, 41), (4096, 3)])
def test_small_and_large_tiles(tile_keys, n_tiles):
    """tile_keys below and above the default: one step per tile and many, and (300 tiles) a digit table of 19 scan tiles. The scan has
    two levels at most: sort_effective_tile (tests/sort_check.cpp) grows the tiles before a third would be needed."""
    n = tile_keys * n_tiles - 3
    rec, words = synthetic(np.random.default_rng(n_tiles), n)
    check(5, rec, words, one_add(n), options=F.sort_options(tile_keys=tile_keys))


@gpu
def test_options_refused():
    for bad in (F.sort_options(tile_keys=100), F.sort_options(tile_keys=BLOCK + 64)):
        with pytest.raises(F.FloxerError, match="tile_keys"):
            F.record_sorter(2, options=bad)
    o = F.sort_options()
    o.reserved[2] = 1
    with pytest.raises(F.FloxerError, match="reserved"):
        F.record_sorter(2, options=o)


# ------------------------------------------------------------------------------------------------ CIGAR words
@gpu
@pytest.mark.parametrize("n_words", [1, 63, 64, 65, 129, 4097])
def test_words(n_words):
    rng = np.random.default_rng(n_words)
    plain = [R.word("=X"[int(rng.integers(0, 2))], int(rng.integers(1, 9))) for _ in range(n_words)]
    gaps = [R.word("=XD"[int(rng.integers(0, 3))], int(rng.integers(1, 9))) for _ in range(n_words)]
    mixed = [R.word("=XIDS"[int(rng.integers(0, 5))], int(rng.integers(1, 9))) for _ in range(n_words)]
    only_i_s = [R.word("IS"[i % 2], 3) for i in range(n_words)]           # no reference column at all: end = position + 1
    # a span that reaches 2^31 - 2: the longest words there are, and the rest in the last one
    longest = (1 << 28) - 1
    far = [R.word("D", longest)] * 8 + [R.word("=", (1 << 31) - 2 - 8 * longest)]
    rows = [(0, 0, 11, plain), (16, 1, 0, gaps), (0, 1, 5, mixed), (2048, 0, 5, only_i_s), (0, 1, 0, far), (16, 1, 1, far), (0, 1, (1 << 31) - 2, []),
            (4, -1, 0, mixed), (0, 0, 0, [])]
    rec, words = R.records_of(rows)
    got = check(2, rec, words, one_add(len(rec)))
    want = R.entries(rec, words, (5 << 32) + np.arange(len(rec), dtype=np.uint64))
    assert (got == want).all() and int(got["end"].max()) == (1 << 31) - 1 and (1 << 31) - 2 in got["end"].tolist()


# ------------------------------------------------------------------------------------------------ growth
@gpu
def test_growth_across_initial_capacity():
    rng = np.random.default_rng(4)
    parts = [1, 62, 1, 1, 64, 65, 200, 3, 1000, 0, 7]
    n = sum(parts)
    rec, words = synthetic(rng, n, max_pos=500)
    cuts = np.cumsum([0] + parts)
    adds = [(np.arange(cuts[k], cuts[k + 1]), (k + 1) << 32) for k in range(len(parts))]
    check(5, rec, words, adds, options=F.sort_options(initial_capacity=64))


# ------------------------------------------------------------------------------------------------ constant digits
@gpu
@pytest.mark.parametrize("case", ["one_reference", "one_position", "one_call", "all_equal", "two_values_top_byte"])
def test_digit_skips(case):
    tile = F.sort_geometry()[0]
    n = 2 * tile + 77
    rng = np.random.default_rng(9)
    rec, words = synthetic(rng, n, one_ref=case in ("one_reference", "all_equal"), one_pos=case in ("one_position", "all_equal"))
    adds = one_add(n)
    if case == "all_equal":                                               # only the ordinals decide, and they come in shuffled adds
        rec["flag"], rec["ref"], rec["pos"] = 0, 2, 77
    if case in ("all_equal", "one_reference"):
        idx = rng.permutation(n)
        adds = [(idx[: n // 3], 9 << 32), (idx[n // 3:], 2 << 32)]
    if case == "two_values_top_byte":                                     # keys that differ in the top byte of hi alone, or in the strand alone
        rec["flag"] = np.where(rng.random(n) < 0.5, 0, 16)
        rec["ref"] = np.where(rng.random(n) < 0.5, 1, 1 | 1 << 24)
        rec["pos"] = 3
    check((1 << 24) + 2, rec, words, adds)


@gpu
def test_ordinals_with_high_bits():
    rng = np.random.default_rng(12)
    n = 3000
    rec, words = synthetic(rng, n, max_pos=40)
    cuts = [0, 1000, 1001, 3000]
    firsts = [(1 << 63) - 1 - 1000, 1 << 62, (1 << 40) + 5]
    check(5, rec, words, [(np.arange(cuts[k], cuts[k + 1]), firsts[k]) for k in range(3)])


# ------------------------------------------------------------------------------------------------ threads
@gpu
def test_eight_threads_add_shuffled_parts():
    rng = np.random.default_rng(21)
    n = 20_000
    rec, words = synthetic(rng, n, max_pos=3000)
    idx = rng.permutation(n)
    cuts = np.sort(rng.choice(np.arange(1, n), size=39, replace=False))
    parts = np.split(idx, cuts)
    adds = [(part, (k + 1) << 32) for k, part in enumerate(parts)]
    threaded = check(5, rec, words, adds, options=F.sort_options(initial_capacity=64), threads=8)
    single, _, _ = on_device(5, rec, words, adds[::-1])
    assert (threaded == single).all()


# ------------------------------------------------------------------------------------------------ refusals and lifetime
@gpu
def test_refusals_leave_the_object_as_it_was():
    rec, words = R.records_of([(0, 0, 5, [R.word("=", 4)]), (16, 1, 9, [R.word("=", 2), R.word("D", 1)]), (4, -1, 0, [])])
    s = F.record_sorter(2)
    s.add_records(rec, words, 1 << 32)

    def refused(r, w, first, match):
        with pytest.raises(F.FloxerError, match=match):
            s.add_records(r, w, first)
        assert len(s) == 3
    bad = rec.copy(); bad["ref"][0] = 2
    refused(bad, words, 2 << 32, "reference_id")
    bad = rec.copy(); bad["pos"][1] = -1
    refused(bad, words, 2 << 32, "negative")
    refused(rec, np.array([R.word("=", 4), 3 << 4 | 0, R.word("D", 1)], dtype=np.uint32), 2 << 32, "op other")
    refused(rec, np.array([R.word("=", 4), 0 << 4 | 7, R.word("D", 1)], dtype=np.uint32), 2 << 32, "length 0")
    refused(rec, words[:2], 2 << 32, "outside the pool")
    bad = rec.copy(); bad["pos"][0] = (1 << 31) - 4
    refused(bad, words, 2 << 32, "2\\^31")
    refused(rec, words, 1 << 63, "2\\^63")
    refused(rec, words, (1 << 63) - 2, "2\\^63")
    refused(rec, words, 1 << 32, "added before")
    s.add_records(rec[:0], words, 1 << 32)                                # an empty add takes no ordinal
    s.add_records(rec, words, 0)
    s.finish()
    want = F.sort_host(2, np.concatenate([rec, rec]), words, np.concatenate([(1 << 32) + np.arange(3), np.arange(3)]).astype(np.uint64))
    assert (s.entries() == want).all()
    for again in (lambda: s.finish(), lambda: s.add_records(rec, words, 7 << 32), lambda: s.entries(0, 7), lambda: s.entries(3, 2)):
        with pytest.raises(F.FloxerError):
            again()
    s.close()
    empty = F.record_sorter(2)
    with pytest.raises(F.FloxerError, match="finish"):
        empty.entries()
    empty.finish()
    assert len(empty.entries()) == 0
    empty.close()


# ------------------------------------------------------------------------------------------------ pipeline
@gpu
def test_aligner_runs(monkeypatch):
    """an aligner run on a small simulated reference with both strands: add(run) equals sort_host on the run's copied records, as a
    RunResult and as a raw run of several parts"""
    import ctypes as C
    from test_md_gpu import RATE, _planted
    chroms, reads = _planted()
    ctx = F.context(F.fmindex(chroms))
    try:
        p = F.params(error_probability=RATE)
        result = F.aligner(ctx, p).align_reads(reads)
        flags = {int(f) for f in result.raw["flag"]}
        assert 0 in flags and 16 in flags and 4 in flags and len(result.raw) > 100
        n = len(result.raw)
        want = F.sort_host(len(chroms), result.raw, result.cigars, (3 << 32) + np.arange(n, dtype=np.uint64))
        assert (want == R.entries(result.raw, result.cigars, (3 << 32) + np.arange(n, dtype=np.uint64))).all()
        s = F.record_sorter(len(chroms))
        order = s.add(result, 3 << 32)
        s.finish()
        assert (s.entries() == want).all() and ((3 << 32) + order.astype(np.uint64) == want["ordinal"]).all()
        s.close()
        L = capi.lib()
        pool, offs, n_reads = F._pool_and_offsets(reads)
        monkeypatch.setenv("FLX_CHUNK_READS", "9")                        # several parts, each with its own word pool
        run = C.c_void_p()
        capi.check(L.flx_align_reads(ctx.h, C.byref(p), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n_reads, C.byref(run)))
        monkeypatch.delenv("FLX_CHUNK_READS")
        assert L.flx_run_num_records(run) == n
        s = F.record_sorter(len(chroms))
        order = s.add(run, 3 << 32)
        L.flx_run_free(run)
        s.finish()
        assert (s.entries() == want).all() and ((3 << 32) + order.astype(np.uint64) == want["ordinal"]).all()
        s.close()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ CLI
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLI_BASE = ["--reference", os.path.join(GOLDEN, "reference.fasta"), "--queries", os.path.join(GOLDEN, "queries.fastq"), "--query-errors", "2", "--seed-errors", "1",
            "--extra-verification-ratio", "2", "--threads", "1"]
CLI_CONFIGS = {"default": [], "selected": ["-D", "-N", "1", "-Q", "--md-tag"], "without_cigar": ["-w"]}


def cli(tmp_path, out, *extra):
    exe = os.path.join(ROOT, "floxer_amd", "floxer")
    env = dict(os.environ, FLX_BATCH_READS="3")                           # several batches: several runs to merge
    r = subprocess.run([exe, *CLI_BASE, "--output", str(tmp_path / out), *extra], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    return str(tmp_path / out), r.stderr.decode()


def sorted_against_plain(tmp_path, config, *devices):
    from test_sort_host import check_index_structure, check_region_queries, record_key
    flags = CLI_CONFIGS[config]
    plain, _ = cli(tmp_path, "plain.bam", *flags, *devices)
    got, log = cli(tmp_path, "sorted.bam", *flags, *devices, "--sort-by-coordinate", "--bam-index", "--sort-tmp", str(tmp_path))
    assert "merging the spilled batches" in log and os.listdir(tmp_path) and not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
    a, b = R.Bam(plain), R.Bam(got)
    assert len(a.records) >= 6 and Counter(r["bytes"] for r in a.records) == Counter(r["bytes"] for r in b.records)
    assert [r["bytes"] for r in b.records] == [r["bytes"] for r in sorted(a.records, key=record_key)]
    assert b.text.startswith("@HD\tVN:1.6\tSO:coordinate\n") and b.text.split("\n", 1)[1] == a.text.split("\n", 1)[1] and b.has_eof
    bai = R.Bai(got + ".bai")
    placed = check_index_structure(b, bai)
    check_region_queries(b, bai, 5, min_hits=len(placed))
    return open(got, "rb").read(), open(got + ".bai", "rb").read()


@gpu
@pytest.mark.parametrize("config", list(CLI_CONFIGS))
def test_cli_sorted_bam_and_index(tmp_path, config):
    sorted_against_plain(tmp_path, config)


@gpu
def test_cli_sorted_bam_leaves_coverage_alone(tmp_path):
    _, _ = cli(tmp_path, "a.bam", "--coverage", str(tmp_path / "a.bedgraph"))
    _, _ = cli(tmp_path, "b.bam", "--coverage", str(tmp_path / "b.bedgraph"), "--sort-by-coordinate", "--bam-index")
    a, b = open(tmp_path / "a.bedgraph", "rb").read(), open(tmp_path / "b.bedgraph", "rb").read()
    assert a == b and len(a) > 0 and os.path.exists(tmp_path / "b.bam.bai") and not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]


@gpu
def test_cli_sorted_bam_on_two_devices(tmp_path):
    if capi.lib().flx_device_count() < 2:
        pytest.skip("one HIP device: nothing to deal the batches to")
    (tmp_path / "one").mkdir()
    (tmp_path / "two").mkdir()
    assert sorted_against_plain(tmp_path / "one", "selected") == sorted_against_plain(tmp_path / "two", "selected", "--devices", "0,1")
