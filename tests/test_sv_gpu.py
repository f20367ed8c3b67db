"""Structural-variant signatures on the GPU (flx_sv): the device tables against the plain-Python rule of tests/sv_ref.py on the same
arrays, signatures and clusters byte for byte: the extract kernel's carries across every pass boundary, the junctions of groups that
straddle waves, the sort's and the scan's tile boundaries, growth, contention on one cluster and on none, the independence of the
result from how the records were added, and the calls behind finish."""
import ctypes as C
import threading

import numpy as np
import pytest

import floxer_amd as F
from floxer_amd import capi
import sv_ref as R

gpu = pytest.mark.gpu
W = R.word
LENGTHS = [1000, 3000, 4_000_000, 1500, 30_000]
BIG = 2                                                                  # (nothing is allocated per position: a long sequence costs nothing)


def device_tables(rec, words, read_lengths, o=None, adds=1, initial_capacity=0, lengths=LENGTHS):
    """(signatures, clusters) of an sv object fed with the records in `adds` calls cut at read boundaries"""
    o = o or R.options()
    s = F.sv(lengths=lengths, options=R.c_options(o, initial_capacity))
    try:
        cuts = [0] + [int(c) for c in _read_cuts(rec, adds)] + [len(rec)]
        for a, b in zip(cuts, cuts[1:]):
            s.add_records(rec[a:b], words, read_lengths)
        s.finish()
        return s.signatures(), s.clusters()
    finally:
        s.close()


def _read_cuts(rec, adds):
    """adds - 1 cut points that split no run of records with one read index"""
    if adds <= 1:
        return []
    ok = [i for i in range(1, len(rec)) if rec["read"][i] != rec["read"][i - 1]]
    return [ok[len(ok) * k // adds] for k in range(1, adds)]


def check(rec, words, read_lengths, o=None, **kw):
    o = o or R.options()
    sig, cl = device_tables(rec, words, read_lengths, o, **kw)
    want = R.signatures(rec, words, read_lengths, o)
    assert sig.tobytes() == R.signature_array(want).tobytes(), (len(sig), len(want))
    assert cl.tobytes() == R.cluster_array(R.clusters(want, o)).tobytes()
    return want


def pass_record(n_words, flag, clipped, swap, ref=BIG, pos=1000):
    """a record of exactly n_words words: single = and X columns, and a qualifying D or I word (alternating) at every word index of
    63, 64, 127, 128, 4095, 4096 that it has; clipped: its first and last words are S"""
    ws = [W("=X"[t % 2], 1) for t in range(n_words)]
    for k, t in enumerate(t for t in (63, 64, 127, 128, 4095, 4096) if t < n_words):
        ws[t] = W("DI"[(k + swap) % 2], 50 + k)
    if clipped and n_words >= 3:
        ws[0], ws[-1] = W("S", 7), W("S", 9)
    return (flag, ref, pos, 0, 0, ws)


@gpu
def test_carries_cross_every_pass_boundary():
    rows = []
    for n_words in (1, 63, 64, 65, 129, 4097):
        for flag, clipped, swap in ((0, False, 0), (16, True, 1), (2064, False, 1), (2048, True, 0)):
            rows.append(pass_record(n_words, flag, clipped, swap, pos=1000 + 7 * len(rows)))
    # 64 and 65 qualifying words in a row: one full pass of them, and one more
    for n in (64, 65):
        rows.append((0, BIG, 50_000, 0, 0, [W("DI"[t % 2], 50 + t) for t in range(n)]))
        rows.append((16, BIG, 90_000, 0, 0, [W("ID"[t % 2], 50 + t) for t in range(n)] + [W("=", 1)]))
    # the anchors and positions of the host test
    rows += [(0, 1, 500, 0, 0, [W("I", 60), W("=", 10)]), (16, 1, 500, 0, 0, [W("S", 5), W("I", 60), W("=", 10)]),
             (0, 1, 500, 0, 0, [W("=", 4), W("D", 3), W("I", 60), W("=", 10)]), (0, 1, 500, 0, 0, [W("D", 3), W("I", 60), W("=", 10)]),
             (0, 1, 500, 0, 0, [W("=", 10), W("I", 60), W("S", 7)]), (0, 0, 0, 0, 0, [W("D", 50), W("=", 10)]),
             (0, 0, 940, 0, 0, [W("=", 5), W("I", 2), W("D", 55), W("S", 3)]),
             (0, 1, 100, 0, 0, [W("=", 10), W("D", 49), W("=", 10), W("D", 50), W("=", 10), W("I", 49), W("=", 5), W("I", 50), W("=", 5)])]
    # every record is its own read: a group of one
    rows = [(f, ref, pos, i, q, ws) for i, (f, ref, pos, _, q, ws) in enumerate(rows)]
    rec, words = R.records_of(rows)
    read_lengths = [R.query_rows(r[5]) for r in rows]
    for o in (R.options(min_support=1), R.options(min_length=52, max_distance=5, min_support=1)):
        want = check(rec, words, read_lengths, o)
        assert sum(s[0] == R.DEL for s in want) > 40 and sum(s[0] == R.INS for s in want) > 40 and not any(s[0] == R.BND for s in want)
    # large coordinates on the device: ones in the high bits of pos_a and q
    big = (1 << 31) - 1
    far = big - 1100
    rows = [(0, 1, far, 0, 0, [W("=", 100), W("D", 900), W("=", 40), W("I", 70), W("=", 60)]),
            (2048, 1, 5, 0, 0, [W("S", 100), W("=", 170)]), (2064, 1, big - 170, 0, 0, [W("=", 170), W("S", 100)])] * 2
    rec, words = R.records_of([r[:3] + (i // 3,) + r[4:] for i, r in enumerate(rows)])
    want = check(rec, words, [270, 270], lengths=[1000, big])
    assert (R.BND, R.L, R.R, 1, 1, 5, big - 1) in want and len(want) == 8


@gpu
def test_junctions_of_groups_that_straddle_waves():
    rng = np.random.default_rng(11)
    rec, words, read_lengths = R.random_records(rng, LENGTHS, 400)

    def group(m, read, ref):
        return [(2048 + 16 * (k % 2) if k else 0, ref, 20 * k, read, 30, ([W("S", 5 * k)] if k else []) + [W("=", 5)] + ([W("S", 5 * (m - 1 - k))] if k < m - 1 else []))
                for k in range(m)]

    rows, extra_lengths = [], []
    for m in (1, 2, 3, 64, 63, 64, 2):
        read = len(read_lengths) + len(extra_lengths)
        g = group(m, read, 1)
        if m == 63:                                                      # a secondary, an unmapped record and a record below min_mapq inside the group
            g.insert(10, (256, 3, 50, read, 30, [W("S", 2), W("=", 5 * m - 2)]))
            g.insert(20, (4, -1, 0, read, 0, []))
            g.insert(30, (2048, 3, 100, read, 1, [W("S", 3), W("=", 5 * m - 3)]))
        rows += g
        extra_lengths.append(5 * m)
    # equal query_start values are ordered by index
    read = len(read_lengths) + len(extra_lengths)
    rows += [(0, 1, 300, read, 30, [W("S", 5), W("=", 10)]), (2048, 1, 100, read, 30, [W("S", 5), W("=", 10)]), (2048, 1, 200, read, 30, [W("=", 15)])]
    extra_lengths.append(15)
    rec2, words2 = R.records_of(rows)
    rec2["coff"] += len(words)
    rec = np.concatenate([rec[:601], rec2, rec[601:]]) if rec["read"][600] != rec["read"][601] else np.concatenate([rec, rec2])
    words = np.concatenate([words, words2])
    read_lengths = read_lengths + extra_lengths
    for o in (R.options(min_support=1), R.options(min_mapq=5, count_secondary=True, min_length=4), R.options(min_mapq=31, min_support=1)):
        want = check(rec, words, read_lengths, o)
        assert sum(s[0] == R.BND for s in want) > (300 if o["min_mapq"] < 31 else 20)


def one_del_records(positions, ref=BIG, q=None):
    """one record with one D word per position: n signatures exactly"""
    rows = [(0, ref, int(p) - 10, i, 0, [W("=", 10), W("D", 50 if q is None else int(q[i])), W("=", 10)]) for i, p in enumerate(positions)]
    rec, words = R.records_of(rows)
    return rec, words, [20] * len(rows)


@gpu
def test_sort_and_scan_boundaries():
    rng = np.random.default_rng(12)
    geometry = F.sort_geometry()
    assert geometry[0] == 2048 and geometry[3] == 4096                   # the sizes below are the sort's tile and the scan's tile
    for n in (2048, 2049, 4096, 4097):
        pos = rng.integers(10, 3_000_000, size=n)
        pos[: n // 4] = rng.integers(10, 2000, size=n // 4)              # a crowd that clusters
        rec, words, rl = one_del_records(pos, q=rng.choice([50, 60, 200, 5000], size=n))
        want = check(rec, words, rl, R.options(min_support=1 + n % 2))
        assert len(want) == n
    # a tile table of more than one scan tile: more than 16 tiles of 2048 keys
    n = 40_000
    rows = []
    for i in range(n // 100):
        ws = [W("=", 1)]
        for _ in range(100):
            ws += [W("D", int(rng.choice([50, 51, 300]))), W("=", int(rng.integers(1, 400)))]
        rows.append((0, BIG, int(rng.integers(0, 3_000_000)), i, 0, ws))
    rec, words = R.records_of(rows)
    want = check(rec, words, [R.query_rows(r[5]) for r in rows], adds=3, initial_capacity=8)      # and several growths
    assert len(want) == n
    # all keys equal: every digit is constant and no pass runs
    rec, words, rl = one_del_records([5000] * 3000)
    assert len(set(check(rec, words, rl))) == 1
    # keys that differ in the top digit only: a DEL and an INS with one reference, position and length
    rows = [(0, BIG, 4990, 2 * i, 0, [W("=", 10), W("D", 50), W("=", 10)]) for i in range(1500)] + [(0, BIG, 4991, 2 * i + 1, 0, [W("=", 10), W("I", 50), W("=", 10)]) for i in range(1500)]
    rng.shuffle(rows)
    rec, words = R.records_of(rows)
    want = check(rec, words, [R.query_rows(r[5]) for r in sorted(rows, key=lambda r: r[3])])
    assert set(want) == {(R.DEL, 0, 0, BIG, BIG, 5000, 50), (R.INS, 0, 0, BIG, BIG, 5000, 50)}
    # nothing added
    sig, cl = device_tables(rec[:0], words, [20])
    assert len(sig) == 0 and len(cl) == 0


@gpu
def test_contention_one_cluster_and_none():
    n = 20_000
    rng = np.random.default_rng(13)
    # a chain: neighbours exactly max_distance apart in pos_a, one q: one cluster of all
    rec, words, rl = one_del_records(rng.permutation(100 + 100 * np.arange(n)))
    want = check(rec, words, rl)
    cl = R.clusters(want, R.options())
    assert len(cl) == 1 and cl[0][3] == n and cl[0][6:8] == (100, 100 * n)
    # 101 apart: every signature alone
    rec, words, rl = one_del_records(rng.permutation(100 + 101 * np.arange(n)))
    want = check(rec, words, rl, R.options(min_support=1))
    assert len(R.clusters(want, R.options(min_support=1))) == n
    assert len(device_tables(rec, words, rl)[1]) == 0                    # none has the default support


@gpu
def test_the_result_does_not_depend_on_how_records_are_added():
    rng = np.random.default_rng(14)
    rec, words, read_lengths = R.random_records(rng, LENGTHS, 600)
    o = R.options(min_length=20, min_support=1)
    want = R.signatures(rec, words, read_lengths, o)
    want_sig, want_cl = R.signature_array(want).tobytes(), R.cluster_array(R.clusters(want, o)).tobytes()
    for adds in (1, 3):
        sig, cl = device_tables(rec, words, read_lengths, o, adds=adds)
        assert sig.tobytes() == want_sig and cl.tobytes() == want_cl
    cuts = [0] + _read_cuts(rec, 8) + [len(rec)]
    # eight host threads
    s = F.sv(lengths=LENGTHS, options=R.c_options(o, 8))
    errors = []

    def add(a, b):
        try:
            s.add_records(rec[a:b], words, read_lengths)
        except Exception as e:                                           # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=add, args=(a, b)) for a, b in zip(cuts, cuts[1:])]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    s.finish()
    assert s.signatures().tobytes() == want_sig and s.clusters().tobytes() == want_cl
    s.close()
    # two objects, then absorbed
    a, b = F.sv(lengths=LENGTHS, options=R.c_options(o, 8)), F.sv(lengths=LENGTHS, options=R.c_options(o))
    for k, (x, y) in enumerate(zip(cuts, cuts[1:])):
        (a if k % 2 else b).add_records(rec[x:y], words, read_lengths)
    a.absorb(b)
    b.add_records(rec[: cuts[1]], words, read_lengths)                   # `from` is left empty and usable
    a.finish()
    b.finish()
    assert a.signatures().tobytes() == want_sig and a.clusters().tobytes() == want_cl
    assert b.signatures().tobytes() == R.signature_array(R.signatures(rec[: cuts[1]], words, read_lengths, o)).tobytes()
    a.close()
    b.close()
    # different options or lengths are not absorbed
    a, b, c = F.sv(lengths=LENGTHS, options=R.c_options(o)), F.sv(lengths=LENGTHS, options=R.c_options(R.options(min_length=21, min_support=1))), F.sv(lengths=LENGTHS[:-1], options=R.c_options(o))
    for other, match in ((b, "options"), (c, "lengths"), (a, "itself")):
        with pytest.raises(F.FloxerError, match=match):
            a.absorb(other)
    for x in (a, b, c):
        x.close()


@gpu
def test_refusals_and_the_calls_behind_finish():
    rows = [(0, 1, 100, read, 0, [W("=", 10), W("D", 60), W("=", 10)]) for read in (0, 1)]
    rec, words = R.records_of(rows)
    s, t = F.sv(lengths=LENGTHS), F.sv(lengths=LENGTHS)
    s.add_records(rec, words, [20, 20])
    # refused on the host before any launch: the object stays as it was
    bad, bad_words = R.records_of(rows + [(0, 1, 100, 2, 0, [W("=", 4), W("S", 3), W("=", 13)])])
    with pytest.raises(F.FloxerError, match="both sides"):
        s.add_records(bad, bad_words, [20, 20, 20])
    with pytest.raises(F.FloxerError, match="read_index"):
        s.add_records(rec, words, [])
    # the copy calls before finish are refused
    for call in (s.signatures, s.clusters):
        with pytest.raises(F.FloxerError, match="flx_sv_finish first"):
            call()
    assert capi.lib().flx_sv_num_signatures(s.h) == 0 and capi.lib().flx_sv_num_clusters(s.h) == 0
    s.finish()
    assert R.signature_tuples(s.signatures()) == [(R.DEL, 0, 0, 1, 1, 110, 60)] * 2
    assert s.clusters().tobytes() == R.cluster_array([(R.DEL, 0, 0, 2, 1, 1, 110, 110, 60, 60, 60)]).tobytes()
    out = np.zeros(1, dtype=F.SV_CLUSTER_DTYPE)
    assert capi.lib().flx_sv_copy_clusters(s.h, out.ctypes.data_as(C.POINTER(capi.SvCluster)), 0) == -3
    sig = np.zeros(2, dtype=F.SV_SIGNATURE_DTYPE)
    assert capi.lib().flx_sv_copy_signatures(s.h, 1, 3, sig.ctypes.data_as(C.POINTER(capi.SvSignature))) == -1
    assert capi.lib().flx_sv_copy_signatures(s.h, 1, 2, sig.ctypes.data_as(C.POINTER(capi.SvSignature))) == 0 and R.signature_tuples(sig[:1]) == [(R.DEL, 0, 0, 1, 1, 110, 60)]
    # add, absorb (either way) and a second finish are refused behind finish
    for call in (lambda: s.add_records(rec, words, [20, 20]),lambda: s.absorb(t), lambda: t.absorb(s), s.finish):
        with pytest.raises(F.FloxerError, match="finished"):
            call()
    s.close()
    t.close()


# ------------------------------------------------------------------------------------------------ end to end
E2E_RATE, E2E_LEN, E2E_CHROM, DEL_AT, DEL_LEN = 0.07, 1500, 40_000, 20_000, 80
CHIM_A, CHIM_B = 5_000, 30_000                                           # where the chimeras' halves come from, on sequence 0 and on sequence 1


def _revcomp(r):
    return (5 - r[::-1]).astype(np.uint8)                                # (ranks 1..4 only)


def e2e_data():
    """two sequences of 40 000 symbols; error-free reads of 1500: five from a sample that lacks [DEL_AT, DEL_AT + 80) of sequence 0, on
    both strands and with the break at different rows; four from the reference as it is; five chimeras whose halves are the two
    children of the root of the reads' PEX tree (tests/test_partial_gpu.py has the construction: such halves are what partial
    alignment finds), the first from sequence 0 forward and the second from sequence 1 reverse, three as made and two reverse
    complemented"""
    from floxer_amd import simulate as S
    _, chroms = S.make_genome_fast(E2E_CHROM, 2, seed=51)
    sample = np.concatenate([chroms[0][:DEL_AT], chroms[0][DEL_AT + DEL_LEN:]])
    reads = []
    for k, off in enumerate((400, 600, 750, 900, 1100)):
        r = sample[DEL_AT - off: DEL_AT - off + E2E_LEN].copy()
        reads.append(_revcomp(r) if k % 2 else r)
    for k, (c, p) in enumerate(((0, 1000), (1, 2000), (0, 33_000), (1, 12_000))):
        r = chroms[c][p: p + E2E_LEN].copy()
        reads.append(_revcomp(r) if k % 2 else r)
    k = int(capi.lib().flx_floating_point_error_aware_ceil(E2E_LEN * E2E_RATE))
    t = F.pex_tree(E2E_LEN, k, 2)
    kids = sorted((nd for nd in t.inner_nodes + t.leaves if nd[0] == 0 and nd is not t.inner_nodes[0]), key=lambda nd: nd[1])
    assert len(kids) == 2 and kids[0][1] == 0 and kids[0][2] + 1 == kids[1][1] and kids[1][2] == E2E_LEN - 1
    la, lb = kids[0][2] + 1, E2E_LEN - kids[0][2] - 1
    chimera = np.concatenate([chroms[0][CHIM_A: CHIM_A + la], _revcomp(chroms[1][CHIM_B: CHIM_B + lb])])
    reads += [chimera.copy(), chimera.copy(), _revcomp(chimera), chimera.copy(), _revcomp(chimera)]
    return chroms, reads, la, lb


def e2e_aligner(ctx, mapq=True):
    return F.aligner(ctx, F.params(error_probability=E2E_RATE), F.output_options(drop_duplicates=True, max_alignments=1, mapq=mapq),
                     partial=F.partial_options(min_query_span=500), extend=F.extend_options(), realign=F.realign_options())


def e2e_raw_run(ctx, reads, mapq=True):
    """an unfreed flx_run handle made with e2e_aligner's options (tests/test_pileup_gpu.py has the pattern)"""
    run = C.c_void_p()
    p = F.params(error_probability=E2E_RATE)
    output, partial, extend, realign = F.output_options(drop_duplicates=True, max_alignments=1, mapq=mapq), F.partial_options(min_query_span=500), F.extend_options(), F.realign_options()
    bundle = capi.RunOptions()
    bundle.output, bundle.partial, bundle.extend = C.pointer(output), C.pointer(partial), C.pointer(extend)
    pool, offs, n = F._pool_and_offsets(reads)
    capi.check(capi.lib().flx_align_reads_realign(ctx.h, C.byref(p), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n, C.byref(bundle), None, None, C.byref(realign),
                                                  C.byref(run)))
    return run


def copied_records(run):
    """the records and CIGAR words of an unfreed flx_run handle, as flx_run_copy lists them"""
    L = capi.lib()
    nr, nc = L.flx_run_num_records(run), L.flx_run_num_cigar_words(run)
    raw, cig = np.zeros(max(1, nr), dtype=R.REC_DTYPE), np.zeros(max(1, nc), dtype=np.uint32)
    skipped = np.zeros(64, dtype=np.uint8)
    capi.check(L.flx_run_copy(run, raw.ctypes.data_as(C.POINTER(capi.Record)), capi.ptr(cig, capi.u32p), capi.ptr(skipped, capi.u8p)))
    return raw[:nr], cig[:nc]


@pytest.fixture(scope="module")
def e2e():
    chroms, reads, la, lb = e2e_data()
    ctx = F.context(F.fmindex(chroms))
    run = e2e_aligner(ctx).align_reads(reads)
    yield chroms, reads, la, lb, ctx, run
    ctx.close()


@gpu
def test_end_to_end_through_the_library(e2e):
    """The precondition, checked on the CPU before the shape was fixed: for the five spanning reads the oracle's edit-distance CIGAR
    against sequence 0 (k = 105 errors) has NM 80, but scatters the deletion over 19 D words of 1 to 14 columns with single matching
    columns between them (402= 9D 3= 2D 1= 3D 2= ... 8D 1081= for the first read): no word reaches 50. The affine rule of
    tests/realign_ref.py (default scores, band 16) turns each into one word: 402= 80D 1098=, 602= 80D 898=, 752= 80D 748=,
    902= 80D 598=, 1102= 80D 398=, the gap two columns right of where it was planted, among equal letters. So with realign the
    reference alone satisfies the DEL assertion below (pos_a 20 002, q 80), and without it no DEL signature would exist."""
    chroms, reads, la, lb, ctx, run = e2e
    lens = [len(r) for r in reads]
    o = R.options()
    s = F.sv(ctx, R.c_options(o))
    s.add_run(run, lens)
    s.finish()
    sig, cl = s.signatures(), s.clusters()
    s.close()
    want = R.signatures(run.raw, run.cigars, lens, o)
    assert sig.tobytes() == R.signature_array(want).tobytes()
    assert cl.tobytes() == R.cluster_array(R.clusters(want, o)).tobytes()
    dels = [c for c in cl if c["type"] == R.DEL and c["ref_a"] == 0 and abs(int(c["pos_a_min"]) - DEL_AT) <= 80 and 50 <= c["q_median"] <= 80]
    assert len(dels) == 1 and dels[0]["support"] == 5
    bnds = [c for c in cl if c["type"] == R.BND and c["ref_a"] == 0 and c["ref_b"] == 1]
    assert len(bnds) == 1 and bnds[0]["support"] == 5 and (bnds[0]["side_a"], bnds[0]["side_b"]) == (R.R, R.R)
    # (the extension runs on past the break while letters match by chance and within its error budget: the ends lie near the
    # construction's, not on them; the clustering distance is the unit that "near" has in this table)
    assert abs(int(bnds[0]["pos_a_min"]) - (CHIM_A + la - 1)) <= 100 and abs(int(bnds[0]["q_median"]) - (CHIM_B + lb - 1)) <= 100
    # min_mapq needs a run made with mapq: the Python check of a RunResult (the C call's own: test_add_run_walks_a_run_and_its_parts)
    plain = e2e_aligner(ctx, mapq=False).align_reads(reads[:2])
    with pytest.raises(F.FloxerError, match="min_mapq needs"):
        F.sv(ctx, F.sv_options(min_mapq=1)).add_run(plain, lens[:2])
    t = F.sv(ctx, F.sv_options(min_mapq=1))
    t.add_run(run, lens)
    t.finish()
    assert t.signatures().tobytes() == R.signature_array(R.signatures(run.raw, run.cigars, lens, R.options(min_mapq=1))).tobytes()
    t.close()


@gpu
def test_add_run_walks_a_run_and_its_parts(e2e, monkeypatch):
    """flx_sv_add_run itself, with raw flx_run handles: a run cut into several parts, each with its own word pool, judged as a whole
    and added piece by piece; its two refusals of a whole run, each with its message and the object as it was"""
    chroms, reads, la, lb, ctx, run = e2e
    L = capi.lib()
    lens = [len(r) for r in reads]
    monkeypatch.setenv("FLX_CHUNK_READS", "4")                           # several parts
    raw = {mapq: e2e_raw_run(ctx, reads, mapq) for mapq in (False, True)}
    monkeypatch.delenv("FLX_CHUNK_READS")
    pw = F.params(error_probability=E2E_RATE, without_cigar=True)
    bare = C.c_void_p()
    pool, offs, n = F._pool_and_offsets(reads)
    capi.check(L.flx_align_reads(ctx.h, C.byref(pw), capi.ptr(pool, capi.u8p), capi.ptr(offs, capi.u64p), n, C.byref(bare)))
    try:
        rec, words = copied_records(raw[True])
        assert R.signatures(rec, words, lens, R.options()) == R.signatures(run.raw, run.cigars, lens, R.options())      # the cut changes no signature
        for o in (R.options(), R.options(min_mapq=1, min_length=60, min_support=1)):
            want = R.signatures(rec, words, lens, o)
            assert o["min_mapq"] or {s[0] for s in want} == {R.DEL, R.BND}
            s = F.sv(ctx, R.c_options(o, 8))
            if o["min_mapq"]:                                            # a run made without mapq holds no mapping quality: refused, nothing added
                with pytest.raises(F.FloxerError, match="min_mapq needs a run made with flx_output_options.mapq"):
                    s.add_run(raw[False], lens)
            # a run made without CIGARs has no signatures (it was made without mapq too: with min_mapq that is what is said first)
            with pytest.raises(F.FloxerError, match="min_mapq needs" if o["min_mapq"] else "without_cigar"):
                s.add_run(bare, lens)
            with pytest.raises(F.FloxerError, match="read_index"):        # judged before anything is added: a later part's read lies outside
                s.add_run(raw[True], lens[:-1])
            s.add_run(raw[True], lens)
            s.finish()
            assert s.signatures().tobytes() == R.signature_array(want).tobytes()                    # the refused runs left nothing behind
            assert s.clusters().tobytes() == R.cluster_array(R.clusters(want, o)).tobytes()
            s.close()
        # without min_mapq the run made without mapq is taken, and has the same words
        rec0, words0 = copied_records(raw[False])
        s = F.sv(ctx)
        s.add_run(raw[False], lens)
        s.finish()
        assert s.signatures().tobytes() == R.signature_array(R.signatures(rec0, words0, lens, R.options())).tobytes()
        s.close()
    finally:
        for r in (raw[False], raw[True], bare):
            L.flx_run_free(r)


@gpu
def test_end_to_end_through_the_cli(e2e, tmp_path):
    import os
    import subprocess
    chroms, reads, la, lb, ctx, run = e2e
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    letters = lambda r: "".join("$ACGTN"[x] for x in r)
    fasta, fastq = str(tmp_path / "ref.fasta"), str(tmp_path / "reads.fastq")
    with open(fasta, "w") as f:
        for i, c in enumerate(chroms):
            f.write(f">chr{i}\n" + "\n".join(letters(c[o: o + 100]) for o in range(0, len(c), 100)) + "\n")
    with open(fastq, "w") as f:
        for i, r in enumerate(reads):
            f.write(f"@read{i}\n{letters(r)}\n+\n{'I' * len(r)}\n")
    base = [os.path.join(root, "floxer_amd", "floxer"), "--reference", fasta, "--queries", fastq, "--error-probability", str(E2E_RATE), "--threads", "2",
            "--partial-alignments", "--partial-min-span", "500", "--partial-extend", "--realign-affine", "-Q", "-N", "1"]

    def cli(out, *extra):
        r = subprocess.run(base + ["--output", str(tmp_path / out)] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        return r.stderr.decode()

    tsv = str(tmp_path / "sv.tsv")
    log = cli("with.sam", "-D", "--sv-signatures", tsv)
    assert "counts records, not reads" not in log
    s = F.sv(ctx)
    s.add_run(run, [len(r) for r in reads])
    s.finish()
    want = R.tsv_lines(s.clusters(), ["chr0", "chr1"])
    s.close()
    assert len(want) >= 2 and open(tsv).read().splitlines() == want
    cli("without.sam", "-D")
    assert open(tmp_path / "with.sam", "rb").read() == open(tmp_path / "without.sam", "rb").read()
    assert "counts records, not reads" in cli("dups.sam", "--sv-signatures", str(tmp_path / "dups.tsv"))
