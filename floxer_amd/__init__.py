"""floxer_amd — MI355X-native seed-and-verify path of the floxer long-read aligner.

Python mirror of the reference's interfaces for the hot path (same names, argument meaning, error behaviour), over the C ABI of
libfloxer_amd.so:

    pex_tree(config)                       pex::pex_tree            (pex.hpp:57-126)
    fmindex(references)                    fmindex(refs, 4, threads) (floxer.cpp:93-97)
    searcher(ctx, config).search_seeds()   search::searcher         (search.hpp:104-112)
    align(reference, query, config)        alignment::align         (alignment.hpp:73-77), batched as align_batch
    aligner(ctx, params).align_reads()     spawn_search_task + query_verifier::verify + write_alignments_for_query
    output_options(...), select_records()  not floxer's: duplicate alignments dropped / alignments per read capped (opt-in)
    output_options(mapq=True), assign_mapq()  not floxer's: mapping quality from a read's distinct loci (opt-in)
    aligner(..., md=True), align(..., md=True)  not floxer's: MD strings, built on the device next to the CIGARs (opt-in)
    aligner(..., partial=partial_options())   not floxer's: soft-clipped partial alignments of reads without a full one (opt-in)
    aligner(..., extend=extend_options()), extend_batch()  not floxer's: the partial records' ends extended to the break (opt-in)
    aligner(..., split=split_options()), cigar_tails()  not floxer's: reads mapped in full that carry a chimeric tail are split (opt-in)
    aligner(..., gaps=gap_options()), left_align()  not floxer's: indels left-aligned on the device behind the traceback (opt-in)
    aligner(..., realign=realign_options()), realign(), realign_batch(), align_batch_realign()  not floxer's: a traced path realigned under affine gap costs inside a band around it (opt-in)
    aligner(..., cs=cs_options()), cs_string(), cs_batch(), align_batch_cs()  not floxer's: minimap2's cs difference string, short or long form, built on the device behind the MD strings (opt-in)
    coverage(ctx, coverage_options()), coverage_host()  not floxer's: depth of coverage accumulated on the device from the records of runs: equal-depth runs, per-window sums (opt-in)
    pileup(ctx, pileup_options()), pileup_host(), pileup_sites_host()  not floxer's: per-position allele counts (depth, mismatch letters, deletions, insertions) accumulated on the device from the records of runs, and the table of candidate variant sites (opt-in)
    sv(ctx, sv_options()), sv_host(), sv_clusters_host()  not floxer's: structural-variant signatures (long deletions, long insertions, split junctions) collected on the device from the records of runs, sorted and merged into clusters with their support (opt-in)
    svcaller(ctx, svcall_options()), svcall_host(), svcaller_geometry()  not floxer's: the DEL and INS clusters of an sv object genotyped from the records of the same runs (how many records span a cluster's locus, counted on the device over the sorted spans), as rows with GT, GQ, QUAL and PL; device=-1 is the host form (opt-in)
    errprof(ctx, errprof_options()), errprof_host()  not floxer's: the error profile of the records of runs (which letter is read as which, indel lengths and homopolymer context, errors by position in the read, identities, error-free stretches), summed on the device (opt-in)
    grid_caps()                           a test hook: the most blocks each capped launch asks for, by kernel name
    record_sorter(n_refs), sort_host(), sort_geometry()  not floxer's: the coordinate order of records (reference, position, strand, then the caller's ordinal), sorted on the device by a radix sort over 128-bit keys (opt-in)

The compute runs in hand-written HIP kernels; nothing here falls back to a CPU implementation.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import FloxerError, check, lib, ptr, as_u8, u8p, u32p, u64p

# The library asks the HIP runtime for its hardware queues when it is loaded (hw_queue_request below), and the runtime reads the request
# when it initialises, with the process's first HIP call. So the library is loaded with the package, not by the first call into it: a
# program that imports torch, imports this package and only then touches the GPU gets the request in time. (A library that is not built
# stays the error of the first call that needs it.)
if capi.os.path.exists(capi.LIB_PATH):
    lib()

CIGAR_OPS = "MIDNSHP=X"
NULL_ID = 0xFFFFFFFF

ORDER = {"errors_first": 0, "count_first": 1, "none": 2}          # search.cpp:59-69
CHOICE = {"round_robin": 0, "full_groups": 1, "first_reported": 2}  # search.cpp:71-81
MODE_EXISTS, MODE_WITHOUT_CIGAR, MODE_WITH_CIGAR = 0, 1, 2


def hw_queue_request():
    """(requested, found): the GPU_MAX_HW_QUEUES the library wrote when it was loaded (FLX_HW_QUEUES, default 16, 4 .. 32; 0 when
    FLX_HW_QUEUES=0 made it leave the variable alone) and the value it found there (-1: the variable was unset)"""
    requested, found = C.c_int(0), C.c_int(-1)
    check(lib().flx_hw_queue_request(C.byref(requested), C.byref(found)))
    return requested.value, found.value


def cigar_string(words):
    return "".join(f"{int(w) >> 4}{CIGAR_OPS[int(w) & 15]}" for w in words)


# ------------------------------------------------------------------------------------------------ math / input
def ceil_div(a, b):
    return lib().flx_ceil_div(a, b)


def floating_point_error_aware_ceil(v):
    return lib().flx_floating_point_error_aware_ceil(float(v))


def saturate_value_to_int32_max(v):
    return lib().flx_saturate_value_to_int32_max(v)


def chars_to_rank_sequence(s):
    b = s.encode() if isinstance(s, str) else bytes(s)
    out = np.zeros(len(b), dtype=np.uint8)
    lib().flx_chars_to_rank_sequence(b, len(b), ptr(out, u8p))
    return out


def reverse_complement_rank(r):
    r = as_u8(r)
    out = np.zeros_like(r)
    lib().flx_reverse_complement_rank(ptr(r, u8p), len(r), ptr(out, u8p))
    return out


# ------------------------------------------------------------------------------------------------ PEX tree
class pex_tree:
    """pex::pex_tree built from (total_query_length, query_num_errors, leaf_max_num_errors, build_strategy)."""

    def __init__(self, total_query_length, query_num_errors, leaf_max_num_errors, bottom_up=False):
        cap = 4 * (query_num_errors + 2) + 16
        nodes = (capi.PexNode * cap)()
        ni, nl = C.c_uint64(), C.c_uint64()
        check(lib().flx_pex_tree_build(total_query_length, query_num_errors, leaf_max_num_errors, int(bottom_up), nodes, cap,
                                       C.byref(ni), C.byref(nl)))
        rows = [(n.parent_id, n.from_, n.to, n.num_errors) for n in nodes[: ni.value + nl.value]]
        self.inner_nodes = rows[: ni.value]
        self.leaves = rows[ni.value:]

    def root(self):
        return self.inner_nodes[0] if self.inner_nodes else self.leaves[0]

    def get_leaves(self):
        return self.leaves

    def generate_seeds(self, step=1):
        """[(offset, length, num_errors, pex_leaf_index)] as pex_tree::generate_seeds (pex.cpp:258-277)."""
        return [(l[1], l[2] - l[1] + 1, l[3], i) for i, l in enumerate(self.leaves)][::step]


# ------------------------------------------------------------------------------------------------ index + context
class fmindex:
    def __init__(self, references=None, path=None, device=None):
        """device: HIP device ordinal to build the suffix arrays on (None: on the host, as flx_index_build)"""
        self.h = C.c_void_p()
        if path is not None and references is None:
            check(lib().flx_index_load(path.encode(), C.byref(self.h)))
        else:
            refs = [as_u8(r) for r in references]
            pool = np.concatenate(refs) if refs else np.zeros(0, np.uint8)
            lens = np.array([len(r) for r in refs], dtype=np.uint64)
            if device is None:
                check(lib().flx_index_build(ptr(pool, u8p), ptr(lens, u64p), len(refs), C.byref(self.h)))
            else:
                check(lib().flx_index_build_on_device(int(device), ptr(pool, u8p), ptr(lens, u64p), len(refs), C.byref(self.h)))

    def save(self, path):
        check(lib().flx_index_save(self.h, path.encode()))

    # ---- the index as an HBM image + a small host part: how a job replicates it across its GPUs (floxer_amd/distributed.py)
    def meta(self):
        n = C.c_uint64(0)
        lib().flx_index_meta_export(self.h, None, C.byref(n))
        buf = np.zeros(n.value, dtype=np.uint8)
        check(lib().flx_index_meta_export(self.h, ptr(buf, u8p), C.byref(n)))
        return buf.tobytes()

    @classmethod
    def from_meta(cls, meta):
        """an index without arrays (sequence starts / lengths and symbol counts only): for context(index, image=...)"""
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        buf = np.frombuffer(meta, dtype=np.uint8).copy()
        check(lib().flx_index_meta_import(ptr(buf, u8p), len(buf), C.byref(self.h)))
        return self

    def image_layout(self):
        """bytes of the five device buffers of the index's HBM image"""
        out = np.zeros(5, dtype=np.uint64)
        check(lib().flx_index_image_layout(self.h, ptr(out, u64p)))
        return [int(x) for x in out]

    def image_upload(self, device, pointers):
        arr = (C.c_void_p * 5)(*[C.c_void_p(int(p)) for p in pointers])
        check(lib().flx_index_image_upload(self.h, int(device), arr))

    def __del__(self):
        if getattr(self, "h", None):
            lib().flx_index_free(self.h)
            self.h = None

    @property
    def text_length(self):
        return lib().flx_index_text_length(self.h)

    @property
    def num_references(self):
        return lib().flx_index_num_references(self.h)

    @property
    def device_bytes(self):
        return lib().flx_index_device_bytes(self.h)

    @property
    def derived_device_bytes(self):
        """inverse suffix array + presence filter a context adds to the image when the device has room"""
        return lib().flx_index_derived_device_bytes(self.h)

    def suffix_array(self):
        out = np.zeros(self.text_length, dtype=np.uint64)
        check(lib().flx_index_copy_sa(self.h, ptr(out, u64p)))
        return out

    def suffix_array_u32(self):
        out = np.empty(self.text_length, dtype=np.uint32)
        check(lib().flx_index_copy_sa_u32(self.h, ptr(out, u32p)))
        return out

    def bwt(self, reversed_text=False):
        out = np.zeros(self.text_length, dtype=np.uint8)
        check(lib().flx_index_copy_bwt(self.h, int(reversed_text), ptr(out, u8p)))
        return out


class context:
    """One HIP device + stream + HBM-resident index."""

    def __init__(self, index, device=0, image=None):
        """image: five device buffers holding the index's HBM image (objects with data_ptr(), e.g. torch uint8 tensors; kept alive by
        this object), as uploaded by fmindex.image_upload or received from another rank; None: the context uploads its own."""
        self.index = index
        self.image = image
        self.h = C.c_void_p()
        if image is None:
            check(lib().flx_ctx_create(device, index.h, C.byref(self.h)))
        else:
            arr = (C.c_void_p * 5)(*[C.c_void_p(int(b.data_ptr())) for b in image])
            sizes = np.array([int(b.numel()) * int(b.element_size()) for b in image], dtype=np.uint64)      # what the buffers hold: checked against the layout
            check(lib().flx_ctx_create_on_image(device, index.h, arr, ptr(sizes, u64p), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().flx_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def set_stream(self, hip_stream):
        check(lib().flx_ctx_set_stream(self.h, hip_stream))

    def enable_kernel_timing(self, on=True):
        check(lib().flx_ctx_enable_kernel_timing(self.h, int(on)))

    def reset_kernel_stats(self):
        check(lib().flx_ctx_reset_kernel_stats(self.h))

    def path_counters(self, reset=False):
        """seeds / anchors / requested DP work of all batches since the context was made (or the counters were reset)"""
        pc = capi.PathCounters()
        check(lib().flx_ctx_get_path_counters(self.h, C.byref(pc)))
        if reset:
            check(lib().flx_ctx_reset_path_counters(self.h))
        out = {n: int(getattr(pc, n)) for n, _ in capi.PathCounters._fields_ if n != "reserved"}
        out["records_dropped"] = int(pc.reserved[0])          # records that output options left out (records: those written)
        out["partial_records"] = int(pc.reserved[1])          # records of partial alignments written (partial_options), and
        out["reads_rescued"] = int(pc.reserved[2])            # the reads that got them in place of their unmapped record
        out["reads_split"] = int(pc.reserved[3])              # the reads mapped in full that split_options split at a chimeric tail
        return out

    def search_counters(self):
        """what the search kernel's work sharing did, over all search launches since the context was made (or path_counters(reset=True)):
        launches, subtrees_queued, lane_handovers, wave_handovers, walks_abandoned"""
        sc = capi.SearchCounters()
        check(lib().flx_ctx_get_search_counters(self.h, C.byref(sc)))
        return {n: int(getattr(sc, n)) for n, _ in capi.SearchCounters._fields_ if n != "reserved"}

    def derived_info(self):
        """the tables the context derived from its image when it was made (flx_ctx_derived_info, a test hook): filter_k, filter_tmin,
        have_isa, have_filter, have_filter_mirrored"""
        di = capi.DerivedInfo()
        check(lib().flx_ctx_derived_info(self.h, C.byref(di)))
        return {n: int(getattr(di, n)) for n, _ in capi.DerivedInfo._fields_ if n != "reserved"}

    def copy_derived(self, which):
        """one derived table read back from HBM (flx_ctx_copy_derived, a test hook): "isa" the inverse suffix array (uint32 per text
        symbol), "filter" / "filter_mirrored" the presence filter's uint64 words. Raises FloxerError for a table the context has not."""
        if which == "isa":
            out = np.empty(self.index.text_length, dtype=np.uint32)
        else:
            out = np.empty((4 ** self.derived_info()["filter_k"] + 63) // 64, dtype=np.uint64)
        check(lib().flx_ctx_copy_derived(self.h, {"isa": 0, "filter": 1, "filter_mirrored": 2}[which], out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def lane_overlap(self, n_lanes, iterations):
        """(start_ms, stop_ms), two lists of n_lanes floats (flx_ctx_lane_overlap, a test hook): one one-wave kernel of `iterations`
        dependent steps on each of the first n_lanes lanes' streams; when each started and stopped, behind one reference event"""
        start, stop = (C.c_float * n_lanes)(), (C.c_float * n_lanes)()
        check(lib().flx_ctx_lane_overlap(self.h, n_lanes, iterations, start, stop))
        return list(start), list(stop)

    def kernel_stats(self):
        arr = (capi.KernelStat * 64)()
        n = C.c_uint32(64)
        check(lib().flx_ctx_get_kernel_stats(self.h, arr, C.byref(n)))
        return {a.name.decode(): dict(launches=a.launches, device_ms=a.device_ms, algorithmic_bytes=a.algorithmic_bytes,
                                      work_units=a.work_units) for a in arr[: n.value]}


class statistics:
    """statistics::search_and_alignment_statistics (statistics.hpp:24-172): attach to a context, align, read the TOML / terminal text"""

    def __init__(self, input_hint=None):
        self.h = C.c_void_p()
        check(lib().flx_stats_create(input_hint.encode() if input_hint else None, C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            lib().flx_stats_free(self.h)
            self.h = None

    def attach(self, ctx):
        check(lib().flx_ctx_set_stats(ctx.h, self.h))
        return self

    @property
    def num_queries(self):
        return lib().flx_stats_num_queries(self.h)

    def format(self, toml=True):
        n = C.c_uint64(0)
        lib().flx_stats_format(self.h, int(toml), None, C.byref(n))
        buf = C.create_string_buffer(n.value)
        check(lib().flx_stats_format(self.h, int(toml), buf, C.byref(n)))
        return buf.value.decode()


# ------------------------------------------------------------------------------------------------ seam 1: searcher
def search_config(max_num_anchors_hard=500, max_num_anchors_soft=50, anchor_group_order="count_first",
                  anchor_choice_strategy="round_robin", erase_useless_anchors=True):
    return capi.SearchConfig(max_num_anchors_hard, max_num_anchors_soft, ORDER[anchor_group_order], CHOICE[anchor_choice_strategy],
                             int(erase_useless_anchors), 0)


class searcher:
    def __init__(self, ctx, config=None):
        self.ctx = ctx
        self.config = config or search_config()

    def _seeds(self, seeds):
        arr = (capi.Seed * len(seeds))()
        for i, (off, ln, err, leaf) in enumerate(seeds):
            arr[i] = capi.Seed(off, ln, err, leaf, 0)
        return arr

    def search_seeds(self, sequence, seeds):
        """seeds: [(offset, length, num_errors, pex_leaf_index)]. Returns (anchors, stats): anchors as an (n,5) uint64 array
        {seed_index, pex_leaf_index, reference_id, reference_position, num_errors} in anchor_iterator order; stats (n_seeds,4)
        {kept_useful, kept_raw, excluded_by_soft_cap, fully_excluded}."""
        seq = as_u8(sequence)
        arr = self._seeds(seeds)
        cap = max(64, len(seeds) * (self.config.max_num_anchors_soft + 1))
        out = (capi.Anchor * cap)()
        n = C.c_uint64(cap)
        stats = (capi.SeedStats * max(1, len(seeds)))()
        check(lib().flx_search_seeds(self.ctx.h, ptr(seq, u8p), len(seq), arr, len(seeds), C.byref(self.config), out, C.byref(n), stats))
        anchors = np.array([(a.seed_index, a.pex_leaf_index, a.reference_id, a.reference_position, a.num_errors) for a in out[: n.value]],
                           dtype=np.uint64).reshape(-1, 5)
        st = np.array([(s.num_kept_useful_anchors, s.num_kept_raw_anchors, s.num_excluded_raw_anchors_by_soft_cap, s.fully_excluded)
                       for s in stats[: len(seeds)]], dtype=np.uint64).reshape(-1, 4)
        return anchors, st

    def search_groups(self, sequence, seeds, max_hits=501):
        """raw search_n emission (kernel K1): (n,4) {seed_index, lb, len, errors} per seed in delegate order."""
        seq = as_u8(sequence)
        arr = self._seeds(seeds)
        cap = 1 << 16
        while True:
            out = (capi.HitGroup * cap)()
            n = C.c_uint64(cap)
            rc = lib().flx_search_groups(self.ctx.h, ptr(seq, u8p), len(seq), arr, len(seeds), max_hits, out, C.byref(n))
            if rc == -3:
                cap = n.value
                continue
            check(rc)
            break
        return np.array([(g.seed_index, g.lb, g.len, g.num_errors) for g in out[: n.value]], dtype=np.uint64).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------ seam 2: align
def align_batch(ctx, query_pool, jobs, reference_pool=None, md=False, gaps=None):
    """jobs: [(ref_offset, ref_length, query_offset, query_length, num_allowed_errors, mode)]. reference_pool None = the context's
    reference text (offsets are then positions in the padded concatenated text). Returns a list of None | (nm, begin, cigar);
    md=True (flx_align_batch_md): None | (nm, begin, cigar, md) with md the MD string as bytes, None for a job without CIGAR.
    gaps: gap_options(...) (flx_align_batch_gaps): the traced paths' gaps left-aligned before the MD strings are built; None: the
    calls above, unchanged."""
    q = as_u8(query_pool)
    arr = (capi.AlignJob * max(1, len(jobs)))()
    cap_words = 16
    for i, (ro, rl, qo, ql, k, mode) in enumerate(jobs):
        arr[i] = capi.AlignJob(ro, qo, rl, ql, k, mode)
        cap_words += 2 * k + 2
    res = (capi.AlignResult * max(1, len(jobs)))()
    cig = np.zeros(cap_words, dtype=np.uint32)
    words = C.c_uint64(cap_words)
    if reference_pool is None:
        rp, rl_ = None, 0
    else:
        ref = as_u8(reference_pool)
        rp, rl_ = ptr(ref, u8p), len(ref)
    if md:
        cap_md = 16 + sum(8 * k + 6 for (_, _, _, _, k, mode) in jobs if mode == MODE_WITH_CIGAR)
        refs = (capi.MdRef * max(1, len(jobs)))()
        mdp = np.zeros(cap_md, dtype=np.uint8)
        md_bytes = C.c_uint64(cap_md)
        if gaps is not None:
            check(lib().flx_align_batch_gaps(ctx.h, rp, rl_, ptr(q, u8p), len(q), arr, len(jobs), res, ptr(cig, u32p), C.byref(words),
                                             refs, ptr(mdp, u8p), C.byref(md_bytes), C.byref(gaps)))
        else:
            check(lib().flx_align_batch_md(ctx.h, rp, rl_, ptr(q, u8p), len(q), arr, len(jobs), res, ptr(cig, u32p), C.byref(words),
                                           refs, ptr(mdp, u8p), C.byref(md_bytes)))
        out = []
        for r, m in zip(res[: len(jobs)], refs[: len(jobs)]):
            out.append((r.num_errors, r.begin, cigar_string(cig[r.cigar_offset: r.cigar_offset + r.cigar_length]),
                        mdp[m.offset: m.offset + m.length].tobytes() if m.length else None) if r.exists else None)
        return out
    if gaps is not None:
        check(lib().flx_align_batch_gaps(ctx.h, rp, rl_, ptr(q, u8p), len(q), arr, len(jobs), res, ptr(cig, u32p), C.byref(words),
                                         None, None, None, C.byref(gaps)))
    else:
        check(lib().flx_align_batch(ctx.h, rp, rl_, ptr(q, u8p), len(q), arr, len(jobs), res, ptr(cig, u32p), C.byref(words)))
    out = []
    for r in res[: len(jobs)]:
        out.append((r.num_errors, r.begin, cigar_string(cig[r.cigar_offset: r.cigar_offset + r.cigar_length])) if r.exists else None)
    return out


def _realign_room(options):
    """(words, MD bytes) that the realigned path of an input with nm errors holds at most, as functions of nm: realign_cap and
    realign_nm_bound of floxer_amd/csrc/flx_realign.hpp, the one place where Python sizes a buffer for a realigned path (a call that
    needs more still says so with FLX_ERR_CAPACITY). options None or without enable: an edit path's 2 nm + 2 words and 8 nm + 6 bytes."""
    if options is None or not options.enable:
        return (lambda nm: 2 * nm + 2), (lambda nm: 8 * nm + 6)
    sc = {k: int(getattr(options, k)) or v for k, v in REALIGN_DEFAULTS.items()}
    c_max = max(sc["match"] + sc["mismatch"], sc["gap_open"] + sc["gap_extend"] + sc["match"])
    c_min = min(sc["match"] + sc["mismatch"], sc["gap_open"] + sc["gap_extend"])
    col_min = min(sc["match"] + sc["mismatch"], sc["gap_extend"])
    return (lambda nm: max(2 * nm + 2, 2 * (nm * c_max // c_min) + 1)), (lambda nm: 8 * (nm * c_max // col_min) + 6)


def align_batch_realign(ctx, query_pool, jobs, realign, reference_pool=None, md=False, gaps=None):
    """flx_align_batch_realign: align_batch with every traced path realigned under affine gap costs behind the traceback
    (realign = realign_options(...)), then left-aligned (gaps = gap_options(...)) and its MD string built (md=True) from the realigned
    words. Returns a list of None | (num_errors, begin, cigar, md or None, score)."""
    q = as_u8(query_pool)
    arr = (capi.AlignJob * max(1, len(jobs)))()
    cap_words = cap_md = 16
    room_words, room_md = _realign_room(realign)
    for i, (ro, rl, qo, ql, k, mode) in enumerate(jobs):
        arr[i] = capi.AlignJob(ro, qo, rl, ql, k, mode)
        cap_words += room_words(k)
        cap_md += room_md(k)
    res = (capi.AlignResult * max(1, len(jobs)))()
    cig = np.zeros(cap_words, dtype=np.uint32)
    words = C.c_uint64(cap_words)
    if reference_pool is None:
        rp, rl_ = None, 0
    else:
        ref = as_u8(reference_pool)
        rp, rl_ = ptr(ref, u8p), len(ref)
    refs = (capi.MdRef * max(1, len(jobs)))() if md else None
    mdp = np.zeros(cap_md if md else 1, dtype=np.uint8)
    md_bytes = C.c_uint64(cap_md)
    scores = np.zeros(max(1, len(jobs)), dtype=np.int32)
    check(lib().flx_align_batch_realign(ctx.h, rp, rl_, ptr(q, u8p), len(q), arr, len(jobs), res, ptr(cig, u32p), C.byref(words), refs,
                                        ptr(mdp, u8p) if md else None, C.byref(md_bytes) if md else None, C.byref(gaps) if gaps is not None else None,
                                        C.byref(realign) if realign is not None else None, scores.ctypes.data_as(C.POINTER(C.c_int32))))
    out = []
    for i, r in enumerate(res[: len(jobs)]):
        m = refs[i] if md else None
        out.append((r.num_errors, r.begin, cigar_string(cig[r.cigar_offset: r.cigar_offset + r.cigar_length]),
                    mdp[m.offset: m.offset + m.length].tobytes() if m is not None and m.length else None, int(scores[i])) if r.exists else None)
    return out


def align_batch_cs(ctx, query_pool, jobs, cs, reference_pool=None, md=False, gaps=None, realign=None):
    """flx_align_batch_cs: align_batch_realign with the cs string of every traced path (cs = cs_options(...)), read off the final words
    (realigned, then left-aligned) behind the MD strings. Returns a list of None | (num_errors, begin, cigar, md or None, score, cs or
    None), the strings as bytes; cs None or cs_options with form 0: no strings (flx_align_batch_realign's results)."""
    q = as_u8(query_pool)
    arr = (capi.AlignJob * max(1, len(jobs)))()
    cap_words = cap_md = cap_cs = 16
    room_words, room_md = _realign_room(realign)
    form = int(cs.form) if cs is not None else 0
    for i, (ro, rl, qo, ql, k, mode) in enumerate(jobs):
        arr[i] = capi.AlignJob(ro, qo, rl, ql, k, mode)
        cap_words += room_words(k)
        cap_md += room_md(k)
        nm = (room_md(k) - 6) // 8                 # the NM that sizes the MD slab sizes the cs slab (cs_slab_bytes, flx_internal.hpp)
        cap_cs += ql + 3 * nm + 1 if form == 2 else 10 * nm + 7
    res = (capi.AlignResult * max(1, len(jobs)))()
    cig = np.zeros(cap_words, dtype=np.uint32)
    words = C.c_uint64(cap_words)
    if reference_pool is None:
        rp, rl_ = None, 0
    else:
        ref = as_u8(reference_pool)
        rp, rl_ = ptr(ref, u8p), len(ref)
    refs = (capi.MdRef * max(1, len(jobs)))() if md else None
    mdp = np.zeros(cap_md if md else 1, dtype=np.uint8)
    md_bytes = C.c_uint64(cap_md)
    scores = np.zeros(max(1, len(jobs)), dtype=np.int32)
    cs_refs = (capi.MdRef * max(1, len(jobs)))()
    csp = np.zeros(cap_cs, dtype=np.uint8)
    cs_bytes = C.c_uint64(cap_cs)
    check(lib().flx_align_batch_cs(ctx.h, rp, rl_, ptr(q, u8p), len(q), arr, len(jobs), res, ptr(cig, u32p), C.byref(words), refs,
                                   ptr(mdp, u8p) if md else None, C.byref(md_bytes) if md else None, C.byref(gaps) if gaps is not None else None,
                                   C.byref(realign) if realign is not None else None, scores.ctypes.data_as(C.POINTER(C.c_int32)),
                                   C.byref(cs) if cs is not None else None, cs_refs, ptr(csp, u8p), C.byref(cs_bytes)))
    out = []
    for i, r in enumerate(res[: len(jobs)]):
        m = refs[i] if md else None
        c = cs_refs[i] if form else None
        out.append((r.num_errors, r.begin, cigar_string(cig[r.cigar_offset: r.cigar_offset + r.cigar_length]),
                    mdp[m.offset: m.offset + m.length].tobytes() if m is not None and m.length else None, int(scores[i]),
                    csp[c.offset: c.offset + c.length].tobytes() if c is not None and c.length else None) if r.exists else None)
    return out


def align_shapes(jobs):
    """the launch shape align_batch would give every job of a call with these jobs (flx_align_shapes; no context, no GPU):
    [(words_per_lane, lanes_per_job, queue)], queue = the hand-over slots the job's ring occupies, 0 for a ring that never waits."""
    arr = (capi.AlignJob * max(1, len(jobs)))()
    for i, (ro, rl, qo, ql, k, mode) in enumerate(jobs):
        arr[i] = capi.AlignJob(ro, qo, rl, ql, k, mode)
    out = (capi.AlignShape * max(1, len(jobs)))()
    check(lib().flx_align_shapes(arr, len(jobs), out))
    return [(s.words_per_lane, s.lanes_per_job, s.queue) for s in out[: len(jobs)]]


def align(ctx, reference, query, num_allowed_errors, mode=MODE_WITH_CIGAR, md=False):
    """alignment::align for one (reference window, query) pair; md=True adds the MD string (see align_batch)."""
    return align_batch(ctx, query, [(0, len(reference), 0, len(query), num_allowed_errors, mode)], reference_pool=reference, md=md)[0]


# ------------------------------------------------------------------------------------------------ seam 3: whole path
def params(error_probability=None, query_errors=None, seed_errors=2, max_anchors_hard=500, max_anchors_soft=50,
           anchor_group_order="count_first", anchor_choice_strategy="round_robin", seed_sampling_step_size=1,
           dont_erase_useless_anchors=False, bottom_up_pex_tree=False, interval_optimization=False,
           extra_verification_ratio=0.05, direct_full_verification=False, num_anchors_per_task=3000, without_cigar=False):
    """cli::command_line_input defaults (floxer_cli.hpp:41-70); one of error_probability / query_errors is required."""
    if error_probability is None and query_errors is None:
        raise FloxerError("Either a fixed number of errors in the query or an error probability must be given.")   # floxer_cli.cpp:174
    p = capi.Params()
    lib().flx_params_default(C.byref(p))
    p.query_error_probability = -1.0 if error_probability is None else float(error_probability)
    p.query_num_errors = 0 if query_errors is None else int(query_errors)
    p.pex_seed_num_errors = seed_errors
    p.search = search_config(max_anchors_hard, max_anchors_soft, anchor_group_order, anchor_choice_strategy, not dont_erase_useless_anchors)
    p.seed_sampling_step_size = seed_sampling_step_size
    p.bottom_up_pex_tree_building = int(bottom_up_pex_tree)
    p.use_interval_optimization = int(interval_optimization)
    p.extra_verification_ratio = extra_verification_ratio
    p.direct_full_verification = int(direct_full_verification)
    p.without_cigar = int(without_cigar)
    p.num_anchors_per_verification_task = num_anchors_per_task
    return p


class RunResult:
    """records of one flx_align_reads* call. `raw` is the flx_record array as the C ABI returns it; `rows` is the same as an (n,7)
    int64 matrix {read_index, flag, ref_id, pos, nm, cigar_off, cigar_len}, made on first use. A run made with md=True also has
    `md_refs` ((n,2) uint64 {offset, length} into `md_bytes`) and `md`, a list of bytes / None per record, made on first use; a run
    made with cs=cs_options(...) has `cs_refs`, `cs_bytes` and `cs` in the same way."""

    def __init__(self, raw, cigars, skipped, md_refs=None, md_bytes=None, scores=None, cs_refs=None, cs_bytes=None, has_mapq=None):
        self.has_mapq = has_mapq        # the run was made with output_options(mapq=True): `mapq` holds mapping qualities (None: unknown, a result not made by an aligner)
        self.cs_refs = cs_refs
        self.cs_bytes = cs_bytes
        self._cs = None
        self.scores = scores            # int32 per record (flx_run_copy_scores) of a run made with realign=realign_options(...), else None
        self.raw = raw
        self.cigars = cigars
        self.skipped = skipped
        self.md_refs = md_refs
        self.md_bytes = md_bytes
        self._rows = None
        self._md = None

    @property
    def md(self):
        """the records' MD strings (bytes; None for a record without one); None for a run made without md=True"""
        if self.md_refs is None:
            return None
        if self._md is None:
            buf = self.md_bytes.tobytes()
            self._md = [buf[int(o): int(o) + int(n)] if n else None for o, n in self.md_refs]
        return self._md

    @property
    def cs(self):
        """the records' cs strings (bytes; None for a record without one); None for a run made without cs=cs_options(...)"""
        if self.cs_refs is None:
            return None
        if self._cs is None:
            buf = self.cs_bytes.tobytes()
            self._cs = [buf[int(o): int(o) + int(n)] if n else None for o, n in self.cs_refs]
        return self._cs

    @property
    def n_records(self):
        return len(self.raw)

    @property
    def rows(self):
        if self._rows is None:
            raw = self.raw
            self._rows = (np.stack([raw["read"].astype(np.int64), raw["flag"].astype(np.int64), raw["ref"].astype(np.int64),
                                    raw["pos"].astype(np.int64), raw["nm"].astype(np.int64), raw["coff"].astype(np.int64),
                                    raw["clen"].astype(np.int64)], axis=1) if len(raw) else np.zeros((0, 7), dtype=np.int64))
        return self._rows

    @property
    def mapq(self):
        """flx_record.reserved of every record: its mapping quality when the run was made with output_options(mapq=True), else 0"""
        return self.raw["res"].astype(np.int64)

    def records(self):
        return [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), cigar_string(self.cigars[r[5]: r[5] + r[6]])) for r in self.rows]

    @property
    def clips(self):
        """(n,2) int64 {leading, trailing} soft-clipped bases of every record, read off its CIGAR in the orientation SAM stores; not 0
        only in the partial records of a run made with partial_options(...)"""
        out = np.zeros((len(self.rows), 2), dtype=np.int64)
        for i, r in enumerate(self.rows):
            if r[6]:
                first, last = int(self.cigars[r[5]]), int(self.cigars[r[5] + r[6] - 1])
                out[i, 0] = first >> 4 if first & 15 == 4 else 0
                out[i, 1] = last >> 4 if last & 15 == 4 and r[6] > 1 else 0
        return out

    def query_intervals(self, read_lengths):
        """(n,2) int64 inclusive {from, to} of every mapped record's aligned part in read-forward coordinates ((-1,-1) for an unmapped
        record or one without CIGAR): the clips turned round for the reverse strand"""
        out = np.full((len(self.rows), 2), -1, dtype=np.int64)
        for i, (r, (lead, trail)) in enumerate(zip(self.rows, self.clips)):
            if r[6] and not r[1] & 4:
                n = int(read_lengths[r[0]])
                out[i] = (trail, n - 1 - lead) if r[1] & 16 else (lead, n - 1 - trail)
        return out


def output_options(drop_duplicates=False, max_alignments=0, mapq=False):
    """flx_output_options (include/floxer_amd.h); not floxer's options, all off by default (then the records are floxer's):
    drop_duplicates: of a read's records with equal reference, strand, start, NM and CIGAR only the first is written;
    max_alignments: N > 0 writes the N records of a read with the smallest (NM, index), in output order (1: the primary only);
    mapq: every record carries a mapping quality made of the read's distinct loci (RunResult.mapq), computed from all of the read's
    records before the two options above drop any."""
    if max_alignments < 0:
        raise FloxerError("max_alignments must be >= 0 (0: no cap)")
    return capi.OutputOptions(int(bool(drop_duplicates)), int(bool(mapq)), int(max_alignments))


_REC_DTYPE = np.dtype([("read", "<u8"), ("flag", "<u4"), ("ref", "<i4"), ("pos", "<i4"), ("nm", "<u4"), ("coff", "<u8"),
                       ("clen", "<u4"), ("res", "<u4")])


def select_records(run_result, options):
    """keep mask (bool array, one entry per record) of flx_select_records: the output options' rule applied to the records of a
    RunResult, e.g. one made without options"""
    raw = np.ascontiguousarray(run_result.raw, dtype=_REC_DTYPE)
    cig = np.ascontiguousarray(run_result.cigars, dtype=np.uint32)
    if len(cig) == 0:
        cig = np.zeros(1, np.uint32)
    keep = np.zeros(max(1, len(raw)), dtype=np.uint8)
    check(lib().flx_select_records(raw.ctypes.data_as(C.POINTER(capi.Record)), len(raw), ptr(cig, u32p), C.byref(options),
                                   ptr(keep, u8p)))
    return keep[: len(raw)].astype(bool)


def assign_mapq(run_result, read_lengths=None):
    """mapping qualities (uint8 array, one entry per record) of flx_assign_mapq: the rule of output_options(mapq=True) applied to the
    records of a RunResult that holds all records of its reads. read_lengths (one entry per read of the batch): the span of a
    record without CIGAR; None: spans come from the CIGARs only"""
    raw = np.ascontiguousarray(run_result.raw, dtype=_REC_DTYPE)
    cig = np.ascontiguousarray(run_result.cigars, dtype=np.uint32)
    if len(cig) == 0:
        cig = np.zeros(1, np.uint32)
    lens = None
    if read_lengths is not None:
        lens = np.ascontiguousarray(read_lengths, dtype=np.uint64)
        if len(raw) and int(raw["read"].max()) >= len(lens):
            raise FloxerError("assign_mapq: read_lengths is shorter than the largest read index")
        if len(lens) == 0:
            lens = np.zeros(1, np.uint64)
    out = np.zeros(max(1, len(raw)), dtype=np.uint8)
    check(lib().flx_assign_mapq(raw.ctypes.data_as(C.POINTER(capi.Record)), len(raw), ptr(cig, u32p),
                                ptr(lens, u64p) if lens is not None else None, ptr(out, u8p)))
    return out[: len(raw)]


def _pool_and_offsets(reads):
    if isinstance(reads, tuple):
        pool, offs = as_u8(reads[0]), np.ascontiguousarray(reads[1], dtype=np.uint64)
        n = len(offs) - 1
    else:
        rs = [as_u8(r) for r in reads]
        n = len(rs)
        offs = np.zeros(n + 1, dtype=np.uint64)
        if n:
            offs[1:] = np.cumsum([len(r) for r in rs])
        pool = np.concatenate(rs) if n else np.zeros(0, np.uint8)
    if len(pool) == 0:
        pool = np.zeros(1, np.uint8)
    return pool, offs, n


class resident_reads:
    """A batch of reads uploaded to HBM once (forward + reverse complement); align it any number of times."""

    def __init__(self, ctx, reads):
        pool, offs, n = _pool_and_offsets(reads)
        self.ctx, self.n = ctx, n
        self.h = C.c_void_p()
        check(lib().flx_reads_upload(ctx.h, ptr(pool, u8p), ptr(offs, u64p), n, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().flx_reads_free(self.h)
            self.h = None

    __del__ = close


_CLIMB_DTYPE = np.dtype([("read", np.uint32), ("orientation", np.uint32), ("leaf", np.uint32), ("ref", np.uint32), ("pos", np.uint64)])


def climb_anchors(ctx, p, reads, anchors, host_rounds=False):
    """the verification rounds alone (flx_climb_anchors, a test hook): anchors = rows (read, orientation, leaf, reference_id,
    position) in (read, orientation) order on a resident_reads batch. Returns (status, node, requests): status[i] 0 dead / 1 at the
    root, node[i] the inner node anchor i failed at or the root's index, requests the call's inner tests requested."""
    arr = np.zeros(len(anchors), dtype=_CLIMB_DTYPE)
    for i, f in enumerate(("read", "orientation", "leaf", "ref", "pos")):
        arr[f] = [a[i] for a in anchors]
    n = len(arr)
    status, node = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint32)
    opt = capi.ClimbOptions(int(host_rounds))
    requests = C.c_uint64(0)
    check(lib().flx_climb_anchors(ctx.h, C.byref(p), reads.h, arr.ctypes.data_as(C.c_void_p), n, C.byref(opt), ptr(status, u8p), ptr(node, u32p),
                                  C.byref(requests)))
    return status[:n], node[:n], int(requests.value)


_MD_DTYPE = np.dtype([("off", np.uint64), ("len", np.uint32), ("res", np.uint32)])


def tag_options(md=False):
    """flx_tag_options (include/floxer_amd.h): optional tags, not floxer's; all off by default."""
    t = capi.TagOptions()
    t.md = int(bool(md))
    return t


def partial_options(min_query_span=0, max_records=0, enable=True):
    """flx_partial_options (include/floxer_amd.h): not floxer's. A read without a full alignment gets, in place of its unmapped record,
    its largest verified parts as soft-clipped records: a primary and non-overlapping supplementaries (flag 2048). min_query_span: the
    fewest query bases of such a part (0: 1000); max_records: the most records of a read (0: 4). Not together with without_cigar."""
    if min_query_span < 0 or max_records < 0:
        raise FloxerError("min_query_span and max_records must be >= 0 (0: the default)")
    o = capi.PartialOptions()
    o.enable, o.min_query_span, o.max_records = int(bool(enable)), int(min_query_span), int(max_records)
    return o


def extend_options(error_weight=0, x_drop=0, max_errors=0, enable=True):
    """flx_extend_options (include/floxer_amd.h): not floxer's. Both ends of every partial record are extended to the break: an
    extension keeps the rows R(d) reached with d errors that maximise R(d) - error_weight * d (0: 4), gives up once that score fell
    x_drop (0: 100) below its maximum and never takes more than max_errors (0: 1024) errors. Needs partial_options(...)."""
    if error_weight < 0 or x_drop < 0 or max_errors < 0:
        raise FloxerError("error_weight, x_drop and max_errors must be >= 0 (0: the default)")
    o = capi.ExtendOptions()
    o.enable, o.error_weight, o.x_drop, o.max_errors = int(bool(enable)), int(error_weight), int(x_drop), int(max_errors)
    return o


def split_options(error_weight=0, x_drop=0, min_tail_rows=0, enable=True):
    """flx_split_options (include/floxer_amd.h): not floxer's. A read mapped in full whose primary's score rows - error_weight * errors
    (0: 4) falls more than x_drop (0: 100) below its maximum towards an end, over at least min_tail_rows (0: 100) query bases, is
    written as a soft-clipped primary plus the supplementaries its anchors proved inside the tail. Needs partial_options(...) and
    output_options(max_alignments=1); not together with without_cigar."""
    if error_weight < 0 or x_drop < 0 or min_tail_rows < 0:
        raise FloxerError("error_weight, x_drop and min_tail_rows must be >= 0 (0: the default)")
    o = capi.SplitOptions()
    o.enable, o.error_weight, o.x_drop, o.min_tail_rows = int(bool(enable)), int(error_weight), int(x_drop), int(min_tail_rows)
    return o


def gap_options(left_align=True):
    """flx_gap_options (include/floxer_amd.h): not floxer's. Every traced path's gaps are moved to the leftmost column they reach without
    crossing an X or a gap of the other kind (the convention of VCF, minimap2 and bwa; floxer's and the default here is right-aligned),
    on the device, before MD strings and tails are computed. Not together with without_cigar."""
    o = capi.GapOptions()
    o.left_align = int(bool(left_align))
    return o


def _left_align_call(fn, head, reference_pool, query_pool, words, jobs):
    w = np.ascontiguousarray(words, dtype=np.uint32)
    n_words = len(w)
    if n_words == 0:
        w = np.zeros(1, np.uint32)
    q = as_u8(query_pool)
    n_q = len(q)
    if n_q == 0:
        q = np.zeros(1, np.uint8)
    if reference_pool is None:
        rp, rl_ = None, 0
    else:
        ref = as_u8(reference_pool)
        rp, rl_ = ptr(ref, u8p), len(ref)
    arr = (capi.LeftAlignJob * max(1, len(jobs)))()
    cap = 16
    for i, (co, cl, ro, rl, begin, qo, ql) in enumerate(jobs):
        arr[i] = capi.LeftAlignJob(int(co), int(cl), 0, int(ro), int(rl), int(begin), int(qo), int(ql), 0)
        cap += 2 * int(cl)
    out = np.zeros(cap, dtype=np.uint32)
    n_out = C.c_uint64(cap)
    refs = (capi.CigarRef * max(1, len(jobs)))()
    check(fn(*head, rp, rl_, ptr(q, u8p), n_q, ptr(w, u32p), n_words, arr, len(jobs), ptr(out, u32p), C.byref(n_out), refs))
    return [out[r.offset: r.offset + r.length].copy() for r in refs[: len(jobs)]]


def left_align(reference_pool, query_pool, words, jobs):
    """flx_left_align, the left-align rule on the host (floxer_amd/csrc/flx_leftalign.hpp): words = BAM CIGAR words (ops = X I D), jobs
    = [(cigar_offset, cigar_length, ref_offset, ref_length, begin, query_offset, query_length)]: the words of the job in the word
    pool, its reference window in reference_pool (column `begin` of it is the path's first) and its query in query_pool. Returns
    the normalised words of every job as a list of uint32 arrays."""
    return _left_align_call(lib().flx_left_align, (), reference_pool, query_pool, words, jobs)


def left_align_batch(ctx, query_pool, words, jobs, reference_pool=None):
    """flx_left_align_batch: the same words from the kernel cigar_left_align. reference_pool None = the context's reference text."""
    return _left_align_call(lib().flx_left_align_batch, (ctx.h,), reference_pool, query_pool, words, jobs)


REALIGN_DEFAULTS = dict(match=2, mismatch=4, gap_open=4, gap_extend=2, band=16)


def realign_options(enable=True, match=0, mismatch=0, gap_open=0, gap_extend=0, band=0):
    """flx_realign_options (include/floxer_amd.h): not floxer's. A traced path is realigned under affine gap costs inside a band around
    it (floxer_amd/csrc/flx_realign.hpp). 0 = the default of a field (REALIGN_DEFAULTS: the first piece of minimap2's map-ont scores,
    conventions, fitted to nothing); each score <= 255, band <= 1024, max(a + b, o + e + a) <= 8 min(a + b, o + e)."""
    o = capi.RealignOptions()
    o.enable = int(bool(enable))
    o.match, o.mismatch, o.gap_open, o.gap_extend, o.band = int(match), int(mismatch), int(gap_open), int(gap_extend), int(band)
    return o


def _realign_call(fn, head, reference_pool, query_pool, words, jobs, options):
    w = np.ascontiguousarray(words, dtype=np.uint32)
    n_words = len(w)
    if n_words == 0:
        w = np.zeros(1, np.uint32)
    q = as_u8(query_pool)
    n_q = len(q)
    if n_q == 0:
        q = np.zeros(1, np.uint8)
    if reference_pool is None:
        rp, rl_ = None, 0
    else:
        ref = as_u8(reference_pool)
        rp, rl_ = ptr(ref, u8p), len(ref)
    arr = (capi.RealignJob * max(1, len(jobs)))()
    for i, (co, cl, ro, rl, begin, qo, ql) in enumerate(jobs):
        arr[i] = capi.RealignJob(int(co), int(cl), 0, int(ro), int(rl), int(begin), int(qo), int(ql), 0)
    res = (capi.RealignResult * max(1, len(jobs)))()
    op = C.byref(options) if options is not None else None
    # room for every job's bound, max(cigar_length, 2 floor(NM c_max / c_min) + 1) (the call is the request: `enable` is not looked at)
    room_words, _ = _realign_room(options if options is not None else realign_options())
    cap = 16
    for co, cl, *_ in jobs:
        part = w[int(co): int(co) + int(cl)] if int(co) + int(cl) <= n_words else w[:0]
        cap += max(int(cl), room_words(int((part[(part & 15) != 7] >> 4).sum())))
    n_out = C.c_uint64(cap)
    out = np.zeros(cap, dtype=np.uint32)
    rc = fn(*head, rp, rl_, ptr(q, u8p), n_q, ptr(w, u32p), n_words, arr, len(jobs), op, ptr(out, u32p), C.byref(n_out), res)
    if rc == -3:                                                       # FLX_ERR_CAPACITY: the need is stored, once more with room for it
        out = np.zeros(n_out.value, dtype=np.uint32)
        rc = fn(*head, rp, rl_, ptr(q, u8p), n_q, ptr(w, u32p), n_words, arr, len(jobs), op, ptr(out, u32p), C.byref(n_out), res)
    check(rc)
    return [dict(words=out[r.offset: r.offset + r.length].copy(), num_errors=int(r.num_errors), score=int(r.score), diag_lo=int(r.diag_lo),
                 diag_hi=int(r.diag_hi), kept=int(r.kept)) for r in res[: len(jobs)]]


def realign(reference_pool, query_pool, words, jobs, options=None):
    """flx_realign, the affine-gap realignment rule on the host (floxer_amd/csrc/flx_realign.hpp): words and jobs as left_align takes
    them, options = realign_options(...) or None for the defaults. Returns one dict per job: words (uint32 array), num_errors, score,
    diag_lo, diag_hi, kept."""
    return _realign_call(lib().flx_realign, (), reference_pool, query_pool, words, jobs, options)


def realign_batch(ctx, query_pool, words, jobs, options=None, reference_pool=None):
    """flx_realign_batch: the same words and numbers from the kernel cigar_realign. reference_pool None = the context's reference text."""
    return _realign_call(lib().flx_realign_batch, (ctx.h,), reference_pool, query_pool, words, jobs, options)


def cs_options(long=False):
    """flx_cs_options (include/floxer_amd.h): not floxer's. Every mapped record gets minimap2's cs difference string, built on the device
    behind the MD strings (floxer_amd/csrc/flx_cs.hpp): the short form, or with long=True the long form, which holds the matched letters
    as well. Not together with without_cigar."""
    o = capi.CsOptions()
    o.form = 2 if long else 1
    return o


def _cs_call(fn, head, reference_pool, query_pool, words, jobs, long):
    q = as_u8(query_pool)
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32))
    if reference_pool is None:
        rp, rl_ = None, 0
    else:
        ref = as_u8(reference_pool)
        rp, rl_ = ptr(ref, u8p), len(ref)
    arr = (capi.CsJob * max(1, len(jobs)))()
    cap = 16
    for i, (co, cl, ro, rl, begin, qo, ql) in enumerate(jobs):
        arr[i] = capi.CsJob(int(co), int(cl), 0, int(ro), int(rl), int(begin), int(qo), int(ql), 0)
        # (the short form of a word is never longer than its long form: 1 + len, 3 len for X)
        cap += sum((3 if int(x) & 15 == 8 else 1) * (int(x) >> 4) + 1 for x in w[int(co): int(co) + int(cl)]) if 0 <= int(co) <= len(w) else 0
    refs = (capi.MdRef * max(1, len(jobs)))()
    options = cs_options(long=long)
    while True:
        out = np.zeros(cap, dtype=np.uint8)
        n = C.c_uint64(cap)
        rc = fn(*head, rp, rl_, ptr(q, u8p), len(q), ptr(w, u32p), len(w), arr, len(jobs), C.byref(options), ptr(out, u8p), C.byref(n), refs)
        if rc == -3 and n.value > cap:
            cap = n.value
            continue
        check(rc)
        break
    return [out[r.offset: r.offset + r.length].tobytes() for r in refs[: len(jobs)]]


def cs_string(reference_pool, query_pool, words, jobs, long=False):
    """flx_cs, the cs rule on the host (floxer_amd/csrc/flx_cs.hpp): words = BAM CIGAR words (ops = X I D), jobs = [(cigar_offset,
    cigar_length, ref_offset, ref_length, begin, query_offset, query_length)] as left_align takes them, query_offset the path's first
    query row. Returns one bytes object per job."""
    return _cs_call(lib().flx_cs, (), reference_pool, query_pool, words, jobs, long)


def cs_batch(ctx, query_pool, words, jobs, long=False, reference_pool=None):
    """flx_cs_batch: the same bytes from the kernel cs_build. reference_pool None = the context's reference text."""
    return _cs_call(lib().flx_cs_batch, (ctx.h,), reference_pool, query_pool, words, jobs, long)


def realign_counters(ctx):
    """flx_ctx_get_realign_counters: (paths_realigned, paths_changed, paths_kept) since the last reset of the path counters"""
    c = capi.RealignCounters()
    check(lib().flx_ctx_get_realign_counters(ctx.h, C.byref(c)))
    return int(c.paths_realigned), int(c.paths_changed), int(c.paths_kept)


TAIL_FIELDS = ("left_rows", "left_cols", "left_errors", "left_words", "right_rows", "right_cols", "right_errors", "right_words")


def _tail_jobs(words, jobs):
    w = np.ascontiguousarray(words, dtype=np.uint32)
    n_words = len(w)
    if n_words == 0:
        w = np.zeros(1, np.uint32)
    arr = (capi.TailJob * max(1, len(jobs)))()
    for i, j in enumerate(jobs):
        off, ln, ew, x, mr = (list(j) + [0, 0, 0])[:5]
        arr[i] = capi.TailJob(int(off), int(ln), int(ew), int(x), int(mr))
    return w, n_words, arr, (capi.TailResult * max(1, len(jobs)))()


def _tail_rows(res, n):
    return np.array([[getattr(r, f) for f in TAIL_FIELDS] for r in res[:n]], dtype=np.int64).reshape(-1, 8)


def cigar_tails(words, jobs):
    """flx_cigar_tails, the tail rule on the host: words = BAM CIGAR words (ops = X I D), jobs = [(cigar_offset, cigar_length[,
    error_weight, x_drop, min_tail_rows])] (the last three 0 or left out: the defaults). Returns an (n,8) int64 array {left_rows,
    left_cols, left_errors, left_words, right_rows, right_cols, right_errors, right_words} (TAIL_FIELDS); an absent tail is zeros."""
    w, n_words, arr, res = _tail_jobs(words, jobs)
    check(lib().flx_cigar_tails(ptr(w, u32p), n_words, arr, len(jobs), res))
    return _tail_rows(res, len(jobs))


def cigar_tails_batch(ctx, words, jobs):
    """flx_cigar_tails_batch: the same numbers from the kernel cigar_tails"""
    w, n_words, arr, res = _tail_jobs(words, jobs)
    check(lib().flx_cigar_tails_batch(ctx.h, ptr(w, u32p), n_words, arr, len(jobs), res))
    return _tail_rows(res, len(jobs))


EXTEND_STOP = {1: "x_drop", 2: "rows", 3: "max_errors"}


def extend_batch(ctx, query_pool, jobs, reference_pool=None):
    """flx_extend_batch, the extension kernel alone: jobs = [(text_pos, ref_limit, q_pos, row_limit, direction, error_weight, x_drop,
    max_errors)] (the last three 0: the defaults). reference_pool None = the context's reference text. Returns an (n,4) int64 array
    {rows, cols, errors, stop reason (EXTEND_STOP)}."""
    q = as_u8(query_pool)
    if len(q) == 0:
        q = np.zeros(1, np.uint8)
    arr = (capi.ExtendJob * max(1, len(jobs)))()
    for i, (tp, rl, qp, il, direction, w, x, dm) in enumerate(jobs):
        arr[i] = capi.ExtendJob(int(tp), int(qp), int(rl), int(il), int(direction), int(w), int(x), int(dm))
    res = (capi.ExtendResult * max(1, len(jobs)))()
    if reference_pool is None:
        rp, rl_ = None, 0
    else:
        ref = as_u8(reference_pool)
        rp, rl_ = ptr(ref, u8p), len(ref)
    check(lib().flx_extend_batch(ctx.h, rp, rl_, ptr(q, u8p), len(query_pool), arr, len(jobs), res))
    return np.array([(r.rows, r.cols, r.errors, r.stop_reason) for r in res[: len(jobs)]], dtype=np.int64).reshape(-1, 4)


def choose_partials(candidates, cigars=None, options=None):
    """flx_choose_partials: candidates = rows {read_index, q_from, q_to, orientation, reference_id, start, nm, cigar_offset, cigar_length}
    (a read's rows contiguous, in verification order; forward query coordinates). Returns an int32 array: -1 for a candidate that is not
    written, else its SAM flag."""
    arr = (capi.PartialCandidate * max(1, len(candidates)))()
    for a, c in zip(arr, candidates):
        a.read_index, a.q_from, a.q_to, a.orientation, a.reference_id, a.start, a.nm, a.cigar_offset, a.cigar_length = [int(x) for x in c]
    cig = np.ascontiguousarray(cigars, dtype=np.uint32) if cigars is not None and len(cigars) else None
    out = np.zeros(max(1, len(candidates)), dtype=np.int32)
    check(lib().flx_choose_partials(arr, len(candidates), ptr(cig, u32p) if cig is not None else None,
                                    C.byref(options) if options is not None else None, out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out[: len(candidates)]


def _collect_run(run, n, md=False, scores=False, cs=False, has_mapq=None):
    try:
        nr = lib().flx_run_num_records(run)
        nc = lib().flx_run_num_cigar_words(run)
        raw = np.empty(max(1, nr), dtype=_REC_DTYPE)
        cig = np.empty(max(1, nc), dtype=np.uint32)
        skipped = np.zeros(max(1, n), dtype=np.uint8)
        check(lib().flx_run_copy(run, raw.ctypes.data_as(C.POINTER(capi.Record)), ptr(cig, u32p), ptr(skipped, u8p)))
        raw = raw[:nr]
        md_refs = md_bytes = None
        if md:
            nb = lib().flx_run_num_md_bytes(run)
            refs = np.zeros(max(1, nr), dtype=_MD_DTYPE)
            md_bytes = np.zeros(max(1, nb), dtype=np.uint8)
            check(lib().flx_run_copy_md(run, refs.ctypes.data_as(C.POINTER(capi.MdRef)), ptr(md_bytes, u8p)))
            md_refs = np.stack([refs["off"][:nr], refs["len"][:nr].astype(np.uint64)], axis=1) if nr else np.zeros((0, 2), dtype=np.uint64)
            md_bytes = md_bytes[:nb]
        sc = None
        if scores:
            sc = np.zeros(max(1, nr), dtype=np.int32)
            check(lib().flx_run_copy_scores(run, sc.ctypes.data_as(C.POINTER(C.c_int32))))
            sc = sc[:nr]
        cs_refs = cs_bytes = None
        if cs:
            nb = lib().flx_run_num_cs_bytes(run)
            refs = np.zeros(max(1, nr), dtype=_MD_DTYPE)
            cs_bytes = np.zeros(max(1, nb), dtype=np.uint8)
            check(lib().flx_run_copy_cs(run, refs.ctypes.data_as(C.POINTER(capi.MdRef)), ptr(cs_bytes, u8p)))
            cs_refs = np.stack([refs["off"][:nr], refs["len"][:nr].astype(np.uint64)], axis=1) if nr else np.zeros((0, 2), dtype=np.uint64)
            cs_bytes = cs_bytes[:nb]
    finally:
        lib().flx_run_free(run)
    return RunResult(raw, cig[:nc], skipped[:n], md_refs, md_bytes, sc, cs_refs, cs_bytes, has_mapq)


class aligner:
    def __init__(self, ctx, p, output=None, md=False, partial=None, extend=None, split=None, gaps=None, realign=None, cs=None):
        """output: output_options(...), None: every alignment is written (floxer's output); md: every mapped record gets its MD
        string (RunResult.md), built on the device; not together with without_cigar; partial: partial_options(...), None: a read
        without a full alignment is written as unmapped (floxer's output); extend: extend_options(...), None: a partial record ends at
        its PEX node's boundary (needs partial); split: split_options(...), None: a read mapped in full is one record whatever its
        ends look like (needs partial and output_options(max_alignments=1)); gaps: gap_options(...), None: gaps stay right-aligned
        (floxer's output); realign: realign_options(...), None: every CIGAR stays an edit-distance path (floxer's output); with it
        RunResult.scores holds the records' scores; cs: cs_options(...), None: no cs strings (floxer's output); with it RunResult.cs
        holds the records' cs strings"""
        self.ctx, self.params, self.output, self.md, self.partial, self.extend, self.split = ctx, p, output, bool(md), partial, extend, split
        self.gaps = gaps
        self.realign = realign
        self.cs = cs

    def align_reads(self, reads):
        """reads: list of rank arrays, (pool, offsets), or resident_reads. Returns RunResult with records in --threads 1 order."""
        run = C.c_void_p()
        tags = tag_options(md=self.md)
        bundle = capi.RunOptions()
        bundle.tags = C.pointer(tags)
        for name in ("output", "partial", "extend"):
            if getattr(self, name) is not None:
                setattr(bundle, name, C.pointer(getattr(self, name)))
        split = C.byref(self.split) if self.split is not None else None
        gaps = C.byref(self.gaps) if self.gaps is not None else None
        realign = C.byref(self.realign) if self.realign is not None else None
        want_cs = self.cs is not None and bool(self.cs.form)
        if self.cs is not None:
            cs = C.byref(self.cs)
            if isinstance(reads, resident_reads):
                n = reads.n
                check(lib().flx_align_reads_resident_cs(self.ctx.h, C.byref(self.params), reads.h, C.byref(bundle), split, gaps, realign, cs, C.byref(run)))
            else:
                pool, offs, n = _pool_and_offsets(reads)
                check(lib().flx_align_reads_cs(self.ctx.h, C.byref(self.params), ptr(pool, u8p), ptr(offs, u64p), n, C.byref(bundle), split, gaps,
                                               realign, cs, C.byref(run)))
        elif isinstance(reads, resident_reads):
            n = reads.n
            check(lib().flx_align_reads_resident_realign(self.ctx.h, C.byref(self.params), reads.h, C.byref(bundle), split, gaps, realign, C.byref(run)))
        else:
            pool, offs, n = _pool_and_offsets(reads)
            check(lib().flx_align_reads_realign(self.ctx.h, C.byref(self.params), ptr(pool, u8p), ptr(offs, u64p), n, C.byref(bundle), split, gaps,
                                                realign, C.byref(run)))
        return _collect_run(run, n, md=self.md, scores=self.realign is not None and bool(self.realign.enable), cs=want_cs,
                            has_mapq=self.output is not None and bool(self.output.mapq))


def coverage_options(count_deletions=False, count_secondary=False, min_mapq=0, report_zero=False):
    """flx_coverage_options: count_deletions: D columns add depth (samtools depth -J); count_secondary: flag-256 records count;
    min_mapq: a record counts only with at least this mapping quality (needs runs made with output_options(mapq=True));
    report_zero: runs() lists the stretches of depth 0 too"""
    o = capi.CoverageOptions()
    o.count_deletions = 1 if count_deletions else 0
    o.count_secondary = 1 if count_secondary else 0
    o.min_mapq = int(min_mapq)
    o.report_zero = 1 if report_zero else 0
    return o


RUN_DTYPE = np.dtype([("ref", "<i4"), ("depth", "<u4"), ("start", "<u8"), ("end", "<u8")])
WINDOW_DTYPE = np.dtype([("ref", "<i4"), ("max_depth", "<u4"), ("start", "<u8"), ("end", "<u8"), ("depth_sum", "<u8"), ("covered", "<u8")])


def _records_and_words(records, cigar_words):
    rec = np.ascontiguousarray(np.asarray(records, dtype=_REC_DTYPE))
    words = np.ascontiguousarray(np.asarray(cigar_words, dtype=np.uint32))
    return rec, words


def coverage_geometry():
    """(elements per scan tile, tile sums per second-level block) of the finish scan: a test hook"""
    g = np.zeros(2, dtype=np.uint32)
    check(lib().flx_coverage_geometry(ptr(g, u32p)))
    return int(g[0]), int(g[1])


class coverage:
    """Depth of coverage over the sequences of a context's index (ctx) or over `lengths` on `device`: add the records of runs, absorb
    the objects of other devices, finish once, then read runs(), windows(w) and depth(ref, a, b). Not floxer's. Adds may come from
    several threads at once."""

    def __init__(self, ctx=None, options=None, lengths=None, device=0):
        self.h = C.c_void_p()
        self.min_mapq = int(options.min_mapq) if options is not None else 0
        opt = C.byref(options) if options is not None else None
        if ctx is not None:
            check(lib().flx_coverage_create(ctx.h, opt, C.byref(self.h)))
        else:
            if lengths is None:
                raise FloxerError("coverage needs a context or a list of reference lengths")
            lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
            check(lib().flx_coverage_create_for_lengths(int(device), ptr(lens, u64p), len(lens), opt, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().flx_coverage_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, run):
        """run: a RunResult (its records and CIGAR words are added), or a raw flx_run handle (ctypes.c_void_p) that has not been freed.
        With min_mapq a run made without output_options(mapq=True) is refused, as flx_coverage_add_run refuses it: its records hold no
        mapping quality. add_records cannot know and takes the records' `res` as it stands."""
        if isinstance(run, RunResult):
            if self.min_mapq > 0 and run.has_mapq is False:
                raise FloxerError("coverage.add: min_mapq needs a run made with output_options(mapq=True)")
            return self.add_records(run.raw, run.cigars)
        check(lib().flx_coverage_add_run(self.h, run))

    def add_records(self, records, cigar_words):
        """records: an array of the C ABI's flx_record (RunResult.raw's dtype); cigar_words: the uint32 pool their offsets refer to"""
        rec, words = _records_and_words(records, cigar_words)
        check(lib().flx_coverage_add_records(self.h, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p), len(words)))

    def absorb(self, other):
        check(lib().flx_coverage_absorb(self.h, other.h))

    def finish(self):
        check(lib().flx_coverage_finish(self.h))

    def runs(self):
        n = lib().flx_coverage_num_runs(self.h)
        out = np.zeros(max(1, n), dtype=RUN_DTYPE)
        check(lib().flx_coverage_copy_runs(self.h, out.ctypes.data_as(C.POINTER(capi.DepthRun)), n))
        return out[:n]

    def windows(self, w=0):
        n = lib().flx_coverage_num_windows(self.h, int(w))
        out = np.zeros(max(1, n), dtype=WINDOW_DTYPE)
        check(lib().flx_coverage_copy_windows(self.h, int(w), out.ctypes.data_as(C.POINTER(capi.DepthWindow)), n))
        return out[:n]

    def depth(self, ref, a, b):
        out = np.zeros(max(1, int(b) - int(a)), dtype=np.uint32)
        check(lib().flx_coverage_copy_depth(self.h, int(ref), int(a), int(b), ptr(out, u32p)))
        return out[: max(0, int(b) - int(a))]


def coverage_host(lengths, records, cigar_words, options=None):
    """the rule alone on the host (flx_coverage_host): the depth of every position of the concatenated sequences, uint32"""
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
    rec, words = _records_and_words(records, cigar_words)
    depth = np.zeros(max(1, int(lens.sum())), dtype=np.uint32)
    check(lib().flx_coverage_host(ptr(lens, u64p), len(lens), C.byref(options) if options is not None else None,
                                  rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p), len(words), ptr(depth, u32p)))
    return depth[: int(lens.sum())]


def pileup_options(count_secondary=False, min_mapq=0, min_depth=0, min_count=0, min_permille=0):
    """flx_pileup_options: count_secondary: flag-256 records count; min_mapq: a record counts only with at least this mapping quality
    (needs runs made with output_options(mapq=True)); a position is a site when DEPTH + DEL >= min_depth, its largest plane among A, C,
    G, T, DEL, INS >= min_count and that plane * 1000 >= min_permille * (DEPTH + DEL); 0 takes the defaults 4, 2 and 200, conventions of
    this project that are fitted to nothing"""
    o = capi.PileupOptions()
    o.count_secondary = 1 if count_secondary else 0
    o.min_mapq = int(min_mapq)
    o.min_depth, o.min_count, o.min_permille = int(min_depth), int(min_count), int(min_permille)
    return o


SITE_DTYPE = np.dtype([("ref", "<i4"), ("pos", "<u4"), ("depth", "<u4"), ("del", "<u4"), ("ins", "<u4"), ("alt", "<u4", (4,)), ("res", "<u4")])
PILEUP_PLANES = ("DEPTH", "DEL", "A", "C", "G", "T", "INS")


class pileup:
    """Allele pileup over the sequences of a context's index (ctx) or over `lengths` on `device`: per position the depth, the read letter
    of every mismatch column, the deletions and the insertions of the records added; absorb the objects of other devices, finish once,
    then read sites() and counts(ref, a, b). Not floxer's, and no variant caller: exact counts. Adds may come from several threads."""

    def __init__(self, ctx=None, options=None, lengths=None, device=0):
        self.h = C.c_void_p()
        self.min_mapq = int(options.min_mapq) if options is not None else 0
        opt = C.byref(options) if options is not None else None
        if ctx is not None:
            check(lib().flx_pileup_create(ctx.h, opt, C.byref(self.h)))
        else:
            if lengths is None:
                raise FloxerError("pileup needs a context or a list of reference lengths")
            lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
            check(lib().flx_pileup_create_for_lengths(int(device), ptr(lens, u64p), len(lens), opt, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().flx_pileup_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, run, reads):
        """run: a RunResult (its records and CIGAR words are added), or a raw flx_run handle (ctypes.c_void_p) that has not been freed;
        reads: the batch the run was made from: a list of rank arrays, (pool, offsets), or a resident_reads batch (with a raw handle only:
        its letters are read in HBM). With min_mapq a run made without output_options(mapq=True) is refused."""
        if isinstance(run, RunResult):
            if self.min_mapq > 0 and run.has_mapq is False:
                raise FloxerError("pileup.add: min_mapq needs a run made with output_options(mapq=True)")
            if isinstance(reads, resident_reads):
                raise FloxerError("pileup.add: a RunResult needs the reads in host memory; a resident batch goes with a raw run handle")
            return self.add_records(run.raw, run.cigars, reads)
        if isinstance(reads, resident_reads):
            check(lib().flx_pileup_add_run_resident(self.h, run, reads.h))
        else:
            pool, offs, n = _pool_and_offsets(reads)
            check(lib().flx_pileup_add_run(self.h, run, ptr(pool, u8p), ptr(offs, u64p), n))

    def add_records(self, records, cigar_words, reads):
        """records: an array of the C ABI's flx_record (RunResult.raw's dtype); cigar_words: the uint32 pool their offsets refer to;
        reads: a list of rank arrays or (pool, offsets), indexed by the records' `read`"""
        rec, words = _records_and_words(records, cigar_words)
        pool, offs, n = _pool_and_offsets(reads)
        check(lib().flx_pileup_add_records(self.h, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p), len(words),
                                           ptr(pool, u8p), ptr(offs, u64p), n))

    def absorb(self, other):
        check(lib().flx_pileup_absorb(self.h, other.h))

    def finish(self):
        check(lib().flx_pileup_finish(self.h))

    def sites(self):
        n = lib().flx_pileup_num_sites(self.h)
        out = np.zeros(max(1, n), dtype=SITE_DTYPE)
        check(lib().flx_pileup_copy_sites(self.h, out.ctypes.data_as(C.POINTER(capi.PileupSite)), n))
        return out[:n]

    def counts(self, ref, a, b):
        """the seven planes of [a, b) of sequence ref: a (7, b - a) uint32 array in the order of PILEUP_PLANES"""
        w = max(0, int(b) - int(a))
        out = np.zeros(7 * max(1, w), dtype=np.uint32)
        check(lib().flx_pileup_copy_counts(self.h, int(ref), int(a), int(b), ptr(out, u32p)))
        return out[: 7 * w].reshape(7, w)


def pileup_host(lengths, records, cigar_words, reads, options=None, counts=None):
    """the rule alone on the host (flx_pileup_host): a (7, total) uint32 array over the concatenated sequences in the order of
    PILEUP_PLANES; counts: such an array that is added to"""
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
    rec, words = _records_and_words(records, cigar_words)
    pool, offs, n = _pool_and_offsets(reads)
    total = int(lens.sum())
    out = np.zeros((7, max(1, total)), dtype=np.uint32) if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
    check(lib().flx_pileup_host(ptr(lens, u64p), len(lens), C.byref(options) if options is not None else None,
                                rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p), len(words), ptr(pool, u8p), ptr(offs, u64p), n,
                                ptr(out, u32p)))
    return out[:, :total] if counts is None else out


def pileup_sites_host(lengths, counts, options=None):
    """the site rule alone on the host (flx_pileup_sites_host) over a (7, total) count array: a structured array of SITE_DTYPE"""
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
    cnt = np.ascontiguousarray(counts, dtype=np.uint32)
    opt = C.byref(options) if options is not None else None
    n = C.c_uint64(0)
    rc = lib().flx_pileup_sites_host(ptr(lens, u64p), len(lens), opt, ptr(cnt, u32p), None, C.byref(n))
    if rc not in (0, -3):                                               # (FLX_ERR_CAPACITY: n holds the need)
        check(rc)
    out = np.zeros(max(1, n.value), dtype=SITE_DTYPE)
    check(lib().flx_pileup_sites_host(ptr(lens, u64p), len(lens), opt, ptr(cnt, u32p), out.ctypes.data_as(C.POINTER(capi.PileupSite)), C.byref(n)))
    return out[: n.value]


# ------------------------------------------------------------------------------------------------ error profile of the alignments
ERRPROF_SECTIONS = tuple(name for name, _ in capi.ERRPROF_SECTIONS if name != "reserved")
ERRPROF_TOTALS = ("records", "matches", "mismatches", "ins_events", "ins_bases", "del_events", "del_bases", "clip_bases")


def errprof_options(count_secondary=False, min_mapq=0, flush_threshold=0):
    """flx_errprof_options: count_secondary: flag-256 records count; min_mapq: a record counts only with at least this mapping quality
    (needs runs made with output_options(mapq=True)); flush_threshold: the columns plus rows after which a wave of the kernel adds its
    on-chip sums to the table (a test hook; 0 takes 2^30; no sum depends on it)"""
    o = capi.ErrprofOptions()
    o.count_secondary = 1 if count_secondary else 0
    o.min_mapq = int(min_mapq)
    o.flush_threshold = int(flush_threshold)
    return o


def _errprof_dict(table):
    return {name: np.array(getattr(table, name), dtype=np.uint64) for name in ERRPROF_SECTIONS}


def _concatenated_text(text):
    """(ranks of the unpadded concatenation, lengths) of a list of rank arrays; a single array is one sequence"""
    if isinstance(text, np.ndarray) and text.ndim == 1:
        text = [text]
    seqs = [as_u8(t) for t in text]
    return (np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.uint8)), [len(s) for s in seqs]


class errprof:
    """Error profile of the records added: which letter is read as which, the lengths of insertions and deletions and how many sit in
    homopolymers, errors by position in the read, identities and the lengths of error-free stretches, summed on the device. Over the text
    of a context's index (ctx), or over `text` on `device`: a list of rank arrays, or their concatenation with `lengths`. table() gives the
    sums so far at any time; absorb the objects of other devices. Not floxer's. Adds may come from several threads."""

    def __init__(self, ctx=None, options=None, text=None, lengths=None, device=0):
        self.h = C.c_void_p()
        self.min_mapq = int(options.min_mapq) if options is not None else 0
        opt = C.byref(options) if options is not None else None
        if ctx is not None:
            check(lib().flx_errprof_create(ctx.h, opt, C.byref(self.h)))
        else:
            if text is None:
                raise FloxerError("errprof needs a context or a reference text")
            concat, lens = (as_u8(text), list(lengths)) if lengths is not None else _concatenated_text(text)
            lens = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64))
            if int(lens.sum()) != len(concat):
                raise FloxerError("errprof: the lengths do not sum to the text's length")
            check(lib().flx_errprof_create_for_text(int(device), ptr(concat, u8p), ptr(lens, u64p), len(lens), opt, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().flx_errprof_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, run, reads):
        """run: a RunResult (its records and CIGAR words are added), or a raw flx_run handle (ctypes.c_void_p) that has not been freed;
        reads: the batch the run was made from: a list of rank arrays or (pool, offsets). With min_mapq a run made without
        output_options(mapq=True) is refused."""
        if isinstance(reads, resident_reads):
            return self.add_resident(run, reads)
        if isinstance(run, RunResult):
            if self.min_mapq > 0 and run.has_mapq is False:
                raise FloxerError("errprof.add: min_mapq needs a run made with output_options(mapq=True)")
            return self.add_records(run.raw, run.cigars, reads)
        pool, offs, n = _pool_and_offsets(reads)
        check(lib().flx_errprof_add_run(self.h, run, ptr(pool, u8p), ptr(offs, u64p), n))

    def add_resident(self, run, reads):
        """run: a raw flx_run handle; reads: the resident_reads batch it was made from: its letters are read in HBM when it lives on this
        object's device"""
        if isinstance(run, RunResult):
            raise FloxerError("errprof.add_resident: a RunResult needs the reads in host memory; a resident batch goes with a raw run handle")
        check(lib().flx_errprof_add_run_resident(self.h, run, reads.h))

    def add_records(self, records, cigar_words, reads):
        """records: an array of the C ABI's flx_record (RunResult.raw's dtype); cigar_words: the uint32 pool their offsets refer to;
        reads: a list of rank arrays or (pool, offsets), indexed by the records' `read`"""
        rec, words = _records_and_words(records, cigar_words)
        pool, offs, n = _pool_and_offsets(reads)
        check(lib().flx_errprof_add_records(self.h, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p), len(words),
                                            ptr(pool, u8p), ptr(offs, u64p), n))

    def absorb(self, other):
        check(lib().flx_errprof_absorb(self.h, other.h))

    def table(self):
        """the sums so far: a dict of uint64 arrays by the names of ERRPROF_SECTIONS (PAIR_EQ and PAIR_X: 36 entries, t * 6 + q)"""
        t = capi.ErrprofTable()
        check(lib().flx_errprof_copy(self.h, C.byref(t)))
        return _errprof_dict(t)


def errprof_host(text, lengths, records, cigar_words, reads, options=None, table=None):
    """the rule alone on the host (flx_errprof_host): text: the ranks of the unpadded concatenation of the sequences (or a list of rank
    arrays with lengths None); table: a dict as errprof.table() gives it, which is added to. Returns such a dict."""
    concat, lens = (as_u8(text), list(lengths)) if lengths is not None else _concatenated_text(text)
    lens = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64))
    if int(lens.sum()) != len(concat):
        raise FloxerError("errprof_host: the lengths do not sum to the text's length")
    rec, words = _records_and_words(records, cigar_words)
    pool, offs, n = _pool_and_offsets(reads)
    t = capi.ErrprofTable()
    if table is not None:
        for name in ERRPROF_SECTIONS:
            getattr(t, name)[:] = [int(x) for x in table[name]]
    check(lib().flx_errprof_host(ptr(concat, u8p), ptr(lens, u64p), len(lens), C.byref(options) if options is not None else None,
                                 rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p), len(words), ptr(pool, u8p), ptr(offs, u64p), n,
                                 C.byref(t)))
    return _errprof_dict(t)


# ------------------------------------------------------------------------------------------------ consensus sequence
CHANGE_DTYPE = np.dtype([("ref", "<i4"), ("pos", "<u4"), ("kind", "<u4"), ("ref_rank", "<u4"), ("alt_rank", "<u4"), ("length", "<u4"), ("count", "<u4"),
                         ("cov", "<u4"), ("letters", "<u8")])
ALLELE_DTYPE = np.dtype([("ref", "<i4"), ("pos", "<u4"), ("length", "<u4"), ("count", "<u4"), ("letters", "<u8")])
CONSENSUS_KINDS = ("SUB", "DEL", "INS")


def consensus_options(count_secondary=False, min_mapq=0, min_depth=0, min_count=0, min_permille=0, mask_low_depth=False):
    """flx_consensus_options: count_secondary and min_mapq as pileup_options has them; a position with DEPTH + DEL below min_depth keeps
    the reference letter (N with mask_low_depth); a call other than the reference letter, and the winning insertion behind a position,
    stand only with a count >= min_count and count * 1000 >= min_permille * (DEPTH + DEL); 0 takes the defaults 3, 2 and 500,
    conventions of this project that are fitted to nothing"""
    o = capi.ConsensusOptions()
    o.count_secondary = 1 if count_secondary else 0
    o.min_mapq = int(min_mapq)
    o.min_depth, o.min_count, o.min_permille = int(min_depth), int(min_count), int(min_permille)
    o.mask_low_depth = 1 if mask_low_depth else 0
    return o


def consensus_geometry():
    """(grid cap of consensus_ins_keys in blocks, its waves per block, the longest allele) (flx_consensus_geometry, a test hook)"""
    out = np.zeros(4, dtype=np.uint32)
    check(lib().flx_consensus_geometry(ptr(out, u32p)))
    return tuple(int(x) for x in out[:3])


def consensus_letters_of(letters, length):
    """the inserted letters of a change or an allele as a string: two bits each from the top of `letters`"""
    return "".join("ACGT"[(int(letters) >> (62 - 2 * k)) & 3] for k in range(int(length)))


class consensus:
    """Reference-guided consensus of the records added: pileup's counts plus the letters of every insertion of up to 32 bases, called on
    the device at finish. Over the text of a context's index (ctx), or over `text` on `device`: a list of rank arrays, or their
    concatenation with `lengths`. finish once, then read letters(ref), changes() and alleles(). One device: there is no absorb. Not
    floxer's. Adds may come from several threads."""

    def __init__(self, ctx=None, options=None, text=None, lengths=None, device=0):
        self.h = C.c_void_p()
        self.min_mapq = int(options.min_mapq) if options is not None else 0
        opt = C.byref(options) if options is not None else None
        if ctx is not None:
            check(lib().flx_consensus_create(ctx.h, opt, C.byref(self.h)))
        else:
            if text is None:
                raise FloxerError("consensus needs a context or a reference text")
            concat, lens = (as_u8(text), list(lengths)) if lengths is not None else _concatenated_text(text)
            lens = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64))
            if int(lens.sum()) != len(concat):
                raise FloxerError("consensus: the lengths do not sum to the text's length")
            check(lib().flx_consensus_create_for_text(int(device), ptr(concat, u8p), ptr(lens, u64p), len(lens), opt, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().flx_consensus_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, run, reads):
        """run: a RunResult (its records and CIGAR words are added), or a raw flx_run handle (ctypes.c_void_p) that has not been freed;
        reads: the batch the run was made from: a list of rank arrays, (pool, offsets), or a resident_reads batch (with a raw handle
        only). With min_mapq a run made without output_options(mapq=True) is refused."""
        if isinstance(run, RunResult):
            if self.min_mapq > 0 and run.has_mapq is False:
                raise FloxerError("consensus.add: min_mapq needs a run made with output_options(mapq=True)")
            if isinstance(reads, resident_reads):
                raise FloxerError("consensus.add: a RunResult needs the reads in host memory; a resident batch goes with a raw run handle")
            return self.add_records(run.raw, run.cigars, reads)
        if isinstance(reads, resident_reads):
            check(lib().flx_consensus_add_run_resident(self.h, run, reads.h))
        else:
            pool, offs, n = _pool_and_offsets(reads)
            check(lib().flx_consensus_add_run(self.h, run, ptr(pool, u8p), ptr(offs, u64p), n))

    def add_records(self, records, cigar_words, reads):
        """records: an array of the C ABI's flx_record (RunResult.raw's dtype); cigar_words: the uint32 pool their offsets refer to;
        reads: a list of rank arrays or (pool, offsets), indexed by the records' `read`"""
        rec, words = _records_and_words(records, cigar_words)
        pool, offs, n = _pool_and_offsets(reads)
        check(lib().flx_consensus_add_records(self.h, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p), len(words),
                                              ptr(pool, u8p), ptr(offs, u64p), n))

    def finish(self):
        check(lib().flx_consensus_finish(self.h))

    def letters(self, ref):
        """the consensus of sequence ref as a str (possibly empty)"""
        n = lib().flx_consensus_num_letters(self.h, int(ref))
        out = np.zeros(max(1, n), dtype=np.uint8)
        check(lib().flx_consensus_copy_letters(self.h, int(ref), out.ctypes.data_as(C.c_char_p), n))
        return out[:n].tobytes().decode("ascii")

    def changes(self):
        """every place the consensus departs from the text, in position order: a structured array of CHANGE_DTYPE"""
        n = lib().flx_consensus_num_changes(self.h)
        out = np.zeros(max(1, n), dtype=CHANGE_DTYPE)
        check(lib().flx_consensus_copy_changes(self.h, out.ctypes.data_as(C.POINTER(capi.ConsensusChange)), n))
        return out[:n]

    def alleles(self):
        """every insertion allele with its count, in key order (a test hook): a structured array of ALLELE_DTYPE"""
        n = lib().flx_consensus_num_alleles(self.h)
        out = np.zeros(max(1, n), dtype=ALLELE_DTYPE)
        check(lib().flx_consensus_copy_alleles(self.h, out.ctypes.data_as(C.POINTER(capi.ConsensusAllele)), n))
        return out[:n]


def consensus_host(text, lengths, records, cigar_words, reads, options=None):
    """the rule alone on the host (flx_consensus_host): text and lengths as errprof_host takes them. Returns (letters, changes, alleles):
    a list of str per sequence and two structured arrays (CHANGE_DTYPE, ALLELE_DTYPE)."""
    concat, lens = (as_u8(text), list(lengths)) if lengths is not None else _concatenated_text(text)
    lens = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64))
    if int(lens.sum()) != len(concat):
        raise FloxerError("consensus_host: the lengths do not sum to the text's length")
    rec, words = _records_and_words(records, cigar_words)
    pool, offs, n = _pool_and_offsets(reads)
    opt = C.byref(options) if options is not None else None
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    need = [C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)]

    def call(letters, changes, alleles):
        return lib().flx_consensus_host(ptr(concat, u8p), ptr(lens, u64p), len(lens), opt, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p),
                                        len(words), ptr(pool, u8p), ptr(offs, u64p), n, ptr(offsets, u64p),
                                        letters.ctypes.data_as(C.c_char_p) if letters is not None else None, C.byref(need[0]),
                                        changes.ctypes.data_as(C.POINTER(capi.ConsensusChange)) if changes is not None else None, C.byref(need[1]),
                                        alleles.ctypes.data_as(C.POINTER(capi.ConsensusAllele)) if alleles is not None else None, C.byref(need[2]))

    rc = call(None, None, None)
    if rc not in (0, -3):                                               # (FLX_ERR_CAPACITY: need holds the sizes)
        check(rc)
    letters = np.zeros(max(1, need[0].value), dtype=np.uint8)
    changes = np.zeros(max(1, need[1].value), dtype=CHANGE_DTYPE)
    alleles = np.zeros(max(1, need[2].value), dtype=ALLELE_DTYPE)
    check(call(letters, changes, alleles))
    text_out = letters[: need[0].value].tobytes().decode("ascii")
    return ([text_out[int(offsets[r]): int(offsets[r + 1])] for r in range(len(lens))], changes[: need[1].value], alleles[: need[2].value])


# ------------------------------------------------------------------------------------------------ diploid small-variant calls
VARIANT_DTYPE = np.dtype([("ref", "<i4"), ("pos", "<u4"), ("kind", "<u4"), ("ref_rank", "<u4"), ("alt_rank", "<u4"), ("length", "<u4"), ("ref_count", "<u4"),
                          ("alt_count", "<u4"), ("cov", "<u4"), ("gt", "<u4"), ("gq", "<u4"), ("qual", "<u4"), ("pl", "<u4", (3,)), ("reserved", "<u4"),
                          ("letters", "<u8")])
VARIANT_ALLELE_DTYPE = np.dtype([("ref", "<i4"), ("pos", "<u4"), ("kind", "<u4"), ("length", "<u4"), ("count", "<u4"), ("reserved", "<u4"), ("letters", "<u8")])
VARIANT_KINDS = ("SNV", "DEL", "INS")


def variants_options(count_secondary=False, min_mapq=0, min_depth=0, min_qual=0, max_del=0, cost_match=0, cost_mismatch=0, cost_het=0, prior_het=0, prior_hom=0):
    """flx_variants_options: count_secondary and min_mapq as pileup_options has them; a call is written only with DEPTH + DEL >= min_depth
    and a quality of at least min_qual (centi-phred); a deletion of more than max_del bases is no allele; the five costs of the genotype
    model in centi-phred (-1000 log10 of a probability). 0 takes the defaults 4, 2000, 50 and 36 / 1574 / 325 / 3000 / 3301 (a per-read
    error of 0.08, a heterozygosity of 0.001), conventions of this project that are fitted to nothing"""
    o = capi.VariantsOptions()
    o.count_secondary = 1 if count_secondary else 0
    o.min_mapq = int(min_mapq)
    o.min_depth, o.min_qual, o.max_del = int(min_depth), int(min_qual), int(max_del)
    o.cost_match, o.cost_mismatch, o.cost_het, o.prior_het, o.prior_hom = int(cost_match), int(cost_mismatch), int(cost_het), int(prior_het), int(prior_hom)
    return o


def variants_geometry():
    """(grid cap of variants_indel_keys in blocks, its waves per block, the longest insertion, the default max_del) (flx_variants_geometry,
    a test hook)"""
    out = np.zeros(4, dtype=np.uint32)
    check(lib().flx_variants_geometry(ptr(out, u32p)))
    return tuple(int(x) for x in out)


def variants_genotype(ref_n, alt_n, oth, options=None):
    """the genotype of one candidate (flx_variants_genotype, a test hook): dict(gt, gq, qual, pl, row); gt 0 = 0/0, 1 = 0/1, 2 = 1/1; row:
    whether a call would be written with cov = ref_n + alt_n + oth"""
    out = np.zeros(8, dtype=np.uint32)
    check(lib().flx_variants_genotype(C.byref(options) if options is not None else None, int(ref_n), int(alt_n), int(oth), ptr(out, u32p)))
    return dict(gt=int(out[0]), gq=int(out[1]), qual=int(out[2]), pl=[int(x) for x in out[3:6]], row=bool(out[6]))


class variants:
    """Diploid small-variant calls of the records added: pileup's counts plus one key per insertion of up to 32 bases and per deletion of
    up to max_del, genotyped on the device at finish. Over the text of a context's index (ctx), or over `text` on `device`: a list of
    rank arrays, or their concatenation with `lengths`. finish once, then read rows() and alleles(). One device: there is no absorb.
    Not floxer's. Adds may come from several threads."""

    def __init__(self, ctx=None, options=None, text=None, lengths=None, device=0):
        self.h = C.c_void_p()
        self.min_mapq = int(options.min_mapq) if options is not None else 0
        opt = C.byref(options) if options is not None else None
        if ctx is not None:
            check(lib().flx_variants_create(ctx.h, opt, C.byref(self.h)))
        else:
            if text is None:
                raise FloxerError("variants needs a context or a reference text")
            concat, lens = (as_u8(text), list(lengths)) if lengths is not None else _concatenated_text(text)
            lens = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64))
            if int(lens.sum()) != len(concat):
                raise FloxerError("variants: the lengths do not sum to the text's length")
            check(lib().flx_variants_create_for_text(int(device), ptr(concat, u8p), ptr(lens, u64p), len(lens), opt, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().flx_variants_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, run, reads):
        """run: a RunResult (its records and CIGAR words are added), or a raw flx_run handle (ctypes.c_void_p) that has not been freed;
        reads: the batch the run was made from: a list of rank arrays, (pool, offsets), or a resident_reads batch (with a raw handle
        only). With min_mapq a run made without output_options(mapq=True) is refused."""
        if isinstance(run, RunResult):
            if self.min_mapq > 0 and run.has_mapq is False:
                raise FloxerError("variants.add: min_mapq needs a run made with output_options(mapq=True)")
            if isinstance(reads, resident_reads):
                raise FloxerError("variants.add: a RunResult needs the reads in host memory; a resident batch goes with a raw run handle")
            return self.add_records(run.raw, run.cigars, reads)
        if isinstance(reads, resident_reads):
            check(lib().flx_variants_add_run_resident(self.h, run, reads.h))
        else:
            pool, offs, n = _pool_and_offsets(reads)
            check(lib().flx_variants_add_run(self.h, run, ptr(pool, u8p), ptr(offs, u64p), n))

    def add_records(self, records, cigar_words, reads):
        """records: an array of the C ABI's flx_record (RunResult.raw's dtype); cigar_words: the uint32 pool their offsets refer to;
        reads: a list of rank arrays or (pool, offsets), indexed by the records' `read`"""
        rec, words = _records_and_words(records, cigar_words)
        pool, offs, n = _pool_and_offsets(reads)
        check(lib().flx_variants_add_records(self.h, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p), len(words),
                                             ptr(pool, u8p), ptr(offs, u64p), n))

    def finish(self):
        check(lib().flx_variants_finish(self.h))

    def rows(self):
        """the calls in position order, an SNV in front of the indel of the same position: a structured array of VARIANT_DTYPE"""
        n = lib().flx_variants_num_rows(self.h)
        out = np.zeros(max(1, n), dtype=VARIANT_DTYPE)
        check(lib().flx_variants_copy_rows(self.h, out.ctypes.data_as(C.POINTER(capi.Variant)), n))
        return out[:n]

    def alleles(self):
        """every insertion and deletion allele with its count, in key order (a test hook): a structured array of VARIANT_ALLELE_DTYPE"""
        n = lib().flx_variants_num_alleles(self.h)
        out = np.zeros(max(1, n), dtype=VARIANT_ALLELE_DTYPE)
        check(lib().flx_variants_copy_alleles(self.h, out.ctypes.data_as(C.POINTER(capi.VariantAllele)), n))
        return out[:n]


def variants_host(text, lengths, records, cigar_words, reads, options=None):
    """the rule alone on the host (flx_variants_host): text and lengths as errprof_host takes them. Returns (rows, alleles): two
    structured arrays (VARIANT_DTYPE, VARIANT_ALLELE_DTYPE)."""
    concat, lens = (as_u8(text), list(lengths)) if lengths is not None else _concatenated_text(text)
    lens = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64))
    if int(lens.sum()) != len(concat):
        raise FloxerError("variants_host: the lengths do not sum to the text's length")
    rec, words = _records_and_words(records, cigar_words)
    pool, offs, n = _pool_and_offsets(reads)
    opt = C.byref(options) if options is not None else None
    need = [C.c_uint64(0), C.c_uint64(0)]

    def call(rows, alleles):
        return lib().flx_variants_host(ptr(concat, u8p), ptr(lens, u64p), len(lens), opt, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p),
                                       len(words), ptr(pool, u8p), ptr(offs, u64p), n,
                                       rows.ctypes.data_as(C.POINTER(capi.Variant)) if rows is not None else None, C.byref(need[0]),
                                       alleles.ctypes.data_as(C.POINTER(capi.VariantAllele)) if alleles is not None else None, C.byref(need[1]))

    rc = call(None, None)
    if rc not in (0, -3):                                               # (FLX_ERR_CAPACITY: need holds the sizes)
        check(rc)
    rows = np.zeros(max(1, need[0].value), dtype=VARIANT_DTYPE)
    alleles = np.zeros(max(1, need[1].value), dtype=VARIANT_ALLELE_DTYPE)
    check(call(rows, alleles))
    return rows[: need[0].value], alleles[: need[1].value]


# ------------------------------------------------------------------------------------------------ read-backed phasing
PHASE_SITE_DTYPE = np.dtype([("ref", "<i4"), ("pos", "<u4"), ("kind", "<u4"), ("alt_rank", "<u4"), ("length", "<u4"), ("reserved", "<u4"), ("letters", "<u8")])
PHASE_RESULT_DTYPE = np.dtype([("phase_set", "<u4"), ("phased", "<u4"), ("phase", "<u4"), ("cis", "<u4"), ("trans", "<u4"), ("keep", "<u4"), ("swap", "<u4"), ("reserved", "<u4")])
PHASE_TAG_DTYPE = np.dtype([("add", "<u4"), ("read", "<u4"), ("hap", "<u4"), ("phase_set", "<u4"), ("h1", "<u4"), ("h2", "<u4"), ("n_slots", "<u4"), ("reserved", "<u4")])


def phase_options(count_secondary=False, min_mapq=0, min_link=0, min_margin=0, refine_rounds=0, skip_refine=False):
    """flx_phase_options: count_secondary and min_mapq as pileup_options has them; neighbouring sites are joined when the records for
    and against differ by at least min_link; a record is tagged when its observations for one haplotype lead by at least min_margin;
    refine_rounds rounds of votes (at most 8), none with skip_refine. 0 takes the defaults 2 / 1 / 1, conventions of this project that
    are fitted to nothing"""
    o = capi.PhaseOptions()
    o.count_secondary = 1 if count_secondary else 0
    o.min_mapq, o.min_link, o.min_margin, o.refine_rounds = int(min_mapq), int(min_link), int(min_margin), int(refine_rounds)
    o.skip_refine = 1 if skip_refine else 0
    return o


def phase_geometry():
    """(grid cap of phase_observe in blocks, its waves per block, the scan tile, the longest insertion) (flx_phase_geometry, a test hook)"""
    out = np.zeros(4, dtype=np.uint32)
    check(lib().flx_phase_geometry(ptr(out, u32p)))
    return tuple(int(x) for x in out)


def phase_sites_from_rows(rows):
    """the sites of a variants result: its heterozygous rows (gt == 1), in their order, as an array of PHASE_SITE_DTYPE"""
    rows = np.asarray(rows, dtype=VARIANT_DTYPE)
    het = rows[rows["gt"] == 1]
    out = np.zeros(len(het), dtype=PHASE_SITE_DTYPE)
    for name in ("ref", "pos", "kind", "alt_rank", "length", "letters"):
        out[name] = het[name]
    return out


def _phase_sites(sites):
    return np.ascontiguousarray(np.asarray(sites, dtype=PHASE_SITE_DTYPE))


class phase:
    """Read-backed phasing of the heterozygous `sites` (an array of PHASE_SITE_DTYPE, phase_sites_from_rows makes one) by the records
    added: one observation per record and site in its span, links between neighbouring sites, phase sets, haplotype tags, rounds of
    votes. For a context (ctx), or over `text` on `device`: a list of rank arrays, or their concatenation with `lengths`. finish once,
    then read results() and tags(). One device: there is no absorb. Not floxer's. Adds may come from several threads."""

    def __init__(self, ctx=None, options=None, sites=None, text=None, lengths=None, device=0):
        self.h = C.c_void_p()
        self.min_mapq = int(options.min_mapq) if options is not None else 0
        opt = C.byref(options) if options is not None else None
        sites = _phase_sites(sites if sites is not None else [])
        sp = sites.ctypes.data_as(C.POINTER(capi.PhaseSite))
        if ctx is not None:
            check(lib().flx_phase_create(ctx.h, opt, sp, len(sites), C.byref(self.h)))
        else:
            if text is None:
                raise FloxerError("phase needs a context or a reference text")
            concat, lens = (as_u8(text), list(lengths)) if lengths is not None else _concatenated_text(text)
            lens = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64))
            if int(lens.sum()) != len(concat):
                raise FloxerError("phase: the lengths do not sum to the text's length")
            check(lib().flx_phase_create_for_text(int(device), ptr(concat, u8p), ptr(lens, u64p), len(lens), opt, sp, len(sites), C.byref(self.h)))

    def close(self):
        if self.h:
            lib().flx_phase_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, run, reads):
        """run: a RunResult (its records and CIGAR words are added), or a raw flx_run handle (ctypes.c_void_p) that has not been freed;
        reads: the batch the run was made from: a list of rank arrays, (pool, offsets), or a resident_reads batch (with a raw handle
        only). With min_mapq a run made without output_options(mapq=True) is refused."""
        if isinstance(run, RunResult):
            if self.min_mapq > 0 and run.has_mapq is False:
                raise FloxerError("phase.add: min_mapq needs a run made with output_options(mapq=True)")
            if isinstance(reads, resident_reads):
                raise FloxerError("phase.add: a RunResult needs the reads in host memory; a resident batch goes with a raw run handle")
            return self.add_records(run.raw, run.cigars, reads)
        if isinstance(reads, resident_reads):
            check(lib().flx_phase_add_run_resident(self.h, run, reads.h))
        else:
            pool, offs, n = _pool_and_offsets(reads)
            check(lib().flx_phase_add_run(self.h, run, ptr(pool, u8p), ptr(offs, u64p), n))

    def add_records(self, records, cigar_words, reads):
        """records: an array of the C ABI's flx_record (RunResult.raw's dtype); cigar_words: the uint32 pool their offsets refer to;
        reads: a list of rank arrays or (pool, offsets), indexed by the records' `read`"""
        rec, words = _records_and_words(records, cigar_words)
        pool, offs, n = _pool_and_offsets(reads)
        check(lib().flx_phase_add_records(self.h, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p), len(words), ptr(pool, u8p), ptr(offs, u64p), n))

    def finish(self):
        check(lib().flx_phase_finish(self.h))

    def results(self):
        """one row per site, in the sites' order: a structured array of PHASE_RESULT_DTYPE"""
        n = lib().flx_phase_num_sites(self.h)
        out = np.zeros(max(1, n), dtype=PHASE_RESULT_DTYPE)
        check(lib().flx_phase_copy_results(self.h, out.ctypes.data_as(C.POINTER(capi.PhaseResult)), n))
        return out[:n]

    def tags(self):
        """one row per counted record, in counting order: a structured array of PHASE_TAG_DTYPE"""
        n = lib().flx_phase_num_tags(self.h)
        out = np.zeros(max(1, n), dtype=PHASE_TAG_DTYPE)
        check(lib().flx_phase_copy_tags(self.h, out.ctypes.data_as(C.POINTER(capi.PhaseTag)), n))
        return out[:n]


def phase_host(text, lengths, sites, records, cigar_words, reads, options=None):
    """the rule alone on the host (flx_phase_host): text and lengths as variants_host takes them. Returns (results, tags): two
    structured arrays (PHASE_RESULT_DTYPE, PHASE_TAG_DTYPE)."""
    concat, lens = (as_u8(text), list(lengths)) if lengths is not None else _concatenated_text(text)
    lens = np.ascontiguousarray(np.asarray(lens, dtype=np.uint64))
    if int(lens.sum()) != len(concat):
        raise FloxerError("phase_host: the lengths do not sum to the text's length")
    sites = _phase_sites(sites)
    rec, words = _records_and_words(records, cigar_words)
    pool, offs, n = _pool_and_offsets(reads)
    opt = C.byref(options) if options is not None else None
    need = C.c_uint64(len(rec))
    results = np.zeros(max(1, len(sites)), dtype=PHASE_RESULT_DTYPE)
    tags = np.zeros(max(1, len(rec)), dtype=PHASE_TAG_DTYPE)
    check(lib().flx_phase_host(ptr(concat, u8p), ptr(lens, u64p), len(lens), opt, sites.ctypes.data_as(C.POINTER(capi.PhaseSite)), len(sites),
                               rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p), len(words), ptr(pool, u8p), ptr(offs, u64p), n,
                               results.ctypes.data_as(C.POINTER(capi.PhaseResult)), tags.ctypes.data_as(C.POINTER(capi.PhaseTag)), C.byref(need)))
    return results[: len(sites)], tags[: need.value]


# ------------------------------------------------------------------------------------------------ structural-variant signatures
SV_SIGNATURE_DTYPE = np.dtype([("type", "<u4"), ("side_a", "<u4"), ("side_b", "<u4"), ("res", "<u4"), ("ref_a", "<i4"), ("ref_b", "<i4"), ("pos_a", "<u4"), ("q", "<u4")])
SV_CLUSTER_DTYPE = np.dtype([("type", "<u4"), ("side_a", "<u4"), ("side_b", "<u4"), ("support", "<u4"), ("ref_a", "<i4"), ("ref_b", "<i4"), ("pos_a_min", "<u4"),
                             ("pos_a_max", "<u4"), ("q_min", "<u4"), ("q_median", "<u4"), ("q_max", "<u4"), ("res", "<u4")])
SV_TYPES = ("DEL", "INS", "BND")


def sv_options(min_length=0, max_distance=0, min_support=0, count_secondary=False, min_mapq=0, initial_capacity=0):
    """flx_sv_options: min_length: the fewest symbols of a D or I word that is a signature; max_distance: the largest gap, in pos_a and
    in q, between neighbours of one cluster; min_support: the fewest members of a reported cluster; 0 takes the defaults 50, 100 and 2,
    conventions of this project that are fitted to nothing. count_secondary: flag-256 records count (they never form junctions);
    min_mapq: a record counts only with at least this mapping quality (needs runs made with output_options(mapq=True));
    initial_capacity: the keys the table holds before it first grows (a test hook)"""
    o = capi.SvOptions()
    o.min_length, o.max_distance, o.min_support = int(min_length), int(max_distance), int(min_support)
    o.count_secondary = 1 if count_secondary else 0
    o.min_mapq = int(min_mapq)
    o.initial_capacity = int(initial_capacity)
    return o


class sv:
    """Structural-variant signatures over the sequences of a context's index (ctx) or over `lengths` on `device`: one signature per long
    D word, long I word and junction between query-neighbouring records of a read; absorb the objects of other devices, finish once,
    then read signatures() and clusters(). Not floxer's, and no variant caller: an exact table. Support counts records, not reads:
    make the runs with output_options(drop_duplicates=True, max_alignments=1). Adds may come from several threads."""

    def __init__(self, ctx=None, options=None, lengths=None, device=0):
        self.h = C.c_void_p()
        self.min_mapq = int(options.min_mapq) if options is not None else 0
        opt = C.byref(options) if options is not None else None
        if ctx is not None:
            check(lib().flx_sv_create(ctx.h, opt, C.byref(self.h)))
        else:
            if lengths is None:
                raise FloxerError("sv needs a context or a list of reference lengths")
            lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
            check(lib().flx_sv_create_for_lengths(int(device), ptr(lens, u64p), len(lens), opt, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().flx_sv_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_run(self, run, read_lengths):
        """run: a RunResult (its records and CIGAR words are added), or a raw flx_run handle (ctypes.c_void_p) that has not been freed;
        read_lengths: the lengths of the reads of the batch the run was made from. With min_mapq a run made without
        output_options(mapq=True) is refused. A raw handle goes through flx_sv_add_run, which forms a read's group within one piece of
        the run; a RunResult holds the pieces' records in one array and goes through flx_sv_add_records. Both give the same groups:
        all records of a read lie in one piece, next to each other, and neighbouring pieces hold different reads."""
        if isinstance(run, RunResult):
            if self.min_mapq > 0 and run.has_mapq is False:
                raise FloxerError("sv.add_run: min_mapq needs a run made with output_options(mapq=True)")
            return self.add_records(run.raw, run.cigars, read_lengths)
        offs = _read_offsets(read_lengths)
        check(lib().flx_sv_add_run(self.h, run, ptr(offs, u64p), len(offs) - 1))

    def add_records(self, records, cigar_words, read_lengths):
        """records: an array of the C ABI's flx_record (RunResult.raw's dtype); cigar_words: the uint32 pool their offsets refer to;
        read_lengths: indexed by the records' `read`"""
        rec, words = _records_and_words(records, cigar_words)
        offs = _read_offsets(read_lengths)
        check(lib().flx_sv_add_records(self.h, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p) if len(words) else None, len(words),
                                       ptr(offs, u64p), len(offs) - 1))

    def absorb(self, other):
        check(lib().flx_sv_absorb(self.h, other.h))

    def finish(self):
        check(lib().flx_sv_finish(self.h))

    def signatures(self):
        """all signatures in key order, whatever min_support: a structured array of SV_SIGNATURE_DTYPE"""
        out = np.zeros(1, dtype=SV_SIGNATURE_DTYPE)
        check(lib().flx_sv_copy_signatures(self.h, 0, 0, out.ctypes.data_as(C.POINTER(capi.SvSignature))))       # (refused before finish)
        n = lib().flx_sv_num_signatures(self.h)
        out = np.zeros(max(1, n), dtype=SV_SIGNATURE_DTYPE)
        check(lib().flx_sv_copy_signatures(self.h, 0, n, out.ctypes.data_as(C.POINTER(capi.SvSignature))))
        return out[:n]

    def clusters(self):
        """the clusters with support >= min_support, in (class, coarse group, q) order: a structured array of SV_CLUSTER_DTYPE"""
        n = lib().flx_sv_num_clusters(self.h)
        out = np.zeros(max(1, n), dtype=SV_CLUSTER_DTYPE)
        check(lib().flx_sv_copy_clusters(self.h, out.ctypes.data_as(C.POINTER(capi.SvCluster)), n))
        return out[:n]


def sv_host(lengths, records, cigar_words, read_lengths, options=None):
    """the rule alone on the host (flx_sv_host): the signatures of the records in key order, a structured array of SV_SIGNATURE_DTYPE"""
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
    rec, words = _records_and_words(records, cigar_words)
    offs = _read_offsets(read_lengths)
    opt = C.byref(options) if options is not None else None
    args = (ptr(lens, u64p) if len(lens) else None, len(lens), opt, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p) if len(words) else None,
            len(words), ptr(offs, u64p), len(offs) - 1)
    n = C.c_uint64(0)
    rc = lib().flx_sv_host(*args, None, C.byref(n))
    if rc not in (0, -3):                                               # (FLX_ERR_CAPACITY: n holds the need)
        check(rc)
    out = np.zeros(max(1, n.value), dtype=SV_SIGNATURE_DTYPE)
    check(lib().flx_sv_host(*args, out.ctypes.data_as(C.POINTER(capi.SvSignature)), C.byref(n)))
    return out[: n.value]


def sv_clusters_host(signatures, options=None):
    """the cluster rule alone on the host (flx_sv_clusters_host) over signatures in any order: a structured array of SV_CLUSTER_DTYPE"""
    sig = np.ascontiguousarray(np.asarray(signatures, dtype=SV_SIGNATURE_DTYPE))
    opt = C.byref(options) if options is not None else None
    n = C.c_uint64(0)
    rc = lib().flx_sv_clusters_host(opt, sig.ctypes.data_as(C.POINTER(capi.SvSignature)), len(sig), None, C.byref(n))
    if rc not in (0, -3):
        check(rc)
    out = np.zeros(max(1, n.value), dtype=SV_CLUSTER_DTYPE)
    check(lib().flx_sv_clusters_host(opt, sig.ctypes.data_as(C.POINTER(capi.SvSignature)), len(sig), out.ctypes.data_as(C.POINTER(capi.SvCluster)), C.byref(n)))
    return out[: n.value]


# ------------------------------------------------------------------------------------------------ structural-variant calls
SVCALL_ROW_DTYPE = np.dtype([("cluster", "<u4"), ("type", "<u4"), ("ref", "<i4"), ("pos_a_min", "<u4"), ("pos_a_max", "<u4"), ("q_min", "<u4"), ("q_median", "<u4"),
                             ("q_max", "<u4"), ("alt_n", "<u4"), ("ref_n", "<u4"), ("span_n", "<u4"), ("gt", "<u4"), ("gq", "<u4"), ("qual", "<u4"), ("pl", "<u4", (3,)),
                             ("pass", "<u4")])


def svcall_options(count_secondary=False, min_mapq=0, flank=0, min_depth=0, min_qual=0, cost_match=0, cost_mismatch=0, cost_het=0, prior_het=0, prior_hom=0):
    """flx_svcall_options: flank: the columns a record must reach on both sides of a cluster to count as spanning it; min_depth: the
    fewest records (ref_n + alt_n) of a passing row; min_qual: its smallest quality in centi-phred; the five costs of the genotype
    model in centi-phred, flx_variants' own. 0 takes the defaults 50, 4, 2000 and 36 / 1574 / 325 / 3000 / 3301, conventions of this
    project that are fitted to nothing. count_secondary: flag-256 records count; min_mapq: a record counts only with at least this
    mapping quality (the records' `res`, as runs made with output_options(mapq=True) fill it)"""
    o = capi.SvcallOptions()
    o.count_secondary = 1 if count_secondary else 0
    o.min_mapq, o.flank, o.min_depth, o.min_qual = int(min_mapq), int(flank), int(min_depth), int(min_qual)
    o.cost_match, o.cost_mismatch, o.cost_het, o.prior_het, o.prior_hom = int(cost_match), int(cost_mismatch), int(cost_het), int(prior_het), int(prior_hom)
    return o


def _sv_clusters(clusters):
    return np.ascontiguousarray(np.asarray(clusters, dtype=SV_CLUSTER_DTYPE))


def svcall_host(lengths, records, cigar_words, clusters, options=None):
    """the rule alone on the host (flx_svcall_host): the rows of the clusters over the records, a structured array of SVCALL_ROW_DTYPE"""
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
    rec, words = _records_and_words(records, cigar_words)
    cl = _sv_clusters(clusters)
    opt = C.byref(options) if options is not None else None
    args = (ptr(lens, u64p) if len(lens) else None, len(lens), opt, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p) if len(words) else None,
            len(words), cl.ctypes.data_as(C.POINTER(capi.SvCluster)) if len(cl) else None, len(cl))
    n = C.c_uint64(0)
    rc = lib().flx_svcall_host(*args, None, C.byref(n))
    if rc not in (0, -3):                                               # (FLX_ERR_CAPACITY: n holds the need)
        check(rc)
    out = np.zeros(max(1, n.value), dtype=SVCALL_ROW_DTYPE)
    check(lib().flx_svcall_host(*args, out.ctypes.data_as(C.POINTER(capi.SvcallRow)), C.byref(n)))
    return out[: n.value]


SVCALL_SPAN_DTYPE = np.dtype([("ref", "<i4"), ("rs", "<u4"), ("re", "<u4"), ("res", "<u4")])


def svcaller_geometry():
    """a test hook: the most blocks of an svcall_spans launch and of an svcall_count launch, the waves of a block (a wave takes one record
    or one row at a time), and the sort's tile in keys"""
    out = np.zeros(4, dtype=np.uint32)
    check(lib().flx_svcaller_geometry(ptr(out, u32p)))
    return dict(spans_grid_cap=int(out[0]), count_grid_cap=int(out[1]), waves_per_block=int(out[2]), sort_tile=int(out[3]))


class svcaller:
    """Structural-variant calls over the sequences of a context's index (ctx) or over `lengths` on `device` (-1: the host form, which
    touches nothing of the device): every run's records are added as spans, the objects of other devices absorbed, and finish(clusters)
    genotypes the DEL and INS clusters of an sv object fed the same runs; then read rows() and spans(). Adds may come from several
    threads. initial_capacity: the spans the table holds before it first grows (a test hook; 0 takes 2^16)."""

    def __init__(self, ctx=None, options=None, lengths=None, device=0, initial_capacity=0):
        self.h = C.c_void_p()
        self.min_mapq = int(options.min_mapq) if options is not None else 0
        opt = C.byref(options) if options is not None else None
        if ctx is not None:
            check(lib().flx_svcaller_create(ctx.h, opt, C.byref(self.h)))
        else:
            if lengths is None:
                raise FloxerError("svcaller needs a context or a list of reference lengths")
            lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64))
            check(lib().flx_svcaller_create_for_lengths(int(device), ptr(lens, u64p) if len(lens) else None, len(lens), opt, int(initial_capacity), C.byref(self.h)))

    def close(self):
        if self.h:
            lib().flx_svcaller_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, run):
        """run: a RunResult (its records and CIGAR words are added), or a raw flx_run handle (ctypes.c_void_p) that has not been freed.
        With min_mapq a run made without output_options(mapq=True) is refused."""
        if isinstance(run, RunResult):
            if self.min_mapq > 0 and run.has_mapq is False:
                raise FloxerError("svcaller.add: min_mapq needs a run made with output_options(mapq=True)")
            return self.add_records(run.raw, run.cigars)
        check(lib().flx_svcaller_add_run(self.h, run))

    def add_records(self, records, cigar_words):
        """records: an array of the C ABI's flx_record (RunResult.raw's dtype); cigar_words: the uint32 pool their offsets refer to"""
        rec, words = _records_and_words(records, cigar_words)
        check(lib().flx_svcaller_add_records(self.h, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p) if len(words) else None, len(words)))

    def absorb(self, other):
        check(lib().flx_svcaller_absorb(self.h, other.h))

    def finish(self, clusters):
        """clusters: sv.clusters() of an sv object fed the same runs (a structured array of SV_CLUSTER_DTYPE). Final."""
        cl = _sv_clusters(clusters)
        check(lib().flx_svcaller_finish(self.h, cl.ctypes.data_as(C.POINTER(capi.SvCluster)) if len(cl) else None, len(cl)))

    def max_span(self):
        return int(lib().flx_svcaller_max_span(self.h))

    def spans(self):
        """all spans in (ref, rs, re) order: a structured array of SVCALL_SPAN_DTYPE"""
        check(lib().flx_svcaller_copy_spans(self.h, 0, 0, None))       # (refused before finish)
        n = lib().flx_svcaller_num_spans(self.h)
        out = np.zeros(max(1, n), dtype=SVCALL_SPAN_DTYPE)
        check(lib().flx_svcaller_copy_spans(self.h, 0, n, out.ctypes.data_as(C.POINTER(capi.SvcallSpan))))
        return out[:n]

    def rows(self):
        """one row per DEL / INS cluster in the clusters' order: a structured array of SVCALL_ROW_DTYPE"""
        n = lib().flx_svcaller_num_rows(self.h)
        out = np.zeros(max(1, n), dtype=SVCALL_ROW_DTYPE)
        check(lib().flx_svcaller_copy_rows(self.h, out.ctypes.data_as(C.POINTER(capi.SvcallRow)), n))
        return out[:n]


# ------------------------------------------------------------------------------------------------ coordinate order of records
SORT_ENTRY_DTYPE = np.dtype([("ordinal", "<u8"), ("ref", "<i4"), ("pos", "<i4"), ("end", "<u4"), ("flag", "<u4")])


def sort_options(initial_capacity=0, tile_keys=0):
    """flx_sort_options, both test hooks (0: the default): initial_capacity: the records the key table holds before it first grows;
    tile_keys: the keys one block orders per pass, a multiple of the block's threads"""
    o = capi.SortOptions()
    o.initial_capacity = int(initial_capacity)
    o.tile_keys = int(tile_keys)
    return o


def sort_geometry():
    """(default keys per tile, bits per digit, default initial capacity, entries per tile of the digit table's scan): a test hook"""
    g = np.zeros(4, dtype=np.uint32)
    check(lib().flx_sort_geometry(ptr(g, u32p)))
    return tuple(int(x) for x in g)


GRID_CAP_NAMES = ("md_build", "cs_build", "cigar_left_align", "cigar_tails", "ed_extend", "cigar_realign", "paf_summarise", "coverage_add", "pileup_add",
                  "sv_extract", "sort_keys_add", "errprof_add", "sort_census", "sort_strided", "sv_strided")


def grid_caps():
    """name -> the most blocks that launch asks for (behind them a wave or a thread takes further jobs in turns): a test hook. The
    first seven have one wave per block, the next five four waves with a record each, the last three 256 threads with an element each"""
    g = np.zeros(16, dtype=np.uint32)
    check(lib().flx_grid_caps(ptr(g, u32p)))
    return {name: int(g[i]) for i, name in enumerate(GRID_CAP_NAMES)}


class record_sorter:
    """The coordinate order of the records of runs: add records (record i of an add has ordinal first_ordinal + i), finish once, then
    read entries(a, b). Not floxer's. device=-1 opens no device and orders on the host (for machines without a GPU). Adds may come from
    several threads at once."""

    def __init__(self, n_refs, device=0, options=None):
        self.h = C.c_void_p()
        check(lib().flx_sort_create(int(device), int(n_refs), C.byref(options) if options is not None else None, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().flx_sort_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(lib().flx_sort_num_records(self.h))

    def add_records(self, records, cigar_words, first_ordinal, want_order=True):
        """records: an array of the C ABI's flx_record (RunResult.raw's dtype); cigar_words: the uint32 pool their offsets refer to.
        Returns the add's own records in key order, as indices into `records` (None with want_order=False)."""
        rec, words = _records_and_words(records, cigar_words)
        order = np.zeros(max(1, len(rec)), dtype=np.uint32) if want_order else None
        check(lib().flx_sort_add_records(self.h, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p), len(words), int(first_ordinal),
                                         ptr(order, u32p) if want_order else None))
        return order[: len(rec)] if want_order else None

    def add(self, run, first_ordinal, want_order=True):
        """run: a RunResult (its records and CIGAR words are added), or a raw flx_run handle (ctypes.c_void_p) that has not been freed"""
        if isinstance(run, RunResult):
            return self.add_records(run.raw, run.cigars, first_ordinal, want_order)
        n = int(lib().flx_run_num_records(run))
        order = np.zeros(max(1, n), dtype=np.uint32) if want_order else None
        check(lib().flx_sort_add_run(self.h, run, int(first_ordinal), ptr(order, u32p) if want_order else None))
        return order[:n] if want_order else None

    def finish(self):
        check(lib().flx_sort_finish(self.h))

    def entries(self, a=0, b=None):
        """the sorted entries [a, b) behind finish: a structured array of SORT_ENTRY_DTYPE (an unplaced record's ref is -1)"""
        b = len(self) if b is None else int(b)
        out = np.zeros(max(1, b - int(a)), dtype=SORT_ENTRY_DTYPE)
        check(lib().flx_sort_copy(self.h, int(a), b, out.ctypes.data_as(C.POINTER(capi.SortEntry))))
        return out[: max(0, b - int(a))]


def sort_host(n_refs, records, cigar_words, ordinals):
    """the rule alone on the host (flx_sort_host): record i has ordinal ordinals[i]; the entries in key order"""
    rec, words = _records_and_words(records, cigar_words)
    ords = np.ascontiguousarray(np.asarray(ordinals, dtype=np.uint64))
    if len(ords) != len(rec):
        raise FloxerError("sort_host: one ordinal per record")
    out = np.zeros(max(1, len(rec)), dtype=SORT_ENTRY_DTYPE)
    check(lib().flx_sort_host(int(n_refs), rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p), len(words), ptr(ords, u64p),
                              out.ctypes.data_as(C.POINTER(capi.SortEntry))))
    return out[: len(rec)]


# ------------------------------------------------------------------------------------------------ PAF output
PAF_SUMMARY_DTYPE = np.dtype([(n, "<u4") for n in ("query_start", "query_end", "ref_end", "matches", "mismatches", "ins_bases", "del_bases", "gap_opens")])


def _read_offsets(read_lengths):
    lens = np.asarray(read_lengths, dtype=np.uint64)
    offs = np.zeros(len(lens) + 1, dtype=np.uint64)
    if len(lens):
        offs[1:] = np.cumsum(lens)
    return offs


def _paf_call(fn, head, records, cigar_words, read_lengths, ref_lens, out):
    rec, words = _records_and_words(records, cigar_words)
    offs = _read_offsets(read_lengths)
    lens = np.ascontiguousarray(np.asarray(ref_lens, dtype=np.uint64))
    if out is None:
        out = np.zeros(max(1, len(rec)), dtype=PAF_SUMMARY_DTYPE)
    elif out.dtype != PAF_SUMMARY_DTYPE or not out.flags["C_CONTIGUOUS"] or len(out) < len(rec):
        raise FloxerError("paf: out must be a contiguous PAF_SUMMARY_DTYPE array with one entry per record")
    check(fn(*head, rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p) if len(words) else None, len(words), ptr(offs, u64p), len(offs) - 1,
             ptr(lens, u64p) if len(lens) else None, len(lens), out.ctypes.data_as(C.POINTER(capi.PafSummary))))
    return out[: len(rec)]


class paf:
    """Per-record PAF summaries (query interval, reference end, matching columns, block length, gap opens), reduced on `device` from the
    records' CIGAR words. Not floxer's. device=-1 opens no device and applies the host rule (for machines without a GPU). Calls may
    come from several threads; they are serialised inside the object."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        check(lib().flx_paf_create(int(device), C.byref(self.h)))

    def close(self):
        if self.h:
            lib().flx_paf_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def summarize(self, records, cigar_words, read_lengths, ref_lens, out=None):
        """records: an array of the C ABI's flx_record (RunResult.raw's dtype); cigar_words: the uint32 pool their offsets refer to;
        read_lengths: one entry per read of the batch, indexed by the records' `read`; ref_lens: the reference sequences' lengths.
        Returns a structured array of PAF_SUMMARY_DTYPE, one entry per record (all zeros for an unmapped record); out: such an array
        to fill. A refused call (FloxerError) leaves `out` as it was."""
        return _paf_call(lib().flx_paf_summarize, (self.h,), records, cigar_words, read_lengths, ref_lens, out)


def paf_summarize_host(records, cigar_words, read_lengths, ref_lens, out=None):
    """the rule alone on the host (flx_paf_summarize_host); arguments and result as paf.summarize"""
    return _paf_call(lib().flx_paf_summarize_host, (), records, cigar_words, read_lengths, ref_lens, out)


def paf_options(write_cigar=False, write_unmapped=False, mapq_from_records=False, skip_secondary=False):
    """flx_paf_options: write_cigar: a cg:Z tag with the record's own words (= and X kept, S included); write_unmapped: a line for
    every unmapped record (minimap2's --paf-no-hit form); mapq_from_records: column 12 from the records instead of 255;
    skip_secondary: records with flag 256 produce no line"""
    o = capi.PafOptions()
    o.write_cigar, o.write_unmapped = int(bool(write_cigar)), int(bool(write_unmapped))
    o.mapq_from_records, o.skip_secondary = int(bool(mapq_from_records)), int(bool(skip_secondary))
    return o


class paf_writer:
    """A PAF file (flx_paf_open): write(...) appends one line per mapped record in call order. Host only."""

    def __init__(self, path, ref_ids, ref_lens, options=None):
        self.h = C.c_void_p()
        ids = [r.encode() if isinstance(r, str) else bytes(r) for r in ref_ids]
        arr = (C.c_char_p * max(1, len(ids)))(*ids)
        lens = np.ascontiguousarray(np.asarray(ref_lens, dtype=np.uint64))
        if len(lens) != len(ids):
            raise FloxerError("paf_writer: one length per reference id")
        check(lib().flx_paf_open(str(path).encode(), arr, ptr(lens, u64p) if len(lens) else None, len(ids), C.byref(options) if options is not None else None,
                                 C.byref(self.h)))

    def write(self, read_ids, read_lengths, records, cigar_words, summaries, scores=None, cs_refs=None, cs_bytes=None):
        """read_ids / read_lengths: one entry per read of the batch; summaries: paf.summarize's result for `records`; scores: int32 per
        record (RunResult.scores) for AS:i; cs_refs / cs_bytes: RunResult.cs_refs and RunResult.cs_bytes for cs:Z"""
        rec, words = _records_and_words(records, cigar_words)
        ids = [r.encode() if isinstance(r, str) else bytes(r) for r in read_ids]
        arr = (C.c_char_p * max(1, len(ids)))(*ids)
        offs = _read_offsets(read_lengths)
        summ = np.ascontiguousarray(summaries, dtype=PAF_SUMMARY_DTYPE)
        if len(summ) != len(rec):
            raise FloxerError("paf_writer.write: one summary per record")
        sc = np.ascontiguousarray(scores, dtype=np.int32) if scores is not None else None
        refs = cs = None
        if cs_refs is not None:
            refs = np.zeros(max(1, len(rec)), dtype=_MD_DTYPE)
            r2 = np.asarray(cs_refs)
            if len(r2):
                if r2.dtype.names:
                    refs[: len(rec)] = r2
                else:
                    refs["off"][: len(rec)], refs["len"][: len(rec)] = r2[:, 0], r2[:, 1]
            cs = as_u8(cs_bytes) if cs_bytes is not None and len(cs_bytes) else np.zeros(1, np.uint8)
        check(lib().flx_paf_write(self.h, arr, ptr(offs, u64p), rec.ctypes.data_as(C.POINTER(capi.Record)), len(rec), ptr(words, u32p) if len(words) else None,
                                  summ.ctypes.data_as(C.POINTER(capi.PafSummary)), sc.ctypes.data_as(C.POINTER(C.c_int32)) if sc is not None else None,
                                  refs.ctypes.data_as(C.POINTER(capi.MdRef)) if refs is not None else None, ptr(cs, u8p) if cs is not None else None))

    def close(self):
        if self.h:
            h, self.h = self.h, C.c_void_p()
            check(lib().flx_paf_close(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
