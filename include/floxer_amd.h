/*
 * floxer_amd — C ABI of the MI355X-native seed-and-verify path (libfloxer_amd.so).
 *
 * floxer has no plugin/FFI interface; its hot path sits behind four C++ seams. Each entry point
 * below replaces one of those seams and cites it. Conventions: caller owns every buffer; plain pointers + sizes; no
 * exceptions cross the boundary — every function returns FLX_OK (0) or a negative flx_status and flx_last_error()
 * describes the failure (the reference throws C++ exceptions that its task wrappers turn into a stop flag,
 * parallelization.cpp:149-157). A flx_ctx owns one HIP device, its HBM-resident index and a set of lanes (a HIP stream with
 * its workspaces each); calls on different contexts are independent. The compute calls (flx_search_seeds, flx_search_groups,
 * flx_align_batch, flx_align_reads*, flx_reads_upload) may be issued from several host threads on one context: each takes a
 * free lane and waits when there is none, so batches overlap on the GPU. Configuration calls (flx_ctx_set_stream,
 * flx_ctx_enable_kernel_timing, flx_ctx_reset_kernel_stats, flx_ctx_destroy) must not overlap anything else.
 *
 * Sequences are rank sequences as the reference stores them (input.cpp:165-176): $=0 A=1 C=2 G=3 T=4 N/other=5.
 * CIGARs are BAM words (len<<4|op) with ops I=1 D=2 '='=7 X=8 (extended CIGAR, alignment.cpp:178), and S=4 in partial records only.
 */
#ifndef FLOXER_AMD_H
#define FLOXER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum flx_status {
    FLX_OK = 0,
    FLX_ERR_INVALID = -1,      /* bad argument / shape */
    FLX_ERR_NO_DEVICE = -2,    /* no HIP device / HIP runtime failure: the product never falls back to a CPU path */
    FLX_ERR_CAPACITY = -3,     /* caller buffer too small; required size is reported through the size out-parameter */
    FLX_ERR_UNSUPPORTED = -4,
    FLX_ERR_INTERNAL = -5,
    FLX_ERR_IO = -6
} flx_status;

const char* flx_last_error(void);
const char* flx_version(void);

/* ------------------------------------------------------------------------------------------------ host-side arithmetic
 * math.hpp:10-27, input.cpp:26-34 — must be bit-identical incl. the double arithmetic, so it is host code. */
uint64_t flx_ceil_div(uint64_t a, uint64_t b);
uint64_t flx_floating_point_error_aware_ceil(double value);
int32_t flx_saturate_value_to_int32_max(uint64_t value);
/* input.cpp:161-176 + ivs::reverse_complement_rank (input.cpp:132) */
void flx_chars_to_rank_sequence(const char* chars, uint64_t n, uint8_t* out_ranks);
void flx_reverse_complement_rank(const uint8_t* ranks, uint64_t n, uint8_t* out_ranks);

/* ------------------------------------------------------------------------------------------------ PEX tree
 * replaces pex::pex_tree::pex_tree (pex.hpp:57-126, pex.cpp:84-256). Nodes: inner nodes first (root = inner[0], or
 * leaves[0] when the tree is a single node), then leaves. parent_id indexes the inner nodes; FLX_NULL_ID for the root. */
#define FLX_NULL_ID 0xFFFFFFFFu
typedef struct flx_pex_node {
    uint32_t parent_id;
    uint32_t from;        /* inclusive */
    uint32_t to;          /* inclusive */
    uint32_t num_errors;
} flx_pex_node;
int flx_pex_tree_build(uint64_t query_length, uint64_t query_num_errors, uint64_t leaf_max_num_errors, int bottom_up,
                       flx_pex_node* nodes, uint64_t capacity, uint64_t* n_inner, uint64_t* n_leaves);

/* ------------------------------------------------------------------------------------------------ index lifetime
 * replaces fmindex(refs, sampling_rate=4, threads) / load_index / save_index (floxer.cpp:62-107, input.cpp:150-157,
 * output.cpp:25-40). Built on the host; own versioned file format (not cereal-compatible). */
typedef struct flx_index flx_index;
int flx_index_build(const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs, flx_index** out);
/* The same index with its two suffix arrays built on a HIP device (prefix doubling with radix sorts instead of the host's SA-IS:
 * seconds instead of a minute for a chromosome-sized reference); 36 bytes of HBM per reference symbol while it runs. */
int flx_index_build_on_device(int hip_device, const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs, flx_index** out);
int flx_index_save(const flx_index* index, const char* path);
int flx_index_load(const char* path, flx_index** out);
void flx_index_free(flx_index* index);
uint64_t flx_index_text_length(const flx_index* index);     /* concatenated text incl. sentinel padding */
uint32_t flx_index_num_references(const flx_index* index);
uint64_t flx_index_device_bytes(const flx_index* index);    /* HBM footprint of the index image once uploaded */
/* what a context adds to the image when the device has room for it: the inverse suffix array (4 B per text symbol) and the presence
   filter of the seeding kernels (4^K / 8 bytes, K = ceil(log4 n) + 2); a context made without either gives the same results, slower */
uint64_t flx_index_derived_device_bytes(const flx_index* index);
/* FLX_OK iff the index was built from exactly these reference sequences (guards --index against a stale file, floxer.cpp:63-79) */
int flx_index_matches_reference(const flx_index* index, const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs);
/* test hooks: suffix array / BWT as built (text_length entries) */
int flx_index_copy_sa(const flx_index* index, uint64_t* out);
int flx_index_copy_sa_u32(const flx_index* index, uint32_t* out);   /* the same as stored (text < 2^32 symbols) */
int flx_index_copy_bwt(const flx_index* index, int reversed, uint8_t* out);

/* ------------------------------------------------------------------------------------------------ device context */
typedef struct flx_ctx flx_ctx;
int flx_device_count(void);                                  /* HIP devices visible to the process (0: none / no runtime) */
int flx_ctx_create(int hip_device, const flx_index* index, flx_ctx** out);   /* uploads index + reference text to HBM */
/* Refused (FLX_ERR_INVALID, the context stays as it is and usable) while a read batch made on it with flx_reads_upload has not been
 * freed: a batch hands its device buffers back to its context when it is freed. NULL: FLX_OK. */
int flx_ctx_destroy(flx_ctx* ctx);
/* Index replicas across the GPUs of a job (the FM index is replicated per GPU). The HBM image of an index is five
 * device buffers (occurrence table of the text, of the reversed text, suffix array, text with its guard bytes, k-mer table). A rank
 * that built or loaded the index uploads the image into buffers it owns (flx_index_image_upload), sends them to the other ranks
 * (RCCL broadcast over xGMI: floxer_amd/distributed.py) together with the small host part (flx_index_meta_export), and every rank
 * makes its context on its copy (flx_ctx_create_on_image; the buffers must outlive the context): no rank but the first holds the
 * index in host memory, builds it or reads it from a file. */
typedef struct flx_index_image { uint64_t bytes[5]; } flx_index_image;
int flx_index_image_layout(const flx_index* index, flx_index_image* out);
int flx_index_image_upload(const flx_index* index, int hip_device, void* const device_buffers[5]);
int flx_index_meta_export(const flx_index* index, uint8_t* buf, uint64_t* len /* in: capacity, out: needed */);
int flx_index_meta_import(const uint8_t* buf, uint64_t len, flx_index** out);   /* an index without arrays: for flx_ctx_create_on_image */
/* sizes: the bytes the caller's five buffers hold; they must be the index's layout (a stale image, e.g. of another build's block size,
 * is refused instead of read out of bounds) */
int flx_ctx_create_on_image(int hip_device, const flx_index* index, void* const device_buffers[5], const flx_index_image* sizes, flx_ctx** out);
/* use a caller-owned HIP stream (hipStream_t passed as void*) for all launches; NULL restores the context's own stream */
int flx_ctx_set_stream(flx_ctx* ctx, void* hip_stream);

/* ------------------------------------------------------------------------------------------------ seam 1: seeding
 * replaces search_result searcher::search_seeds(std::vector<seed> const&) const (search.hpp:104-112, search.cpp:143-324) */
typedef struct flx_seed {            /* search::seed, search.hpp:17-22 */
    uint64_t seq_offset;             /* into the sequence pool */
    uint32_t length;
    uint32_t num_errors;             /* 0..3 */
    uint32_t pex_leaf_index;
    uint32_t reserved;
} flx_seed;

enum { FLX_ORDER_ERRORS_FIRST = 0, FLX_ORDER_COUNT_FIRST = 1, FLX_ORDER_NONE = 2 };             /* search.hpp:44-46 */
enum { FLX_CHOICE_ROUND_ROBIN = 0, FLX_CHOICE_FULL_GROUPS = 1, FLX_CHOICE_FIRST_REPORTED = 2 };  /* search.hpp:50-52 */

typedef struct flx_search_config {   /* search::search_config, search.hpp:56-62; defaults floxer_cli.hpp:52-56 */
    uint64_t max_num_anchors_hard;
    uint64_t max_num_anchors_soft;
    int32_t anchor_group_order;
    int32_t anchor_choice_strategy;
    int32_t erase_useless_anchors;
    int32_t reserved;
} flx_search_config;

typedef struct flx_anchor {          /* search::anchor_t, search.hpp:27-38 */
    uint32_t seed_index;             /* index into the seeds array of the call */
    uint32_t pex_leaf_index;
    uint32_t reference_id;
    uint32_t num_errors;
    uint64_t reference_position;
} flx_anchor;

typedef struct flx_seed_stats {      /* search_result::anchors_of_seed, search.hpp:80-87 */
    uint32_t num_kept_useful_anchors;
    uint32_t num_kept_raw_anchors;
    uint32_t num_excluded_raw_anchors_by_soft_cap;
    uint32_t fully_excluded;
} flx_seed_stats;

/* anchors are written in search_result::anchor_iterator order (seed, reference, position; search.cpp:78-100).
 * n_anchors: in = capacity, out = number produced (FLX_ERR_CAPACITY if larger than capacity). */
int flx_search_seeds(flx_ctx* ctx, const uint8_t* seq_pool, uint64_t seq_pool_len, const flx_seed* seeds, uint64_t n_seeds,
                     const flx_search_config* cfg, flx_anchor* out_anchors, uint64_t* n_anchors, flx_seed_stats* out_stats);

/* raw search_ng21::search_n emission for the seeds (test hook for kernel K1): rows {seed_index, lb, len, errors} */
typedef struct flx_hit_group { uint32_t seed_index, lb, len, num_errors; } flx_hit_group;
int flx_search_groups(flx_ctx* ctx, const uint8_t* seq_pool, uint64_t seq_pool_len, const flx_seed* seeds, uint64_t n_seeds,
                      uint64_t max_hits_per_seed, flx_hit_group* out, uint64_t* n_out);

/* ------------------------------------------------------------------------------------------------ seam 2: alignment
 * replaces alignment_result align(span<const u8> reference, span<const u8> query, alignment_config const&)
 * (alignment.hpp:57-77, alignment.cpp:83-181), batched. */
enum { FLX_MODE_EXISTS = 0, FLX_MODE_WITHOUT_CIGAR = 1, FLX_MODE_WITH_CIGAR = 2 };                /* alignment.hpp:53-55 */
typedef struct flx_align_job {
    uint64_t ref_offset;     /* into ref_pool, or into the context's reference text when ref_pool == NULL */
    uint64_t query_offset;   /* into query_pool */
    uint32_t ref_length;
    uint32_t query_length;
    uint32_t num_allowed_errors;
    uint32_t mode;
} flx_align_job;
typedef struct flx_align_result {
    uint32_t exists;         /* alignment_outcome::alignment_exists */
    uint32_t num_errors;
    uint64_t begin;          /* start in the given reference window (caller adds reference_span_offset) */
    uint64_t cigar_offset;   /* into cigar_pool (words) */
    uint32_t cigar_length;
    uint32_t reserved;
} flx_align_result;
int flx_align_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool,
                    uint64_t query_pool_len, const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out,
                    uint32_t* cigar_pool, uint64_t* cigar_pool_words /* in: capacity, out: used */);

/* The launch shape flx_align_batch would give every job of a call with these jobs (a diagnostic and test hook; host arithmetic only: no
 * context, no GPU). The kernels run a job on a ring of lanes_per_job lanes, words_per_lane 64-row words of the query per lane;
 * queue = the hand-over slots the job's ring occupies in LDS, 0 for a ring that never waits for a lane. */
typedef struct flx_align_shape { uint32_t words_per_lane, lanes_per_job, queue; } flx_align_shape;
int flx_align_shapes(const flx_align_job* jobs, uint64_t n_jobs, flx_align_shape* out);

/* flx_align_batch plus the MD string (see flx_tag_options) of every WITH_CIGAR job that exists: out_md[i] refers into md_pool, length 0 for
 * every other job. md_pool_bytes: in = capacity, out = used (FLX_ERR_CAPACITY if larger than the capacity; 8 * num_allowed_errors + 6 bytes
 * per WITH_CIGAR job always suffice). */
typedef struct flx_md_ref { uint64_t offset; uint32_t length; uint32_t reserved; } flx_md_ref;   /* into the MD bytes; length 0: the record has no MD */
int flx_align_batch_md(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool,
                       uint64_t query_pool_len, const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out,
                       uint32_t* cigar_pool, uint64_t* cigar_pool_words, flx_md_ref* out_md, uint8_t* md_pool, uint64_t* md_pool_bytes);

/* ------------------------------------------------------------------------------------------------ seam 3: whole path
 * replaces parallelization::spawn_search_task + spawn_verification_task + query_verifier::verify +
 * alignment_output::write_alignments_for_query (parallelization.cpp:45-293, verification.hpp:22-48, output.cpp:49-108)
 * for a batch of reads, with --threads 1 record order. */
typedef struct flx_params {          /* cli::command_line_input, floxer_cli.hpp:41-70 */
    double query_error_probability;  /* < 0: use query_num_errors */
    uint64_t query_num_errors;
    uint64_t pex_seed_num_errors;    /* default 2 */
    flx_search_config search;
    uint64_t seed_sampling_step_size;/* default 1 */
    int32_t bottom_up_pex_tree_building;
    int32_t use_interval_optimization;
    double extra_verification_ratio; /* default 0.05 */
    int32_t direct_full_verification;
    int32_t without_cigar;
    uint64_t num_anchors_per_verification_task;   /* default 3000 */
} flx_params;
void flx_params_default(flx_params* p);

typedef struct flx_record {          /* one SAM/BAM record, output.cpp:49-108 */
    uint64_t read_index;
    uint32_t flag;                   /* 0 / 16 / 256 / 272 / 4; 2048 / 2064 with flx_partial_options */
    int32_t reference_id;            /* -1 when unmapped */
    int32_t position;                /* 0-based, saturated to int32 (output.cpp:85) */
    uint32_t num_errors;             /* NM */
    uint64_t cigar_offset;
    uint32_t cigar_length;
    uint32_t reserved;               /* MAPQ when the run was made with flx_output_options.mapq, else 0 */
} flx_record;

typedef struct flx_run flx_run;      /* result of one batch */
/* Reads are given as one rank pool; read i = pool[offsets[i], offsets[i+1]). The read filters of input.cpp:95-129 apply
 * (filtered reads produce no record and are flagged in the skipped array). */
int flx_align_reads(flx_ctx* ctx, const flx_params* params, const uint8_t* read_pool, const uint64_t* read_offsets,
                    uint64_t n_reads, flx_run** out);
/* The same with the reads already resident in HBM (the measured configuration of bench.py): upload once, align many times. */
typedef struct flx_reads flx_reads;
int flx_reads_upload(flx_ctx* ctx, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads, flx_reads** out);
/* Free a batch only after every run on it has returned (its device buffers are reused by the next batch without a device-wide wait),
 * and before its context is destroyed. */
void flx_reads_free(flx_reads* reads);
int flx_align_reads_resident(flx_ctx* ctx, const flx_params* params, const flx_reads* reads, flx_run** out);

/* Output options: not floxer's, which writes every alignment verification found (alignment.cpp:39-46, output.cpp:48). All are off
 * when the struct is zeroed, and with all off the records are floxer's, byte for byte. Applied per read to its records in output
 * order (per reference id ascending, verification order within a reference):
 *   drop_duplicates != 0: of the mapped records with equal reference id, strand (flag bit 16), start, NM and CIGAR words (compared
 *     word by word) only the first is kept: floxer's alignment operator== (alignment.cpp:20-34) plus the reference id;
 *   max_alignments_per_read = N > 0: of the mapped records left, the N with the smallest (NM, index in output order) are kept and
 *     written in their original order; N = 1 keeps exactly the primary.
 *   mapq = 1 (0: off, anything else is refused): flx_record.reserved of every record receives a mapping quality made of the read's
 *     distinct loci, computed from all of the read's records before the two options above select among them, so that the primary
 *     kept by max_alignments_per_read = 1 tells of the loci that were dropped. Records that overlap on one (reference, strand) are one
 *     locus with the smallest NM of its records; with b the NM of the primary's locus, n the loci of that NM and s the next larger NM
 *     of a locus: n >= 2 gives 3, 2, 1 for n = 2, 3, 4 and 0 beyond, a single locus 60, else min(60, 10 * (s - b)) (the factor 10 is
 *     this project's convention, not fitted to anything). The records of the primary's locus get the value, all others 0. The full
 *     rule and its limits: floxer_amd/csrc/flx_mapq.hpp. No other field of any record changes.
 * Kept records are unchanged (no flag is rewritten); the unmapped record of a read without alignments is always kept. --stats and
 * flx_path_counters.root_alignments_found still describe what verification found; flx_path_counters.records counts records written
 * and reserved[0] the records dropped. The reserved fields must be 0. */
typedef struct flx_output_options {
    uint32_t drop_duplicates;
    uint32_t mapq;
    uint64_t max_alignments_per_read;    /* 0: no cap */
    uint64_t reserved2[2];
} flx_output_options;
/* flx_align_reads / flx_align_reads_resident with output options (NULL: none, the same as the calls without them) */
int flx_align_reads_with_options(flx_ctx* ctx, const flx_params* params, const uint8_t* read_pool, const uint64_t* read_offsets,
                                 uint64_t n_reads, const flx_output_options* options, flx_run** out);
int flx_align_reads_resident_with_options(flx_ctx* ctx, const flx_params* params, const flx_reads* reads,
                                          const flx_output_options* options, flx_run** out);
/* The same rule on any record array (host only): the records of a read are contiguous and in output order, as in every flx_run.
 * keep[i] = 1 when record i is kept, else 0. Starts compare by `position` (the pipeline compares the unsaturated start; the two
 * differ only for sequences of 2^31 symbols or more). cigar_words may be NULL when no record has a CIGAR. */
int flx_select_records(const flx_record* records, uint64_t n, const uint32_t* cigar_words, const flx_output_options* options,
                       uint8_t* keep);
/* The mapq rule on any record array (host only; records as for flx_select_records, the records' `reserved` is not read): mapq[i]
 * receives record i's mapping quality. Call it on all of a read's records, before any selection. A record without CIGAR spans
 * read_lengths[read_index] reference symbols; read_lengths may be NULL: then the span comes from the CIGAR only (1 without one). */
int flx_assign_mapq(const flx_record* records, uint64_t n, const uint32_t* cigar_words, const uint64_t* read_lengths, uint8_t* mapq);

/* Optional tags: not floxer's, which writes NM only. All are off when the struct is zeroed (or NULL), and with all off nothing changes: no
 * launch, no byte of any output.
 *   md = 1 (0: off, anything else is refused): every mapped record of the run gets an MD string (SAM spec, the rule of samtools calmd on the
 *     record's extended CIGAR): walk the reference-consuming columns from the record's position; '=' columns increment a counter; every X
 *     column emits the counter (decimal, possibly 0), the reference letter, and resets the counter; every D op emits the counter, '^', the
 *     op's reference letters, and resets the counter; I emits nothing; the end emits the counter ("10A5^AC6"; X X gives A0C, D then X gives
 *     ^AC0T). Letters come from the index's ranks: 1..4 -> ACGT, anything else N: IUPAC and lower-case letters of the FASTA are not
 *     recoverable. Reference-forward orientation for both strands. The strings are built on the device next to the CIGARs (a context made
 *     on an index image has no host text). Records that share a CIGAR share their MD bytes. params->without_cigar has no trace: md together
 *     with it is refused (FLX_ERR_INVALID) before any work. Output options select records together with their MD; the MD bytes of dropped
 *     records stay in the pool (it is not compacted). The reserved fields must be 0. */
typedef struct flx_tag_options { uint32_t md; uint32_t reserved[7]; } flx_tag_options;
int flx_align_reads_with_tags(flx_ctx* ctx, const flx_params* params, const uint8_t* read_pool, const uint64_t* read_offsets,
                              uint64_t n_reads, const flx_output_options* options, const flx_tag_options* tags, flx_run** out);
int flx_align_reads_resident_with_tags(flx_ctx* ctx, const flx_params* params, const flx_reads* reads, const flx_output_options* options,
                                       const flx_tag_options* tags, flx_run** out);
uint64_t flx_run_num_md_bytes(const flx_run* run);                   /* 0 for a run made without md */
/* refs: one per record, in record order; md_bytes: flx_run_num_md_bytes bytes (what lies between the strings is unspecified). Either may be NULL. A run made without md: FLX_ERR_INVALID. */
int flx_run_copy_md(const flx_run* run, flx_md_ref* refs, uint8_t* md_bytes);

/* Partial alignments: not floxer's, which maps a read only when its whole length aligns within its errors (a chimeric read, or one
 * across a structural break, is written as unmapped). Off when the struct is zeroed (or NULL), and then nothing changes: no launch, no
 * byte of any output. With enable = 1 (anything else but 0 is refused) a read that is not skipped and that has no mapped record gets,
 * in place of its unmapped record, the largest parts of it that verification proved to align, as soft-clipped records:
 *   - candidate of an anchor: the highest PEX node on its leaf-to-root path that it passed - the child, on that path, of the node it
 *     failed at (the leaf itself when its first inner node failed; a leaf counts as passed), or the child of the root when the anchor
 *     reached the root and the root alignment failed. With params->direct_full_verification nothing climbs: the candidates are leaves;
 *   - it counts when its node has at least min_query_span rows (0: the default 1000, a convention of this project, not fitted to
 *     anything), and is traced in exactly the window it was tested in (no extension, k = the node's errors): an alignment exists.
 *     Identical (orientation, node, reference, window) candidates are traced once, overlapping windows of a node share one DP as root
 *     windows do, with MD strings when flx_tag_options.md is on;
 *   - per read (query intervals in read-forward coordinates: node [from, to] of the reverse complement is [len-1-to, len-1-from]):
 *     candidates equal to an earlier one in (orientation, reference, start, NM, CIGAR words) are dropped, the others ordered by (rows
 *     descending, NM ascending, reference id, verification order) and taken greedily: the first is the primary (flag 0 / 16), a later
 *     one is kept as supplementary (flag 2048 | strand) when its interval overlaps no kept one, until max_records (0: the default 4)
 *     are kept. They are written primary first, then the supplementaries by forward query start;
 *   - a kept record: position = the reference start of the aligned part, num_errors = its NM (clipped bases are not counted), CIGAR =
 *     [from]S + the traced words + [rows behind the node]S in the oriented sequence (zero-length clips omitted), MD of the traced part.
 * Output options: drop_duplicates and max_alignments_per_read leave a read's partial records alone (they are selected already;
 * flx_select_records keeps all records of a read that has a flag-2048 record); mapq gives each kept record read_mapq's value over the
 * read's traced candidates with exactly its forward query interval. params->without_cigar has no trace: refused together with enable
 * (FLX_ERR_INVALID) before any work. --stats and every named flx_path_counters field keep describing verification; reserved[1] counts
 * the partial records written and reserved[2] the reads that got them. Each record ends at a PEX node's boundary unless
 * flx_extend_options moves its ends to the break; the SA tag is the writer's (flx_sam_set_sa). The rule and its limits:
 * floxer_amd/csrc/flx_partial.hpp. */
typedef struct flx_partial_options {
    uint32_t enable;
    uint32_t min_query_span;     /* 0: 1000 */
    uint32_t max_records;        /* 0: 4 */
    uint32_t reserved[5];
} flx_partial_options;
/* Extension of the partial records to the break: not floxer's. Off when the struct is zeroed (or NULL), and then nothing changes: no
 * launch, no byte of any output. With enable = 1 (anything else but 0 is refused; it needs flx_partial_options.enable, else
 * FLX_ERR_INVALID before any work) both ends of every kept partial record are extended from the cell behind its traced part, as far
 * as the sequence keeps aligning (kernel ed_extend, one score-only wavefront job per end), and the records that moved are traced
 * again over the longer interval:
 *   - a job walks at most the rows up to the read's end, or up to the original node interval of the read's next kept record on that
 *     side, and at most the symbols up to the end of its reference sequence;
 *   - with D the unit-cost edit distance from the start cell, m(i) = min_j D[i][j], R(d) = max{i : m(i) <= d} and
 *     score(d) = R(d) - error_weight * d, it scans d = 0, 1, .. and stops at the first d with (running maximum - score(d)) > x_drop,
 *     R(d) = the row limit, or d = max_errors; the end moves by R(d*) rows and j* symbols at d* errors, d* the first d of the maximum
 *     and j* the smallest j with D[R(d*)][j] = d*;
 *   - error_weight (0: 4), x_drop (0: 100) and max_errors (0: 1024) are conventions of this project, not fitted to anything; a peak
 *     behind a valley deeper than x_drop, or behind max_errors errors, is not found. max_errors above 4093 (what the kernel's two
 *     wavefronts hold in LDS), error_weight above 65535 and x_drop above 2^30 are refused.
 * A record that moved: query rows [from - iL, to + iR], reference window exactly [start - jL, end + jR], traced with nm + dL + dR
 * allowed errors; position, NM, CIGAR and MD come from that trace, the soft clips are what remains of the read; its mapping quality
 * (flx_output_options.mapq) keeps the value computed before the extension. Records that did not move keep their words. Flags, the
 * order of a read's records and the counters do not change. The full rule: floxer_amd/csrc/flx_partial.hpp. The reserved fields
 * must be 0. */
typedef struct flx_extend_options {
    uint32_t enable;
    uint32_t error_weight;       /* 0: 4 */
    uint32_t x_drop;             /* 0: 100 */
    uint32_t max_errors;         /* 0: 1024 */
    uint32_t reserved[4];
} flx_extend_options;
/* Every option of a run in one bundle: each pointer may be NULL (that option off). A NULL bundle, or one of NULLs / zeroed structs, is
 * exactly flx_align_reads / flx_align_reads_resident; the calls above forward here. The reserved pointers must be NULL. */
typedef struct flx_run_options {
    const flx_output_options* output;
    const flx_tag_options* tags;
    const flx_partial_options* partial;
    const flx_extend_options* extend;
    const void* reserved[4];
} flx_run_options;
int flx_align_reads_opt(flx_ctx* ctx, const flx_params* params, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads,
                        const flx_run_options* options, flx_run** out);
int flx_align_reads_resident_opt(flx_ctx* ctx, const flx_params* params, const flx_reads* reads, const flx_run_options* options, flx_run** out);
/* The selection on any candidate array (host only): the candidates of a read are contiguous and in verification order; q_from / q_to are
 * inclusive read-forward coordinates. keep_flag[i] = -1 when candidate i is not written, else its SAM flag (0 / 16 / 2048 / 2064).
 * cigar_words may be NULL: then CIGARs compare by (offset, length). options NULL: the defaults (enable is not read). */
typedef struct flx_partial_candidate {
    uint64_t read_index;
    uint32_t q_from, q_to;
    uint32_t orientation;        /* 0 forward, 1 reverse complement */
    int32_t reference_id;
    uint64_t start;              /* reference start of the aligned part */
    uint32_t nm;
    uint32_t cigar_length;
    uint64_t cigar_offset;
} flx_partial_candidate;
int flx_choose_partials(const flx_partial_candidate* candidates, uint64_t n, const uint32_t* cigar_words, const flx_partial_options* options,
                        int32_t* keep_flag);
/* the mapping quality of the kept candidates (keep_flag as flx_choose_partials gave it), 0 for the others. cigar_words NULL: a
 * candidate spans as many reference symbols as query rows. */
int flx_partial_mapq(const flx_partial_candidate* candidates, uint64_t n, const uint32_t* cigar_words, const int32_t* keep_flag, uint8_t* mapq);

/* The extension kernel alone (ed_extend), in the style of seam 2: one job per end. ref_pool == NULL: the context's reference text
 * (text_pos is then a position in the padded concatenated text). A job starts at reference symbol text_pos and query symbol q_pos
 * (the first column and row of its matrix) and walks both sequences upwards (direction +1) or downwards (-1) for at most ref_limit
 * symbols and row_limit rows, which must lie in their pools (row_limit < 2^19). error_weight, x_drop, max_errors: 0 takes the
 * defaults of flx_extend_options, with the same bounds. out[i]: the rows and columns the end moves by and the errors of that
 * extension (0, 0, 0: it does not move), and why the scan stopped. */
typedef struct flx_extend_job {
    uint64_t text_pos;
    uint64_t q_pos;
    uint32_t ref_limit;
    uint32_t row_limit;
    int32_t direction;           /* +1 or -1 */
    uint32_t error_weight;
    uint32_t x_drop;
    uint32_t max_errors;
} flx_extend_job;
enum { FLX_EXTEND_STOP_XDROP = 1, FLX_EXTEND_STOP_ROWS = 2, FLX_EXTEND_STOP_MAX_ERRORS = 3 };
typedef struct flx_extend_result { uint32_t rows, cols, errors, stop_reason; } flx_extend_result;
int flx_extend_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                     const flx_extend_job* jobs, uint64_t n_jobs, flx_extend_result* out);

/* Chimeric tails of reads that are mapped in full: not floxer's. A read whose whole length fits its errors is written as one record
 * even when its last few hundred bases belong elsewhere; the break then shows only as a run of X / I / D at one end of the CIGAR. Off
 * when the struct is zeroed (or NULL), and then nothing changes: no launch, no byte of any output. With enable = 1 (anything else but
 * 0 is refused) the rule below is applied to every root alignment's CIGAR on the device, behind the traceback (kernel cigar_tails), and
 * a read whose primary (the first record with the best NM in output order) has a tail is split:
 *   - the rule, on a CIGAR core of T words (ops = X I D): boundary t = 0..T lies behind word t; rows_t / cols_t count the query /
 *     reference consumed, err_t the lengths of X, I and D, S_t = rows_t - error_weight * err_t (signed 64-bit, S_0 = 0). Right tail:
 *     G = max S_t, t_R the smallest t with S_t = G; it exists iff G - S_T > x_drop and rows_T - rows_{t_R} >= min_tail_rows. Left
 *     tail: g = min S_t, t_L the largest t with S_t = g; it exists iff -g > x_drop and rows_{t_L} >= min_tail_rows. Both and
 *     t_L >= t_R: neither. Cuts fall on word boundaries. error_weight (0: 4) and x_drop (0: 100) are the extension's conventions,
 *     min_tail_rows (0: 100) is one of this project; none is fitted to anything. Bounds: error_weight <= 65535, x_drop <= 2^30,
 *     min_tail_rows < 2^19;
 *   - the kept part is traced again over the oriented rows [left_rows, len - 1 - right_rows] in exactly the reference window
 *     [start + left_cols, start + span - right_cols) with nm - left_errors - right_errors allowed errors; it is the primary (flag
 *     0 / 16) with the tails soft-clipped; position, NM, CIGAR and MD come from that trace;
 *   - tail candidates: for every anchor of the read in verification order the highest node on its leaf-to-root path that it passed
 *     (flx_partial_options; every node below the root for an anchor whose root alignment exists) and whose read-forward interval lies
 *     inside one tail's, with at least partial.min_query_span rows, traced in the window it was tested in. flx_choose_partials' rule
 *     over them with max_records - 1 keeps the supplementaries (flag 2048 | strand), written behind the primary by forward query
 *     start. A split read without candidate is its clipped primary alone;
 *   - flx_extend_options then carries every end of these records to the break under its own limits, the primary's cut ends included;
 *   - the read's root records are not written (they count in flx_path_counters.reserved[0]); with flx_output_options.mapq the
 *     primary keeps the value of the read's root records and the supplementaries get flx_partial_mapq's over the tail candidates.
 * It needs flx_partial_options.enable and flx_output_options.max_alignments_per_read == 1 (a tail is judged on the primary; full-length
 * secondaries beside a clipped primary would contradict it) and is refused with params->without_cigar: FLX_ERR_INVALID before any
 * work. Limits: a tail that holds a second good region behind a second break is cut once; a structural indel inside a read whose
 * score recovers afterwards is not a break. flx_path_counters.reserved[1] counts these records too, reserved[3] the reads split.
 * The rule: floxer_amd/csrc/flx_tails.hpp. The reserved fields must be 0. */
typedef struct flx_split_options {
    uint32_t enable;
    uint32_t error_weight;       /* 0: 4 */
    uint32_t x_drop;             /* 0: 100 */
    uint32_t min_tail_rows;      /* 0: 100 */
    uint32_t reserved[4];
} flx_split_options;
/* flx_align_reads_opt / flx_align_reads_resident_opt with the split options (NULL or zeroed: exactly those calls, which forward here) */
int flx_align_reads_split(flx_ctx* ctx, const flx_params* params, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads,
                          const flx_run_options* options, const flx_split_options* split, flx_run** out);
int flx_align_reads_resident_split(flx_ctx* ctx, const flx_params* params, const flx_reads* reads, const flx_run_options* options,
                                   const flx_split_options* split, flx_run** out);
/* The rule alone on any CIGAR words: job i covers words [cigar_offset, cigar_offset + cigar_length) of the pool; a zero in any of the
 * last three fields takes the default. An absent tail reports zeros. A job outside the pool, an op other than = X I D, op lengths that
 * sum to 2^32 or more, or a value beyond its bound is refused (FLX_ERR_INVALID; flx_cigar_tails_batch: before any launch).
 * flx_cigar_tails runs on the host, flx_cigar_tails_batch runs the kernel; both give the same numbers. */
typedef struct flx_tail_job {
    uint64_t cigar_offset;
    uint32_t cigar_length;
    uint32_t error_weight;
    uint32_t x_drop;
    uint32_t min_tail_rows;
} flx_tail_job;
typedef struct flx_tail_result { uint32_t left_rows, left_cols, left_errors, left_words, right_rows, right_cols, right_errors, right_words; } flx_tail_result;
int flx_cigar_tails(const uint32_t* cigar_words, uint64_t n_words, const flx_tail_job* jobs, uint64_t n_jobs, flx_tail_result* out);
int flx_cigar_tails_batch(flx_ctx* ctx, const uint32_t* cigar_words, uint64_t n_words, const flx_tail_job* jobs, uint64_t n_jobs, flx_tail_result* out);

/* Left-aligned indels: not floxer's. The traceback takes an up or left move as soon as one is valid, so inside a homopolymer or a tandem
 * repeat a gap lands on the last copy: every CIGAR has its gaps right-aligned, floxer's (seqan3's) convention and the default here.
 * Variant callers, VCF, minimap2 and bwa put a gap on the first copy. Off when the struct is zeroed (or NULL), and then nothing changes:
 * no launch, no allocation, no byte of any output. With left_align = 1 (anything else but 0 is refused) every traced path of the run
 * (root alignments, partial records, extended and split records) is normalised on the device directly behind the traceback (kernel
 * cigar_left_align), before its MD string and its tails are computed, so CIGAR, MD and the cuts of flx_split_options agree:
 *   - the words are processed left to right into an output list; = and X words are appended, a word of the last output word's op
 *     merging with it. A gap word of kind K (I or D) and length L starts at position c of its own sequence (reference for D, query for
 *     I). Repeat: no previous output word: stop. It is of kind K: remove it, add its length to L, move c left by it, repeat. It is X or
 *     the other gap kind: stop. It is = of length E: Emax = E, or E - 1 when that = is the path's first word; s = the largest
 *     s <= Emax with seq[c - i] == seq[c - i + L] for i = 1..s; s == 0: stop; else shorten the = by s (drop it at 0), c -= s, stop if
 *     s < E, else repeat. Then append the gap and an = of the total shift, which merges with a following = word;
 *   - position, the rows and columns consumed and NM do not change; every = column still pairs equal letters; the word count stays
 *     <= 2 NM + 1 but can grow (5= 2D 1X becomes 2= 2D 3= 1X); the rule is idempotent.
 * Limits: a gap does not move through X or through the other gap kind; a gap never becomes the path's first word (a gap that is the
 * first word stays); letters are the index's ranks, so IUPAC codes collapse as they do in MD. params->without_cigar has no trace:
 * refused together with left_align (FLX_ERR_INVALID) before any work. The rule: floxer_amd/csrc/flx_leftalign.hpp. The reserved fields
 * must be 0. */
typedef struct flx_gap_options { uint32_t left_align; uint32_t reserved[7]; } flx_gap_options;
/* flx_align_reads_split / flx_align_reads_resident_split with the gap options (NULL or zeroed: exactly those calls, which forward here) */
int flx_align_reads_gaps(flx_ctx* ctx, const flx_params* params, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads,
                         const flx_run_options* options, const flx_split_options* split, const flx_gap_options* gaps, flx_run** out);
int flx_align_reads_resident_gaps(flx_ctx* ctx, const flx_params* params, const flx_reads* reads, const flx_run_options* options,
                                  const flx_split_options* split, const flx_gap_options* gaps, flx_run** out);
/* flx_align_batch_md with the gap options: K4, K5, cigar_left_align, md_build on the WITH_CIGAR jobs. The three MD arguments may be NULL
 * (no MD strings); gaps NULL or zeroed: exactly flx_align_batch_md / flx_align_batch. */
int flx_align_batch_gaps(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                         const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out, uint32_t* cigar_pool, uint64_t* cigar_pool_words,
                         flx_md_ref* out_md, uint8_t* md_pool, uint64_t* md_pool_bytes, const flx_gap_options* gaps);
/* The rule alone on any CIGAR words: job i covers words [cigar_offset, cigar_offset + cigar_length) of the word pool, the reference
 * window [ref_offset, ref_offset + ref_length) of ref_pool, whose column `begin` is the path's first, and the query [query_offset,
 * query_offset + query_length) of query_pool. Letters are bytes compared for equality. out[i] receives where job i's words lie in
 * out_words; *out_n_words: in = capacity of out_words in words, out = words used (the jobs' results packed in job order; twice the
 * jobs' cigar_length in total always suffices; FLX_ERR_CAPACITY with the need stored when too small). A job outside its pools, an op
 * other than = X I D, a zero-length word, op lengths that do not fit the window and the query (or reach 2^28), or a reserved field
 * that is not 0 is refused (FLX_ERR_INVALID; flx_left_align_batch: before any launch). flx_left_align runs on the host and needs
 * ref_pool; flx_left_align_batch runs the kernel, ref_pool == NULL there: the context's reference text (ref_offset is then a position
 * in the padded concatenated text). Both give the same words. */
typedef struct flx_left_align_job {
    uint64_t cigar_offset;
    uint32_t cigar_length;
    uint32_t reserved;
    uint64_t ref_offset;
    uint32_t ref_length;
    uint32_t begin;
    uint64_t query_offset;
    uint32_t query_length;
    uint32_t reserved2;
} flx_left_align_job;
typedef struct flx_cigar_ref { uint64_t offset; uint32_t length; uint32_t reserved; } flx_cigar_ref;
int flx_left_align(const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len, const uint32_t* cigar_words,
                   uint64_t n_words, const flx_left_align_job* jobs, uint64_t n_jobs, uint32_t* out_words, uint64_t* out_n_words, flx_cigar_ref* out);
int flx_left_align_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                         const uint32_t* cigar_words, uint64_t n_words, const flx_left_align_job* jobs, uint64_t n_jobs, uint32_t* out_words,
                         uint64_t* out_n_words, flx_cigar_ref* out);

/* Affine-gap realignment of a traced path: not floxer's. Every CIGAR here is an edit-distance path whose traceback takes the first valid
 * move among up, left and diagonal, so an indel of several bases often comes out scattered (1D 2= 1D 1= 1D) where a scored aligner
 * writes 3D and an X or two; left-alignment moves a gap but merges none through an X or the other gap kind. The rule (kernel
 * cigar_realign on the device, floxer_amd/csrc/flx_realign.hpp on the host) runs a global DP with affine gap costs over exactly the rows
 * and columns the path consumes, inside a band around the path, and takes its optimum:
 *   - match a, mismatch b, gap open o, gap extend e, all positive; a gap of length L costs o + e L. Letters are the index's ranks: equal
 *     rank = match, no special case for ranks 0 and 5;
 *   - band: d = j - i over the cells the input path visits, (0,0) included; lo = min d - band, hi = max d + band; nothing outside it;
 *   - H[0][0] = 0, E[i][j] = max(H[i][j-1] - o - e, E[i][j-1] - e) (a D column), F[i][j] = max(H[i-1][j] - o - e, F[i-1][j] - e) (an I
 *     row), H[i][j] = max(H[i-1][j-1] + (a or -b), E[i][j], F[i][j]), 32-bit signed;
 *   - traceback from the last cell in state H, ties as everywhere here up > left > diagonal: H == F: to state F; else H == E: to state
 *     E; else = or X. State F emits one I, steps up and stays while F[i][j] == F[i-1][j] - e; state E is its mirror image with D.
 * Position and the rows and columns consumed never change. score = H[m][n] is at least the input path's score; num_errors = the X, I and
 * D lengths of the new words and can exceed the edit distance; every = pairs equal letters, every X unequal ones; with
 * c_max = max(a + b, o + e + a) and c_min = min(a + b, o + e) the result has at most 2 floor(NM c_max / c_min) + 1 words, NM being the
 * input's X + I + D lengths. The rule is not idempotent: the band follows the input path. Limits: one gap-cost piece; nothing beyond
 * the path's own columns (the ends stay where verification put them).
 * 0 in a score field or in band is its default: match 2, mismatch 4, gap_open 4, gap_extend 2, band 16, the first piece of minimap2's
 * map-ont scores: conventions, fitted to nothing. Bounds: each score <= 255, band <= 1024, c_max <= 8 c_min; enable is 0 or 1 and the
 * reserved fields are 0; anything else is refused (FLX_ERR_INVALID) before any work. */
typedef struct flx_realign_options {
    uint32_t enable;       /* 0 off, 1 on, anything else refused */
    uint32_t match;        /* 0: 2 */
    uint32_t mismatch;     /* 0: 4 */
    uint32_t gap_open;     /* 0: 4 */
    uint32_t gap_extend;   /* 0: 2 */
    uint32_t band;         /* 0: 16 */
    uint32_t reserved[2];  /* must be 0 */
} flx_realign_options;
/* The rule alone on any CIGAR words: the jobs are flx_left_align's (same fields, same checks: a job outside its pools, an op other than
 * = X I D, a zero-length word, op lengths that do not fit the window and the query, a reserved field that is not 0: FLX_ERR_INVALID,
 * flx_realign_batch: before any launch). options: the scores and the band (NULL: the defaults; `enable` is judged and otherwise not
 * looked at: the call is the request). out[i]: where job i's words lie in out_words (packed in job order), and its numbers;
 * *out_n_words: in = capacity of out_words in words, out = words used (FLX_ERR_CAPACITY with the need stored when too small;
 * max(cigar_length, 2 floor(NM c_max / c_min) + 1) per job always suffices). kept = 1: the path keeps its input words, with score 0 and
 * num_errors = its NM: a path so long that (rows + columns + 2) max(a, b, o + e) reaches 2^29, and in flx_realign_batch also one whose
 * trace (about rows * (hi - lo + 1) / 2 bytes) is larger than the context's trace arena. flx_realign runs on the host and needs
 * ref_pool; flx_realign_batch runs the kernel, at most 4096 jobs and one trace arena per launch; ref_pool == NULL there: the context's
 * reference text. Both give the same words and numbers. */
typedef flx_left_align_job flx_realign_job;
typedef struct flx_realign_result {
    uint64_t offset;
    uint32_t length;
    uint32_t num_errors;
    int32_t score;
    int32_t diag_lo;
    int32_t diag_hi;
    uint32_t kept;
} flx_realign_result;
int flx_realign(const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len, const uint32_t* cigar_words,
                uint64_t n_words, const flx_realign_job* jobs, uint64_t n_jobs, const flx_realign_options* options, uint32_t* out_words,
                uint64_t* out_n_words, flx_realign_result* out);
int flx_realign_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                      const uint32_t* cigar_words, uint64_t n_words, const flx_realign_job* jobs, uint64_t n_jobs,
                      const flx_realign_options* options, uint32_t* out_words, uint64_t* out_n_words, flx_realign_result* out);
/* flx_align_batch_gaps with the realign options: K4, K5, cigar_realign, cigar_left_align, md_build on the WITH_CIGAR jobs, in that order,
 * so left-alignment and MD read the realigned words. out[i].num_errors is then the realigned path's num_errors, begin stays, and
 * out_scores[i] (may be NULL) receives its score (0 for jobs without a path, and for kept paths, which flx_realign_counters counts). realign NULL or with enable 0: exactly
 * flx_align_batch_gaps, which forwards here. The launches are cut as flx_realign_batch cuts them. */
int flx_align_batch_realign(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                            const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out, uint32_t* cigar_pool, uint64_t* cigar_pool_words,
                            flx_md_ref* out_md, uint8_t* md_pool, uint64_t* md_pool_bytes, const flx_gap_options* gaps,
                            const flx_realign_options* realign, int32_t* out_scores);
/* flx_align_reads_gaps / flx_align_reads_resident_gaps with the realign options: every traced path of the run (root, partial, extended
 * and split records) goes through cigar_realign behind K5, in front of cigar_left_align, md_build and cigar_tails, which read the
 * realigned words. A record's num_errors is then its realigned path's, and that number is what the primary choice, the output options
 * (-N, -D, MAPQ), the partial choice and the budgets of the split and extend retraces see; positions, rows, columns and the record order never
 * change, and the statistics (flx_ctx_set_stats) keep counting the edit distance verification found. Refused together with
 * params->without_cigar. realign NULL or with enable 0: exactly the _gaps calls, which forward here: no launch, no allocation, no byte
 * of any output changes. */
int flx_align_reads_realign(flx_ctx* ctx, const flx_params* params, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads,
                            const flx_run_options* options, const flx_split_options* split, const flx_gap_options* gaps,
                            const flx_realign_options* realign, flx_run** out);
int flx_align_reads_resident_realign(flx_ctx* ctx, const flx_params* params, const flx_reads* reads, const flx_run_options* options,
                                     const flx_split_options* split, const flx_gap_options* gaps, const flx_realign_options* realign,
                                     flx_run** out);
/* One score per record of a run made with flx_realign_options.enable, in flx_run_copy's order: the score of the record's written path
 * under the run's scores (a per = column, -b per X column, -(o + e L) per I or D word of length L; clips count nothing), which for a
 * root record is H[m][n] of its realignment; 0 for unmapped records. FLX_ERR_INVALID on a run made without the option. */
int flx_run_copy_scores(const flx_run* run, int32_t* scores);
/* what cigar_realign did on this context (runs, flx_realign_batch, flx_align_batch_realign) since the last flx_ctx_reset_path_counters: paths through the kernel, paths whose words
 * changed, paths kept */
typedef struct flx_realign_counters { uint64_t paths_realigned; uint64_t paths_changed; uint64_t paths_kept; uint64_t reserved[5]; } flx_realign_counters;
int flx_ctx_get_realign_counters(flx_ctx* ctx, flx_realign_counters* out);

/* The cs tag, minimap2's difference string, short and long form: not floxer's. MD names the reference letters under an X or a D and says
 * nothing of the read's letters at an X or an I; cs holds both sides in one string, and its long form the matched letters too, so a
 * record's read part and reference part can be rebuilt from the tag alone. Off when the struct is zeroed (or NULL), and then nothing
 * changes: no launch, no allocation, no byte of any output. form = 1 (short) or 2 (long), anything else but 0 refused: every traced path
 * of the run gets its string on the device (kernel cs_build, queued behind md_build's place: K4, K5, cigar_realign, cigar_left_align,
 * md_build, cs_build, then cigar_tails in runs), read off the final words (realigned, then left-aligned), the window in the text and the
 * record's oriented sequence in the query pool (for a flag-16 record the reverse-complemented read, as SEQ is written):
 *   - the walk starts at the path's first reference column and first traced query row and goes left to right; every word emits on its
 *     own, nothing merges across words (which is where cs differs from MD);
 *   - = of length L: short form ':' and L in decimal, long form '=' and the L reference letters in upper case (they equal the query's by
 *     construction); X of length L: per column '*', the reference letter, the query letter, lower case (3 L bytes, both forms); I of
 *     length L: '+' and the L query letters, lower case; D of length L: '-' and the L reference letters, lower case;
 *   - letters are the index's ranks: 1..4 give acgt / ACGT, anything else (0 and 5 included) n / N, the limit MD has: IUPAC codes and
 *     lower-case FASTA letters are not recoverable. Nothing is compared again: an X over equal ranks is emitted as it stands. There is
 *     no '~' (no introns). minimap2's own example has this shape: :6-ata:10+gtc:4*at:3;
 *   - soft clips emit nothing: for partial, extended and split records the string covers the traced core only, like MD, and the query
 *     starts at the core's first row. Records that share a CIGAR share their cs bytes; an unmapped record has none (length 0).
 * A path of m query rows and NM errors needs at most 10 NM + 7 bytes (short) or m + 3 NM + 1 (long): floxer_amd/csrc/flx_internal.hpp.
 * The output options (-D, -N, MAPQ) and SA:Z do not interact with it; MD and cs may both be on. params->without_cigar has no trace:
 * refused together with form != 0 (FLX_ERR_INVALID), as are a form above 2 and a reserved field that is not 0, before any work and
 * before the context is looked at. The rule: floxer_amd/csrc/flx_cs.hpp. */
typedef struct flx_cs_options { uint32_t form; uint32_t reserved[7]; } flx_cs_options;
/* flx_align_reads_realign / flx_align_reads_resident_realign with the cs options (NULL or zeroed: exactly those calls, which forward here) */
int flx_align_reads_cs(flx_ctx* ctx, const flx_params* params, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads,
                       const flx_run_options* options, const flx_split_options* split, const flx_gap_options* gaps,
                       const flx_realign_options* realign, const flx_cs_options* cs, flx_run** out);
int flx_align_reads_resident_cs(flx_ctx* ctx, const flx_params* params, const flx_reads* reads, const flx_run_options* options,
                                const flx_split_options* split, const flx_gap_options* gaps, const flx_realign_options* realign,
                                const flx_cs_options* cs, flx_run** out);
/* The cs strings of a run made with flx_cs_options.form != 0, the contract of flx_run_num_md_bytes / flx_run_copy_md: refs[i] is record
 * i's {offset, length} into the bytes (length 0: the record has none), in flx_run_copy's order; either pointer may be NULL. -D / -N
 * select records together with their cs; the pool is not compacted. FLX_ERR_INVALID on a run made without the option. */
uint64_t flx_run_num_cs_bytes(const flx_run* run);
int flx_run_copy_cs(const flx_run* run, flx_md_ref* refs, uint8_t* bytes);
/* flx_align_batch_realign with the cs options: K4, K5, cigar_realign, cigar_left_align, md_build, cs_build on the WITH_CIGAR jobs.
 * out_cs[i]: where job i's string lies in cs_pool (length 0: a job without a path, or of another mode); *cs_pool_bytes: in = capacity,
 * out = bytes used (the jobs' slabs as the device filled them, gaps included; FLX_ERR_CAPACITY with the need stored when too small).
 * cs NULL or zeroed: exactly flx_align_batch_realign, which forwards here, and the three cs arguments are not looked at. */
int flx_align_batch_cs(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                       const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out, uint32_t* cigar_pool, uint64_t* cigar_pool_words,
                       flx_md_ref* out_md, uint8_t* md_pool, uint64_t* md_pool_bytes, const flx_gap_options* gaps,
                       const flx_realign_options* realign, int32_t* out_scores, const flx_cs_options* cs, flx_md_ref* out_cs,
                       uint8_t* cs_pool, uint64_t* cs_pool_bytes);
/* The rule alone on any CIGAR words: the jobs are flx_left_align's (same fields, same checks: a job outside its pools, an op other than
 * = X I D, a zero-length word, op lengths that do not fit the window and the query, a reserved field that is not 0: FLX_ERR_INVALID,
 * flx_cs_batch: before any launch); query_offset is the path's first query row. options: the form, which must be 1 or 2 here (the call
 * is the request). out[i]: where job i's string lies in out_bytes (packed in job order); *out_n_bytes: in = capacity of out_bytes, out =
 * bytes used (FLX_ERR_CAPACITY with the need stored when too small). flx_cs runs on the host and needs ref_pool; flx_cs_batch runs the
 * kernel, ref_pool == NULL there: the context's reference text (ref_offset is then a position in the padded concatenated text; this
 * needs no host text, so a context on an index image works). Both give the same bytes. */
typedef flx_left_align_job flx_cs_job;
int flx_cs(const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len, const uint32_t* cigar_words,
           uint64_t n_words, const flx_cs_job* jobs, uint64_t n_jobs, const flx_cs_options* options, uint8_t* out_bytes, uint64_t* out_n_bytes,
           flx_md_ref* out);
int flx_cs_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                 const uint32_t* cigar_words, uint64_t n_words, const flx_cs_job* jobs, uint64_t n_jobs, const flx_cs_options* options,
                 uint8_t* out_bytes, uint64_t* out_n_bytes, flx_md_ref* out);

/* ------------------------------------------------------------------------------------------------ depth of coverage
 * Not floxer's, which writes records and leaves their pile-up to a coordinate sort and a second tool. A coverage object belongs to a list
 * of reference lengths and holds one u32 of depth per reference position in HBM, indexed by position in the unpadded concatenation of the
 * sequences in reference-id order (4 bytes per symbol + 4). A sequence of 2^31 symbols or more cannot be addressed by
 * flx_record.position and is refused at creation. The rule (floxer_amd/csrc/flx_coverage.hpp), samtools depth's default filters plus -Q / -J:
 *   - a record with flag & 4 never counts; one with flag & 256 only with count_secondary; supplementary records (2048) always count;
 *     with min_mapq > 0 a record counts only if flx_record.reserved >= min_mapq;
 *   - a counted record is walked from `position` over its CIGAR words: every = and X column adds 1 at its reference position, I and S
 *     add nothing, D columns advance the position and add 1 only with count_deletions;
 *   - refused (FLX_ERR_INVALID, on the host before any launch; the accumulator stays as it was): a counted record without CIGAR words
 *     (a run made with without_cigar), an op other than = X I D S, a zero-length word, a reference_id outside the list, a span that ends
 *     behind its sequence, words outside the pool.
 * flx_coverage_create takes the lengths from the context's index (a meta-imported one included) and allocates and clears the accumulator
 * on the context's device; flx_coverage_create_for_lengths is the same without an index (a test hook, and for callers that kept
 * records). A failed allocation returns FLX_ERR_NO_DEVICE and leaves nothing behind. options NULL: all zero; reserved fields must be 0.
 * flx_coverage_add_run adds the written records of a run (it needs min_mapq == 0 or a run made with flx_output_options.mapq),
 * flx_coverage_add_records any record array with its CIGAR word pool; both may be called from several host threads at once.
 * flx_coverage_absorb: into += from, `from` is left cleared; same lengths and options, both before finish; the two may live on different
 * devices. flx_coverage_finish turns the differences into depths in place and is final: a later add, absorb or finish is
 * FLX_ERR_INVALID, and the copy calls work only behind it:
 *   - runs: maximal stretches of equal depth inside one sequence, 0-based and half-open, in position order; a run never crosses a
 *     sequence boundary; runs of depth 0 only with report_zero. flx_coverage_copy_runs: FLX_ERR_CAPACITY when capacity is too small;
 *   - windows of size W (0: one per sequence): for every sequence and every [kW, min((k+1)W, len)) the sum of the depths, the positions
 *     with depth > 0 and the largest depth; flx_coverage_num_windows counts them;
 *   - flx_coverage_copy_depth (a test hook): the depths of [from, to) of one sequence.
 * Everything is integer: nothing depends on the order of adds, the number of calls, host threads or devices.
 * flx_coverage_geometry (a test hook): out[0] = elements per scan tile, out[1] = tile sums one second-level block scans.
 * flx_coverage_host: the rule alone on the host, no device: depth (sum of ref_lens entries) is added to; the same refusals, and depth
 * is untouched when it refuses. */
typedef struct flx_coverage flx_coverage;
typedef struct flx_coverage_options { uint32_t count_deletions, count_secondary, min_mapq, report_zero; uint32_t reserved[4]; } flx_coverage_options;
typedef struct flx_depth_run    { int32_t reference_id; uint32_t depth; uint64_t start, end; } flx_depth_run;
typedef struct flx_depth_window { int32_t reference_id; uint32_t max_depth; uint64_t start, end, depth_sum, covered; } flx_depth_window;
int  flx_coverage_create(flx_ctx* ctx, const flx_coverage_options* o, flx_coverage** out);
int  flx_coverage_create_for_lengths(int hip_device, const uint64_t* ref_lens, uint32_t n_refs, const flx_coverage_options* o, flx_coverage** out);
void flx_coverage_free(flx_coverage* c);
int  flx_coverage_add_run(flx_coverage* c, const flx_run* run);
int  flx_coverage_add_records(flx_coverage* c, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words);
int  flx_coverage_absorb(flx_coverage* into, flx_coverage* from);
int  flx_coverage_finish(flx_coverage* c);
uint64_t flx_coverage_num_runs(const flx_coverage* c);
int  flx_coverage_copy_runs(const flx_coverage* c, flx_depth_run* out, uint64_t capacity);
uint64_t flx_coverage_num_windows(const flx_coverage* c, uint64_t window);
int  flx_coverage_copy_windows(flx_coverage* c, uint64_t window, flx_depth_window* out, uint64_t capacity);
int  flx_coverage_copy_depth(const flx_coverage* c, uint32_t reference_id, uint64_t from, uint64_t to, uint32_t* out);
int  flx_coverage_geometry(uint32_t out[2]);
int  flx_coverage_host(const uint64_t* ref_lens, uint32_t n_refs, const flx_coverage_options* o, const flx_record* records, uint64_t n,
                       const uint32_t* cigar_words, uint64_t n_words, uint32_t* depth /* sum of ref_lens entries, added to */);

/* ------------------------------------------------------------------------------------------------ allele pileup and variant sites
 * Not floxer's, and coverage's successor: where does the sample differ from the reference, and how many reads say so? A pileup object
 * belongs to a list of reference lengths (the limits of the coverage object: coverage_lengths_valid) and holds seven u32 counts per
 * reference position in HBM, indexed by position in the unpadded concatenation of the sequences in reference-id order, as planes in this
 * fixed order: DEPTH = 0, DEL = 1, A = 2, C = 3, G = 4, T = 5, INS = 6. That is 7 x 4 bytes per reference symbol plus the tile arrays:
 * about 87 GB at GRCh38 size, next to 43 GB of index. Nobody has run it at that size. It is no variant caller: no genotype, no quality
 * model, no base qualities; it is the exact integer counts a caller starts from. The rule (floxer_amd/csrc/flx_pileup.hpp):
 *   - which records count: exactly coverage's filter. flag & 4 never; flag & 256 only with count_secondary; 2048 always; with
 *     min_mapq > 0 only if flx_record.reserved >= min_mapq;
 *   - the walk starts at `position` with query row 0 of the record's oriented sequence: the read as given for flag bit 16 clear, its
 *     reverse complement for bit 16 set, as SEQ is written. Over the CIGAR words, left to right:
 *       =  of length L: DEPTH + 1 on its L columns; both cursors advance;
 *       X  of length L: DEPTH + 1 on its L columns, and for each column the oriented read's rank r at that row decides: r in 1..4 adds 1
 *          to plane A + r - 1 at that position, r = 0 or 5 (N) counts in DEPTH only. Nothing is compared with the reference, whose text is
 *          never read: an X over equal ranks is counted under the read's letter as it stands, as cs does;
 *       D  of length L: DEL + 1 on its L columns; the reference cursor advances;
 *       I  of length L: INS + 1 at one anchor position, the reference position of the record's preceding reference-consuming column (a
 *          column of =, X or D), or the record's first reference-consuming column when none precedes this word; the query cursor
 *          advances; one insertion is one event whatever its length;
 *       S: the query cursor advances, nothing is counted;
 *   - refused (FLX_ERR_INVALID, on the host before any launch; the accumulator stays as it was): all that the coverage calls refuse (a
 *     counted record without CIGAR words, an op other than = X I D S, a zero-length word, a reference_id outside the list, a negative
 *     position, a span that ends behind its sequence, words outside the pool), a read_index outside the reads given, a record whose
 *     query-consuming lengths (= X I S) do not sum to exactly its read's length, a record with no reference-consuming column;
 *   - sites, computed after the DEPTH and DEL differences have been summed: cov = DEPTH + DEL (64-bit), best = max(A, C, G, T, DEL, INS);
 *     position p is a site iff cov >= min_depth, best >= min_count and best * 1000 >= min_permille * cov in 64-bit integers. 0 takes the
 *     defaults min_depth 4, min_count 2, min_permille 200: conventions of this project, fitted to nothing. min_permille above 1000 is
 *     refused. Sites come in position order: reference id ascending, then position ascending.
 * The contracts mirror coverage's one for one. options NULL: all zero; reserved fields must be 0. A failed allocation returns
 * FLX_ERR_NO_DEVICE and leaves nothing behind. Reads are given as flx_align_reads takes them: one rank pool, read i =
 * pool[offsets[i], offsets[i+1]), and flx_record.read_index names one of them. Adds may come from several host threads at once; only the
 * reads that counted records refer to go up, once per orientation used. flx_pileup_add_run walks a run and its parts and judges
 * everything before adding anything; it needs min_mapq == 0 or a run made with flx_output_options.mapq, and refuses a run made with
 * without_cigar. flx_pileup_add_run_resident reads the letters straight from the batch's device pool (the forward sequence and its
 * reverse complement behind it) when the batch lives on the object's device; otherwise the batch's host copy goes through the staged
 * path. flx_pileup_absorb: into += from, `from` is left cleared; equal lengths and options, both unfinished; the two may live on
 * different devices. flx_pileup_finish is final: a later add, absorb or finish is FLX_ERR_INVALID, and the copy calls work only behind it.
 * flx_pileup_copy_sites: FLX_ERR_CAPACITY when capacity is below flx_pileup_num_sites. flx_pileup_copy_counts (a test hook): the seven
 * planes of [from, to) of one sequence. Everything is integer: nothing depends on the order of adds, host threads or devices.
 * flx_pileup_host: the rule alone on the host, no device: counts (7 * sum of ref_lens entries, plane-major) is added to; the same
 * refusals, and counts is untouched when it refuses. flx_pileup_sites_host: the site rule over such counts; *n_sites holds the capacity
 * of `out` on entry and the number of sites on return (FLX_ERR_CAPACITY when that is more; `out` may be NULL with capacity 0).
 * FLX_PILEUP_PROFILE (environment): every add prints its records, words, uploaded bytes, pileup_add's device time and its wall time to
 * stderr. */
typedef struct flx_pileup flx_pileup;
typedef struct flx_pileup_options { uint32_t count_secondary, min_mapq, min_depth, min_count, min_permille; uint32_t reserved[3]; } flx_pileup_options;
typedef struct flx_pileup_site { int32_t reference_id; uint32_t position; uint32_t depth, del, ins; uint32_t alt[4]; uint32_t reserved; } flx_pileup_site;   /* position 0-based; alt: A, C, G, T */
int  flx_pileup_create(flx_ctx* ctx, const flx_pileup_options* o, flx_pileup** out);
int  flx_pileup_create_for_lengths(int hip_device, const uint64_t* ref_lens, uint32_t n_refs, const flx_pileup_options* o, flx_pileup** out);
void flx_pileup_free(flx_pileup* p);
int  flx_pileup_add_records(flx_pileup* p, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words,
                            const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads);
int  flx_pileup_add_run(flx_pileup* p, const flx_run* run, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads);
int  flx_pileup_add_run_resident(flx_pileup* p, const flx_run* run, const flx_reads* reads);
int  flx_pileup_absorb(flx_pileup* into, flx_pileup* from);
int  flx_pileup_finish(flx_pileup* p);
uint64_t flx_pileup_num_sites(const flx_pileup* p);
int  flx_pileup_copy_sites(const flx_pileup* p, flx_pileup_site* out, uint64_t capacity);
int  flx_pileup_copy_counts(const flx_pileup* p, uint32_t reference_id, uint64_t from, uint64_t to, uint32_t* out /* 7 * (to - from), plane-major */);
int  flx_pileup_host(const uint64_t* ref_lens, uint32_t n_refs, const flx_pileup_options* o, const flx_record* records, uint64_t n,
                     const uint32_t* cigar_words, uint64_t n_words, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads,
                     uint32_t* counts /* 7 * total, plane-major, added to */);
int  flx_pileup_sites_host(const uint64_t* ref_lens, uint32_t n_refs, const flx_pileup_options* o, const uint32_t* counts,
                           flx_pileup_site* out, uint64_t* n_sites /* in: capacity, out: needed */);

/* ------------------------------------------------------------------------------------------------ coordinate order of records
 * Not floxer's. A sort object holds one 16-byte key and {end, flag} per record added, in HBM, and orders them on the device with a
 * least-significant-digit radix sort (8-bit digits, floxer_amd/csrc/flx_sort.hip). The rule (floxer_amd/csrc/flx_sort.hpp): a key is
 * two u64 compared ascending as (hi, lo),
 *     hi = ref << 32 | (u32)position     ref = 0xFFFFFFFF for a record with flag & 4 or reference_id < 0 (unplaced), else reference_id
 *     lo = ((flag >> 4) & 1) << 63 | ordinal
 * which is samtools sort's order (reference, position, forward strand before reverse, unplaced records last) with ties broken by the
 * ordinal: record i of an add has ordinal first_ordinal + i. The order is total and does not depend on the order of adds, host
 * threads, batch size or devices. A record's end is position + max(1, span) for a mapped record, span the summed lengths of its = X D
 * words (0 for a record without words, as in a without_cigar run), and position + 1 for an unplaced one: the convention of the BAM bin.
 *   - refused (FLX_ERR_INVALID, on the host before any launch; the object stays as it was): a mapped record with reference_id >= n_refs
 *     or position < 0, an op other than = X I D S, a zero-length word, words outside the pool, an end above 2^31 - 1, an ordinal of 2^63
 *     or more, a first_ordinal that an earlier add of this object was given (a full duplicate check is not made);
 *   - out_order (may be NULL) receives the add's own records in key order, as indices into `records` (flx_sort_add_run: into the run's
 *     records as flx_run_copy lists them), sorted on the device with the same kernels;
 *   - adds may come from several host threads at once. The key table grows by reallocation and a device-to-device copy; a failed
 *     allocation is FLX_ERR_NO_DEVICE and leaves the object as it was. At most 2^32 - 1 records per object: FLX_ERR_CAPACITY beyond;
 *   - flx_sort_finish sorts everything added and is final: a later add or finish is FLX_ERR_INVALID. Behind it flx_sort_copy gives
 *     the sorted entries [from, to); an unplaced record's entry has reference_id -1;
 *   - hip_device = -1: no device is opened, and every add and the finish run flx_sort_host's code on the host. That is for tests on
 *     a machine without a GPU and for callers that want the order without a device; the CLI never uses it;
 *   - flx_sort_options, NULL or all zero for the defaults, the reserved fields 0; both members are test hooks: initial_capacity is the records the
 *     table holds before it first grows, tile_keys the keys one block orders per pass, a multiple of the block's threads;
 *   - flx_sort_geometry (a test hook): out[0] = default keys per tile, out[1] = bits per digit, out[2] = default initial capacity,
 *     out[3] = entries per tile of the digit table's scan. The table has 256 entries per tile of keys and is scanned in two levels at
 *     most: past out[3]^2 / 256 tiles the tiles grow instead;
 *   - flx_sort_host: the rule alone on the host, no device: record i has ordinal ordinals[i]; out_sorted receives n entries.
 * FLX_SORT_PROFILE (environment): every add and the finish print their records, uploaded bytes, passes run, device time and wall
 * time to stderr. */
typedef struct flx_sort flx_sort;
typedef struct flx_sort_options { uint64_t initial_capacity; uint32_t tile_keys; uint32_t reserved[5]; } flx_sort_options;
typedef struct flx_sort_entry { uint64_t ordinal; int32_t reference_id; int32_t position; uint32_t end; uint32_t flag; } flx_sort_entry;
int  flx_sort_create(int hip_device, uint32_t n_refs, const flx_sort_options* o, flx_sort** out);
void flx_sort_free(flx_sort* s);
int  flx_sort_add_records(flx_sort* s, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words,
                          uint64_t first_ordinal, uint32_t* out_order /* n entries; may be NULL */);
int  flx_sort_add_run(flx_sort* s, const flx_run* run, uint64_t first_ordinal, uint32_t* out_order /* flx_run_num_records entries; may be NULL */);
int  flx_sort_finish(flx_sort* s);
uint64_t flx_sort_num_records(const flx_sort* s);
int  flx_sort_copy(const flx_sort* s, uint64_t from, uint64_t to, flx_sort_entry* out);
int  flx_sort_geometry(uint32_t out[4]);
int  flx_sort_host(uint32_t n_refs, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words,
                   const uint64_t* ordinals, flx_sort_entry* out_sorted);

/* ------------------------------------------------------------------------------------------------ grid caps
 * flx_grid_caps (a test hook): the most blocks each capped launch asks for. Behind its cap a wave (or a thread) takes further jobs in
 * turns, so a test that wants those turns sizes its input from here. One wave per job, blocks of one wave: out[0] md_build,
 * out[1] cs_build, out[2] cigar_left_align, out[3] cigar_tails, out[4] ed_extend, out[5] cigar_realign, out[6] paf_summarise. One wave
 * per record, blocks of four waves: out[7] coverage_add, out[8] pileup_add, out[9] sv_extract, out[10] sort_keys_add, out[11]
 * errprof_add. One thread per element, blocks of 256: out[12] sort_census, out[13] sort_iota and sort_entries, out[14] sv_junctions,
 * sv_coarse_flags, sv_regroup, sv_fine_flags, sv_cluster_heads, sv_cluster_bounds, sv_cluster_fill and sv_signatures. out[15] is 0. */
int  flx_grid_caps(uint32_t out[16]);

/* ------------------------------------------------------------------------------------------------ structural-variant signatures
 * Not floxer's, and pileup's sibling for events too long for one position: where is the sample rearranged, and how many records say so?
 * An sv object on a device collects one signature per long deletion, long insertion and split junction of the records added, orders
 * them with the key sort (floxer_amd/csrc/flx_sort.hip) and merges neighbours into clusters with their support. No variant caller: no
 * genotypes, no quality model; it is the exact table a caller starts from. It allocates nothing per reference position. The rule
 * (floxer_amd/csrc/flx_sv.hpp), words len << 4 | op with = 7, X 8, I 1, D 2, S 4, positions 0-based and local to their sequence:
 *   - which records count: exactly the coverage calls' filter (flag & 4 never, flag & 256 only with count_secondary, 2048 always, with
 *     min_mapq > 0 only records whose `reserved` is at least that);
 *   - DEL (type 0): every D word of a counted record with len >= min_length; pos_a = its first deleted column, q = len, ref_b = ref_a,
 *     both sides 0. INS (type 1): every I word with len >= min_length; pos_a = the position of the record's preceding
 *     reference-consuming column, or the record's first reference-consuming column when none precedes the word (pileup's anchor);
 *     q = len, ref_b = ref_a, both sides 0;
 *   - BND (type 2): one per pair of query-neighbouring records of a read. A read's group is the maximal run of neighbouring records of
 *     the given array (within one piece of a run) with equal read_index; its members are its counted records with flag & 256 clear
 *     (secondaries never form junctions, whatever count_secondary says). Each member has a query interval on the read as given (the PAF
 *     summary's query_start / query_end); members are ordered by (query_start, index in the array). Each consecutive pair (a, b) gives
 *     one junction of two ends, with rs = position and re = position + the summed = X D lengths: the end of a is (ref_a, re_a - 1,
 *     side R = 1) when a is forward and (ref_a, rs_a, side L = 0) when a is reverse; the end of b is (ref_b, rs_b, L) when b is forward
 *     and (ref_b, re_b - 1, R) when b is reverse. The two ends are put in ascending (ref, pos, side) order: the smaller is end a, its
 *     position pos_a; the other's position is q. A read and its reverse complement, mapped to the same places, give equal signatures;
 *   - refused (FLX_ERR_INVALID, on the host before any launch; the object stays as it was): all that the coverage calls refuse (a
 *     counted record without CIGAR words, as a run made with without_cigar has them; words outside the pool; an op other than = X I D S;
 *     a zero-length word; a reference_id outside the list; a negative position; a span that ends behind its sequence), a read_index
 *     outside the reads, query-consuming lengths that do not sum to the read's length, no reference-consuming column, an S word with
 *     other words on both sides, a group of more than 64 members, 2^30 sequences or more, min_mapq > 0 on a run made without mapq;
 *   - a signature is one 128-bit key, hi = type << 62 | side_a << 61 | side_b << 60 | ref_a << 30 | ref_b, lo = pos_a << 32 | q: the
 *     class (type, sides, ref_a, ref_b) orders ahead of the coordinates;
 *   - clusters, made by flx_sv_finish in two levels: (1) in key order a coarse group breaks between neighbours whose class differs or
 *     whose pos_a differ by more than max_distance; (2) within a coarse group, in (q, pos_a) order, a cluster breaks where q differs
 *     from its predecessor by more than max_distance. A cluster reports its class, support (the number of its members), pos_a_min,
 *     pos_a_max, q_min, q_max and q_median, the q of member (support - 1) / 2 in that order. Clusters come in the order of (2); those
 *     with support < min_support are dropped. This is single linkage: a chain of close signatures can span more than max_distance;
 *   - 0 takes the defaults min_length 50, max_distance 100, min_support 2: conventions of this project, fitted to nothing;
 *   - support counts records, not reads: at default flags a read writes some forty records at one locus that share one CIGAR. Make the
 *     runs with flx_output_options.drop_duplicates and max_alignments_per_read 1.
 * Equal keys are interchangeable, so both tables are functions of the multiset of signatures alone: nothing depends on the order of
 * adds, host threads, batch cuts or devices. Only read lengths are needed (read i has read_offsets[i + 1] - read_offsets[i] letters),
 * never letters. options NULL: all zero; the reserved fields must be 0; initial_capacity (a test hook) is the keys the table holds
 * before it first grows. Adds may come from several host threads: judging happens outside the object's lock, upload and launches
 * inside it. The key table grows by reallocation and a device-to-device copy; a failed allocation is FLX_ERR_NO_DEVICE and leaves the
 * object as it was; at most 2^32 - 1 signatures, FLX_ERR_CAPACITY beyond. A kernel that finds a record at odds with the host's
 * judgement makes the add return FLX_ERR_INTERNAL. flx_sv_add_run walks a run and its parts and judges everything before it adds
 * anything. flx_sv_absorb: `into` receives `from`'s signatures, `from` is left empty; equal lengths and options, both unfinished; the
 * two may live on different devices. flx_sv_finish is final: a later add, absorb or finish is FLX_ERR_INVALID, and the num and copy
 * calls work only behind it (flx_sv_num_*: 0 before); a finish that fails (FLX_ERR_NO_DEVICE: it allocates its sort buffers and
 * tables) leaves the object unfinished, and empty when it failed behind the first sort (its buffers are reused). flx_sv_copy_signatures: all signatures [from, to) in key order, whatever
 * min_support. flx_sv_copy_clusters: FLX_ERR_CAPACITY when capacity is below flx_sv_num_clusters.
 * flx_sv_host: the rule alone on the host, no device: *n_signatures holds the capacity of `out` on entry and the number of signatures
 * on return, in key order (FLX_ERR_CAPACITY when that is more; `out` may be NULL with capacity 0); the same refusals, `out` untouched
 * when it refuses. flx_sv_clusters_host: the clusters of n signatures in any order, the same way.
 * FLX_SV_PROFILE (environment): every add and the finish print records, words, signatures, passes, device time and wall time to stderr. */
typedef struct flx_sv flx_sv;
typedef struct flx_sv_options { uint32_t min_length, max_distance, min_support, count_secondary, min_mapq; uint32_t reserved[3]; uint64_t initial_capacity; } flx_sv_options;
typedef struct flx_sv_signature { uint32_t type, side_a, side_b, reserved; int32_t ref_a, ref_b; uint32_t pos_a, q; } flx_sv_signature;
typedef struct flx_sv_cluster { uint32_t type, side_a, side_b, support; int32_t ref_a, ref_b; uint32_t pos_a_min, pos_a_max, q_min, q_median, q_max, reserved; } flx_sv_cluster;
int  flx_sv_create(flx_ctx* ctx, const flx_sv_options* o, flx_sv** out);
int  flx_sv_create_for_lengths(int hip_device, const uint64_t* ref_lens, uint32_t n_refs, const flx_sv_options* o, flx_sv** out);
void flx_sv_free(flx_sv* s);
int  flx_sv_add_records(flx_sv* s, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words,
                        const uint64_t* read_offsets, uint64_t n_reads);
int  flx_sv_add_run(flx_sv* s, const flx_run* run, const uint64_t* read_offsets, uint64_t n_reads);
int  flx_sv_absorb(flx_sv* into, flx_sv* from);
int  flx_sv_finish(flx_sv* s);
uint64_t flx_sv_num_signatures(const flx_sv* s);
int  flx_sv_copy_signatures(const flx_sv* s, uint64_t from, uint64_t to, flx_sv_signature* out);
uint64_t flx_sv_num_clusters(const flx_sv* s);
int  flx_sv_copy_clusters(const flx_sv* s, flx_sv_cluster* out, uint64_t capacity);
int  flx_sv_host(const uint64_t* ref_lens, uint32_t n_refs, const flx_sv_options* o, const flx_record* records, uint64_t n,
                 const uint32_t* cigar_words, uint64_t n_words, const uint64_t* read_offsets, uint64_t n_reads,
                 flx_sv_signature* out, uint64_t* n_signatures /* in: capacity, out: needed */);
int  flx_sv_clusters_host(const flx_sv_options* o, const flx_sv_signature* signatures, uint64_t n, flx_sv_cluster* out,
                          uint64_t* n_clusters /* in: capacity, out: needed */);

/* ------------------------------------------------------------------------------------------------ error profile of the alignments
 * Not floxer's. How do the reads err? Which letter is read as which, how long insertions and deletions are, how many of them sit in
 * homopolymers, whether a read's ends are worse than its middle, how identities are distributed and how long the error-free stretches
 * are: the figures behind --error-probability, summed on the device from the records' = X I D S words, the reads' letters and the
 * reference text in HBM. An error-profile object holds one flx_errprof_table of u64 counters (9 KB). The rule
 * (floxer_amd/csrc/flx_errprof.hpp):
 *   - which records count: exactly coverage's filter. flag & 4 never; flag & 256 only with count_secondary; 2048 always; with
 *     min_mapq > 0 only if flx_record.reserved >= min_mapq;
 *   - the walk starts at `position` with row 0 of the record's oriented sequence (the read as given for flag bit 16 clear, its reverse
 *     complement for bit 16 set). t[p]: the reference rank at position p; q[r]: the oriented read rank at row r; [s0, s1): the record's
 *     sequence; len: the read's length; g(r) = reverse ? len - 1 - r : r, the row in the read as given; bin(r) = g(r) * 100 / len in
 *     64-bit integers, 0..99 (0 for a read without letters). Ranks are 0..5 and index the 6 x 6 and 6-entry sections directly;
 *       pair_eq[t * 6 + q], pair_x[t * 6 + q]: + 1 per column of an = word, of an X word; both letters are read for every column, so
 *          pair_eq off its diagonal is an integrity figure: 0 for this aligner's own runs, and nothing relies on that;
 *       ins_len, del_len: a word of length L adds 1 at min(L, 64) - 1; the last entry is "64 or longer";
 *       ins_letter[q], del_letter[t]: + 1 per inserted read letter, per deleted reference letter;
 *       hp_del[34]: for a D word over [p, p + L) with a = t[p]: entry 33 when a is not in 1..4 or a deleted letter differs from a; else
 *          min(32, left + L + right), left the run of a from p - 1 downwards while the position is >= s0, right the run of a from p + L
 *          upwards while the position is < s1, each stopped at 32;
 *       hp_ins[34]: for an I word of letters q[r, r + L) with a = q[r]: p is the reference position of the next reference-consuming
 *          column (`position` when nothing precedes the word; it may be the record's end and may be s1); entry 33 when a is not in 1..4
 *          or the letters differ; else min(32, left + right), left the run of a from p - 1 downwards (>= s0), right the run of a from p
 *          upwards (< s1), each stopped at 32; an inserted run next to no equal letter is entry 0. Runs never cross a sequence boundary;
 *       pos_match, pos_mismatch, pos_ins, pos_clip [100]: + 1 at bin(r) per row of an =, X, I, S word;
 *       pos_del[100]: + 1 per D word (not per base) at bin(min(r, len - 1)), r the row the walk has reached;
 *       eq_run[256]: an = word of length L adds 1 at min(L, 256) - 1 (words are counted: neighbouring = words are not merged);
 *       identity[101]: once per record at matches * 100 / (matches + mismatches + ins_bases + del_bases);
 *       totals[8]: records, matches, mismatches, ins_events, ins_bases, del_events, del_bases, clip_bases;
 *   - refused (FLX_ERR_INVALID, on the host before any launch; the object stays as it was): all that the pileup calls refuse (and with
 *     them the coverage calls), and a record whose reference-consuming plus query-consuming lengths reach 2^31. A reference text with a
 *     rank above 5 is refused at create. Read ranks above 5 are outside the read pool's contract and count as 5.
 * options NULL: all zero; reserved fields must be 0. flush_threshold (a test hook): a wave of the kernel adds its on-chip u32 sums to
 * the table once the columns plus rows it has walked since its last flush reach this; 0 takes 2^30, above 2^31 is refused; no sum
 * depends on it. flx_errprof_create reads the reference letters from the context's own text in HBM (no second copy) and counts as a
 * live object of the context: flx_ctx_destroy refuses until it is freed. flx_errprof_create_for_text uploads the unpadded concatenation
 * of the sequences' ranks itself (coverage's limits on the lengths); hip_device -1 is refused (the host form is flx_errprof_host).
 * Reads are given as flx_align_reads takes them. Adds may come from several host threads at once. flx_errprof_add_run walks a run and
 * its parts and judges everything before adding anything; it needs min_mapq == 0 or a run made with flx_output_options.mapq, and
 * refuses a run made with without_cigar. flx_errprof_add_run_resident reads the letters from the batch's device pool when the batch
 * lives on the object's device, and takes the staged path otherwise. flx_errprof_absorb: into += from, `from` is left cleared; equal
 * lengths, count_secondary and min_mapq; the two may live on different devices. flx_errprof_copy gives the sums so far, at any time:
 * there is no finish call. Everything is integer: nothing depends on the order of adds, the number of calls, host threads, resident
 * or host reads, or devices. flx_errprof_host: the rule alone on the host, no device: `table` is added to; the same refusals, and the
 * table is untouched when it refuses. FLX_ERRPROF_PROFILE (environment): every add prints its records, words, uploaded bytes,
 * errprof_add's device time and its wall time to stderr.
 * Not here: base qualities, per-read tables, denominators for the homopolymer entries (how many reference runs of each length were
 * covered). */
typedef struct flx_errprof flx_errprof;
typedef struct flx_errprof_options { uint32_t count_secondary, min_mapq, flush_threshold; uint32_t reserved[5]; } flx_errprof_options;
typedef struct flx_errprof_table {
    uint64_t pair_eq[36], pair_x[36], ins_len[64], del_len[64], ins_letter[6], del_letter[6], hp_del[34], hp_ins[34];
    uint64_t pos_match[100], pos_mismatch[100], pos_ins[100], pos_clip[100], pos_del[100], eq_run[256], identity[101], totals[8];
    uint64_t reserved[7];
} flx_errprof_table;
int  flx_errprof_create(flx_ctx* ctx, const flx_errprof_options* o, flx_errprof** out);
int  flx_errprof_create_for_text(int hip_device, const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs,
                                 const flx_errprof_options* o, flx_errprof** out);
void flx_errprof_free(flx_errprof* p);
int  flx_errprof_add_records(flx_errprof* p, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words,
                             const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads);
int  flx_errprof_add_run(flx_errprof* p, const flx_run* run, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads);
int  flx_errprof_add_run_resident(flx_errprof* p, const flx_run* run, const flx_reads* reads);
int  flx_errprof_absorb(flx_errprof* into, flx_errprof* from);
int  flx_errprof_copy(const flx_errprof* p, flx_errprof_table* out);
int  flx_errprof_host(const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs, const flx_errprof_options* o,
                      const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words, const uint8_t* read_pool,
                      const uint64_t* read_offsets, uint64_t n_reads, flx_errprof_table* table /* added to */);

/* ------------------------------------------------------------------------------------------------ consensus sequence
 * Not floxer's, and the step behind pileup: the sequence the reads vote for, guided by the reference (polishing a draft, or a sample
 * rebuilt from a related reference). A consensus object holds pileup's seven u32 planes over the concatenation of the sequences (28
 * bytes per reference base) plus one 16-byte key per insertion event, and reads the reference text in HBM. The rule
 * (floxer_amd/csrc/flx_consensus.hpp):
 *   - which records count, what is refused and the seven sums: pileup's, with count_secondary and min_mapq;
 *   - every I word of a counted record is an event. Its anchor is the position of the record's preceding reference-consuming column.
 *     It is an allele when such a column precedes it in the record, its length is 1..32 and all its letters of the oriented sequence
 *     have rank 1..4; otherwise it is dropped (longer insertions are the structural-variant object's business). Equal (anchor, length,
 *     letters) are one allele with a count; the winner at an anchor is the allele with the largest count, ties to the smaller
 *     (anchor, length, letters lexicographic);
 *   - the call at a position: R the text's rank, cov = DEPTH + DEL, n[r] = plane r + (R == r ? DEPTH - A - C - G - T : 0) for r in A,
 *     C, G, T, n[DEL] = DEL. cov < min_depth: uncalled, R's letter (N with mask_low_depth), no insertion, no change. Otherwise best is
 *     the largest of the five, ties to R, else to the first of A, C, G, T, DEL; a best other than R stands only with n[best] >=
 *     min_count and n[best] * 1000 >= min_permille * cov (64-bit), else R stays. A rank outside 1..4 is written N; DEL emits no
 *     letter. The winning insertion behind the position is applied iff cov >= min_depth and its count meets the same two thresholds,
 *     also when the position itself is called DEL. 0 takes the defaults 3 / 2 / 500: conventions of this project, fitted to nothing;
 *   - the outputs: per sequence its letters as ASCII (possibly none); the changes, every place the consensus departs from the text in
 *     position order (kind 0 SUB, 1 DEL, 2 INS; a SUB or DEL row in front of the INS row of the same position; length 1 for SUB and
 *     DEL; alt_rank the called rank for SUB and 0 otherwise; count the winning count; letters the inserted letters, two bits each
 *     from bit 62 down, letter k at bits 63 - 2k and 62 - 2k holding rank - 1, and 0 for SUB and DEL); and, as a test hook, the alleles
 *     in key order.
 * flx_consensus_create reads the context's own text in HBM (no second copy) and counts as a live object of the context:
 * flx_ctx_destroy refuses until it is freed. flx_consensus_create_for_text uploads the unpadded concatenation of the sequences' ranks
 * itself; hip_device -1 is refused (the host form is flx_consensus_host). options NULL: all zero; the reserved fields must be 0 and
 * min_permille at most 1000. The add calls are pileup's: adds may come from several host threads at once, a run made with
 * without_cigar is refused, min_mapq needs a run made with flx_output_options.mapq; a refused add leaves the object as it was. The keys
 * grow by doubling up to 2^32 - 1 events; a failed growth is reported and leaves the object as it was. flx_consensus_finish is final: a
 * later add or finish is FLX_ERR_INVALID, and the copy calls work only behind it. If all letters together would reach 2^32 it returns
 * FLX_ERR_CAPACITY and the object holds no result. flx_consensus_copy_letters, flx_consensus_copy_changes and
 * flx_consensus_copy_alleles return FLX_ERR_CAPACITY with the needed size in the message when capacity is too small.
 * flx_consensus_geometry (a test hook): out[0] the grid cap of consensus_ins_keys in blocks, out[1] its waves per block, out[2] the
 * longest allele, out[3] 0. flx_consensus_host: the rule alone on the host, no device, the same refusals: letter_offsets (n_refs + 1
 * entries) and the three tables; each n_* holds the capacity on entry and the need on return (FLX_ERR_CAPACITY when one is too small;
 * nothing is written then but the needs). Objects of several devices are not merged: there is no absorb call.
 * FLX_CONSENSUS_PROFILE (environment): every add and the finish print their sizes, device time and wall time to stderr. */
typedef struct flx_consensus flx_consensus;
typedef struct flx_consensus_options { uint32_t count_secondary, min_mapq, min_depth, min_count, min_permille, mask_low_depth; uint32_t reserved[2]; } flx_consensus_options;
typedef struct flx_consensus_change { int32_t reference_id; uint32_t position /* 0-based */, kind, ref_rank, alt_rank, length, count, cov; uint64_t letters; } flx_consensus_change;
typedef struct flx_consensus_allele { int32_t reference_id; uint32_t position /* the anchor, 0-based */, length, count; uint64_t letters; } flx_consensus_allele;
int  flx_consensus_create(flx_ctx* ctx, const flx_consensus_options* o, flx_consensus** out);
int  flx_consensus_create_for_text(int hip_device, const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs,
                                   const flx_consensus_options* o, flx_consensus** out);
void flx_consensus_free(flx_consensus* p);
int  flx_consensus_add_records(flx_consensus* p, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words,
                               const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads);
int  flx_consensus_add_run(flx_consensus* p, const flx_run* run, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads);
int  flx_consensus_add_run_resident(flx_consensus* p, const flx_run* run, const flx_reads* reads);
int  flx_consensus_finish(flx_consensus* p);
uint64_t flx_consensus_num_letters(const flx_consensus* p, uint32_t reference_id);
int  flx_consensus_copy_letters(const flx_consensus* p, uint32_t reference_id, char* out, uint64_t capacity);
uint64_t flx_consensus_num_changes(const flx_consensus* p);
int  flx_consensus_copy_changes(const flx_consensus* p, flx_consensus_change* out, uint64_t capacity);
uint64_t flx_consensus_num_alleles(const flx_consensus* p);
int  flx_consensus_copy_alleles(const flx_consensus* p, flx_consensus_allele* out, uint64_t capacity);
int  flx_consensus_geometry(uint32_t out[4]);
int  flx_consensus_host(const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs, const flx_consensus_options* o,
                        const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words, const uint8_t* read_pool,
                        const uint64_t* read_offsets, uint64_t n_reads, uint64_t* letter_offsets, char* letters, uint64_t* n_letters,
                        flx_consensus_change* changes, uint64_t* n_changes, flx_consensus_allele* alleles, uint64_t* n_alleles);

/* ------------------------------------------------------------------------------------------------ diploid small-variant calls
 * Not floxer's, and the step behind the consensus: which small variants the sample carries and in which genotype, as rows a VCF is
 * written from (the tool floxer_variants does that). A variants object holds pileup's seven u32 planes plus one more over the
 * concatenation of the sequences (32 bytes per reference base) plus one 16-byte key per insertion or deletion event, and reads the
 * reference text in HBM. The rule (floxer_amd/csrc/flx_variants.hpp), integer arithmetic throughout:
 *   - which records count, what is refused and the seven sums: pileup's, with count_secondary and min_mapq;
 *   - every I word and every D word of a counted record is an event. Its anchor a is the position of the record's preceding
 *     reference-consuming column. An I word is an allele when such a column precedes it, its length is 1..32 and all its letters of the
 *     oriented sequence have rank 1..4; a D word when such a column precedes it and its length is 1..max_del (0 takes 50, range
 *     1..2^28 - 1; longer deletions are the structural-variant object's business); everything else is dropped. Equal (anchor, kind,
 *     length, letters) are one allele with a count, in the order deletions before insertions, shorter first, then letters; events(a)
 *     is the sum of the counts at a, the winner the allele with the largest count, ties to the smaller key;
 *   - costs in centi-phred (-1000 log10 of a probability): cost_match m (a read shows the allele of a homozygous genotype),
 *     cost_mismatch x (anything else), cost_het h (either allele of a heterozygous genotype), prior_het and prior_hom (the priors of
 *     0/1 and 1/1). 0 takes 36 / 1574 / 325 / 3000 / 3301, the values for a per-read error of 0.08 and a heterozygosity of 0.001:
 *     conventions of this project, fitted to nothing. The library never computes a logarithm. Refused: m >= h, h >= x (the model would
 *     be degenerate), any cost above 2^20 (the sums stay inside 64 bits);
 *   - the SNV candidate at p, only where the text's rank R is 1..4: cov = DEPTH + DEL, n[r] as the consensus has it (the = columns
 *     credited to R), alt the r != R with the largest n[r], ties to the smallest rank, none when that count is 0; ref_n = n[R],
 *     alt_n = n[alt], oth = cov - ref_n - alt_n;
 *   - the indel candidate at an anchor a with an allele: cov = DEPTH[a] + DEL[a], alt_n the winner's count, oth = events(a) - alt_n,
 *     ref_n = cov - events(a), saturating at 0 (a record that ends exactly on a counts towards ref: a known over-count);
 *   - the genotype, for both: L_RR = ref_n m + (alt_n + oth) x, L_RA = (ref_n + alt_n) h + oth x, L_AA = alt_n m + (ref_n + oth) x;
 *     Q_RR = L_RR, Q_RA = L_RA + prior_het, Q_AA = L_AA + prior_hom; the genotype is the smallest Q, ties in the order RR, RA, AA. A row
 *     is written iff the genotype is not RR, cov >= min_depth (0 takes 4) and qual = Q_RR - min(Q_RA, Q_AA) >= min_qual (centi-phred, 0
 *     takes 2000). gq = (the second smallest Q - the smallest) / 100, at most 99; pl[g] = (L_g - min L) / 100; qual and pl saturate at
 *     2^32 - 1, as do ref_count, alt_count and cov;
 *   - the rows, in position order, the SNV row in front of the indel row of the same position (the anchor for indels): kind 0 SNV, 1
 *     DEL, 2 INS; ref_rank the text's rank at the position; alt_rank the called rank for an SNV and 0 otherwise; length 1 for an SNV;
 *     gt 1 = 0/1, 2 = 1/1; letters the inserted letters as the consensus packs them, 0 otherwise; reserved 0. Biallelic: one SNV and
 *     one indel row per position at most. An SNV inside a called deletion is written independently: there is no * allele. No strand
 *     bias, no base qualities. The alleles (a test hook) in key order.
 * Create, add, finish, copy, the lifetime, the refusals and the profile switch (FLX_VARIANTS_PROFILE) are the consensus object's:
 * flx_variants_create reads the context's text and counts as a live object of the context (flx_ctx_destroy refuses until it is freed);
 * adds may come from several host threads; a refused add leaves the object as it was; the keys grow by doubling up to 2^32 - 1 events,
 * a budget that insertion and deletion events share (more: FLX_ERR_CAPACITY); flx_variants_finish is final; 2^32 rows or more:
 * FLX_ERR_CAPACITY and no result. flx_variants_geometry (a test hook): out[0] the grid cap of variants_indel_keys in blocks, out[1] its
 * waves per block, out[2] the longest insertion, out[3] the default max_del. flx_variants_host: the rule alone on the host, no device,
 * the same refusals; each n_* holds the capacity on entry and the need on return (FLX_ERR_CAPACITY when one is too small; nothing is
 * written then but the needs). flx_variants_genotype (a test hook): the genotype of one candidate under the options' costs, counts
 * below 2^34 each: out = gt (0 = 0/0), gq, qual, pl[0..2], then 1 if a row would be written with cov = ref_n + alt_n + oth, then 0. */
typedef struct flx_variants flx_variants;
typedef struct flx_variants_options {
    uint32_t count_secondary, min_mapq, min_depth, min_qual, max_del, cost_match, cost_mismatch, cost_het, prior_het, prior_hom;
    uint32_t reserved[2];
} flx_variants_options;
typedef struct flx_variant {
    int32_t reference_id;
    uint32_t position /* 0-based */, kind, ref_rank, alt_rank, length, ref_count, alt_count, cov, gt, gq, qual, pl[3], reserved;
    uint64_t letters;
} flx_variant;
typedef struct flx_variant_allele { int32_t reference_id; uint32_t position /* the anchor, 0-based */, kind, length, count, reserved; uint64_t letters; } flx_variant_allele;
int  flx_variants_create(flx_ctx* ctx, const flx_variants_options* o, flx_variants** out);
int  flx_variants_create_for_text(int hip_device, const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs,
                                  const flx_variants_options* o, flx_variants** out);
void flx_variants_free(flx_variants* p);
int  flx_variants_add_records(flx_variants* p, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words,
                              const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads);
int  flx_variants_add_run(flx_variants* p, const flx_run* run, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads);
int  flx_variants_add_run_resident(flx_variants* p, const flx_run* run, const flx_reads* reads);
int  flx_variants_finish(flx_variants* p);
uint64_t flx_variants_num_rows(const flx_variants* p);
int  flx_variants_copy_rows(const flx_variants* p, flx_variant* out, uint64_t capacity);
uint64_t flx_variants_num_alleles(const flx_variants* p);
int  flx_variants_copy_alleles(const flx_variants* p, flx_variant_allele* out, uint64_t capacity);
int  flx_variants_geometry(uint32_t out[4]);
int  flx_variants_genotype(const flx_variants_options* o, uint64_t ref_n, uint64_t alt_n, uint64_t oth, uint32_t out[8]);
int  flx_variants_host(const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs, const flx_variants_options* o,
                       const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words, const uint8_t* read_pool,
                       const uint64_t* read_offsets, uint64_t n_reads, flx_variant* rows, uint64_t* n_rows, flx_variant_allele* alleles,
                       uint64_t* n_alleles);

/* ------------------------------------------------------------------------------------------------ read-backed phasing
 * Not floxer's, and the step behind the variant calls: which of the heterozygous calls lie on the same chromosome copy, and which
 * records come from which copy (the tool floxer_phase writes both, as a phased VCF and a table of haplotype tags). A phase object
 * holds its sites, one byte per (counted record, site in its span) and 32 bytes per counted record in HBM; it never reads the
 * reference text on the device. The rule (floxer_amd/csrc/flx_phase.hpp), integer arithmetic throughout:
 *   - the sites are given at create time, strictly increasing by (reference_id, position, kind): kind 0 SNV, 1 DEL, 2 INS as
 *     flx_variant has them, position the SNV's position or the indel's anchor, letters as the consensus packs them (0 for an SNV or a
 *     DEL). Refused: an SNV whose text rank is outside 1..4 or equals alt_rank, or whose alt_rank is outside 1..4; a DEL that runs past
 *     its sequence; an INS of more than 32 letters or with bits behind its length; letters on an SNV or a DEL; a non-zero reserved;
 *     sites out of order (FLX_ERR_INVALID); more than 2^32 - 2 sites (FLX_ERR_CAPACITY);
 *   - which records count and what is refused: pileup's, with count_secondary and min_mapq. The unit of phasing is the counted record,
 *     not the read;
 *   - a counted record has one slot for every site whose anchor lies inside its reference span, and one observation per slot: REF 0,
 *     ALT 1, NONE 2. An SNV: the record's column there is an = word: REF; an X word whose oriented letter is alt_rank: ALT; anything
 *     else NONE. A DEL or INS with anchor a: E is the run of I and D words directly behind the column at a (empty unless a is the last
 *     column of its word); a word of E whose allele key (flx_variants' key, deletions of any length) is the site's: ALT; otherwise, E
 *     empty, the column = or X and a + 1 inside the span: REF; otherwise NONE;
 *   - links: for neighbouring sites i and i + 1, over the records that observe both with REF or ALT, cis(i) counts equal alleles and
 *     trans(i) unequal ones; connected(i) iff both lie in one sequence and |cis - trans| >= min_link (0 takes 2); a phase set is a
 *     maximal run of connected neighbours, its id the index of its first site; p(first) = 0, p(i + 1) = p(i) ^ (trans(i) > cis(i));
 *     a set of one site is unphased; p = 0 puts ALT on haplotype 1 (1|0), p = 1 on haplotype 2 (0|1);
 *   - tags: a record belongs to the phase set in which it has the most REF/ALT observations of phased sites (ties to the first; none:
 *     hap 0, phase_set 2^32 - 1); there h1 counts allele ^ p == 1, h2 the rest; hap 1 if h1 - h2 >= min_margin, 2 if h2 - h1 >=
 *     min_margin (0 takes 1), else 0;
 *   - refinement, refine_rounds times (0 takes 1, at most 8, skip_refine: none): every tagged record votes at the REF/ALT slots of its
 *     set, keep(i) for x == (hap == 1), swap(i) otherwise; p(i) flips where swap > keep; the tags are made again. keep and swap as
 *     reported are the last round's, before its flips.
 * Known limits: links join neighbouring sites only, so one site of noise (a false 0/1) splits a set in two; no base qualities, no
 * read-pair or supplementary linkage; the defaults 2 / 1 / 1 are conventions of this project, fitted to nothing.
 * Create, add, finish, copy, the lifetime, the refusals and the profile switch (FLX_PHASE_PROFILE) are the variants object's:
 * flx_phase_create counts as a live object of the context (flx_ctx_destroy refuses until it is freed); adds may come from several host
 * threads; a refused add leaves the object as it was; observations and records grow by doubling, up to 2^32 - 1 slots in all (more:
 * FLX_ERR_CAPACITY); flx_phase_finish is final. Results: one row per site. Tags: one per counted record in counting order (adds in
 * the order they took the object's lock, a run's pieces in flx_run_copy's order, records in order); add is the 0-based serial of the
 * add call, read the record's read_index. flx_phase_geometry (a test hook): out[0] the grid cap of phase_observe in blocks, out[1] its
 * waves per block, out[2] the scan tile, out[3] the longest insertion. flx_phase_host: the rule alone on the host, no device, the same
 * refusals; results takes n_sites rows; *n_tags holds the capacity on entry and the need on return (FLX_ERR_CAPACITY when too small;
 * nothing else is written then). */
typedef struct flx_phase flx_phase;
typedef struct flx_phase_options { uint32_t count_secondary, min_mapq, min_link, min_margin, refine_rounds, skip_refine; uint32_t reserved[2]; } flx_phase_options;
typedef struct flx_phase_site { int32_t reference_id; uint32_t position /* 0-based */, kind, alt_rank, length, reserved; uint64_t letters; } flx_phase_site;
typedef struct flx_phase_result { uint32_t phase_set, phased, phase, cis, trans, keep, swap, reserved; } flx_phase_result;
typedef struct flx_phase_tag { uint32_t add, read, hap, phase_set, h1, h2, n_slots, reserved; } flx_phase_tag;
int  flx_phase_create(flx_ctx* ctx, const flx_phase_options* o, const flx_phase_site* sites, uint64_t n_sites, flx_phase** out);
int  flx_phase_create_for_text(int hip_device, const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs,
                               const flx_phase_options* o, const flx_phase_site* sites, uint64_t n_sites, flx_phase** out);
void flx_phase_free(flx_phase* p);
int  flx_phase_add_records(flx_phase* p, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words,
                           const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads);
int  flx_phase_add_run(flx_phase* p, const flx_run* run, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads);
int  flx_phase_add_run_resident(flx_phase* p, const flx_run* run, const flx_reads* reads);
int  flx_phase_finish(flx_phase* p);
uint64_t flx_phase_num_sites(const flx_phase* p);
int  flx_phase_copy_results(const flx_phase* p, flx_phase_result* out, uint64_t capacity);
uint64_t flx_phase_num_tags(const flx_phase* p);
int  flx_phase_copy_tags(const flx_phase* p, flx_phase_tag* out, uint64_t capacity);
int  flx_phase_geometry(uint32_t out[4]);
int  flx_phase_host(const uint8_t* ref_ranks_concat, const uint64_t* ref_lens, uint32_t n_refs, const flx_phase_options* o,
                    const flx_phase_site* sites, uint64_t n_sites, const flx_record* records, uint64_t n, const uint32_t* cigar_words,
                    uint64_t n_words, const uint8_t* read_pool, const uint64_t* read_offsets, uint64_t n_reads, flx_phase_result* results,
                    flx_phase_tag* tags, uint64_t* n_tags);

/* ------------------------------------------------------------------------------------------------ structural-variant calls
 * Not floxer's, and the step behind the structural-variant signatures: the DEL and INS clusters of an flx_sv object genotyped from the
 * same records. What flx_sv does not keep is how many counted records cover a cluster's locus without carrying the event; this rule
 * counts them. Three forms run the one rule: flx_svcall_host (all records in one call, no device), the flx_svcaller object below (fed
 * batch by batch, on a device or, with device -1, on the host) and the tool floxer_sv. The rule
 * (floxer_amd/csrc/flx_svcall.hpp), integer arithmetic throughout:
 *   - which records count and what is refused: coverage's, with count_secondary and min_mapq; records and words, no reads;
 *   - a span: [rs, re) on sequence ref, rs the record's position, re = rs + the summed = X D lengths;
 *   - the clusters are an array as flx_sv_copy_clusters returns it. Refused (FLX_ERR_INVALID, nothing written): a type above 2, a
 *     reference id outside the lengths (a DEL or INS with ref_b != ref_a too), pos_a_min > pos_a_max, a DEL or INS without
 *     q_min <= q_median <= q_max, a DEL with pos_a_max + q_max past its sequence, an INS with pos_a_max at or past its sequence's
 *     end, a non-zero reserved field. BND clusters are accepted and get no row;
 *   - the count of a DEL or INS cluster on sequence r of length n_r: lo = pos_a_min, hi = pos_a_max + q_max (DEL) or pos_a_max + 1
 *     (INS), lo' = lo >= flank ? lo - flank : 0, hi' = min(hi + flank, n_r) (flank: 0 takes 50, at most 2^20); span_n = the spans
 *     with ref == r, rs <= lo' and re >= hi'; alt_n = support; ref_n = span_n > alt_n ? span_n - alt_n : 0; dp = ref_n + alt_n;
 *   - the genotype is flx_variants' of (ref_n, alt_n, 0) with its five costs, their defaults 36 / 1574 / 325 / 3000 / 3301 and its
 *     checks; pass = 1 iff gt != 0, dp >= min_depth (0 takes 4) and qual >= min_qual (0 takes 2000);
 *   - one row per DEL / INS cluster in the input's order, failing ones included; `cluster` is the index in the input.
 * Known limits: a carrier that does not span the flanks counts in alt_n and not in span_n, so ref_n errs low by at most that many; a
 * record with two signatures in one cluster counts twice in alt_n; single linkage is inherited from the clusters; BND clusters are not
 * called; there is no inserted sequence; an event larger than the read's error budget leaves the read unmapped and is never seen. The
 * defaults are conventions of this project, fitted to nothing.
 * flx_svcall_host: *n_rows holds the capacity on entry and the need on return (FLX_ERR_CAPACITY when too small; nothing else is
 * written then). */
typedef struct flx_svcall_options {
    uint32_t count_secondary, min_mapq, flank, min_depth, min_qual, cost_match, cost_mismatch, cost_het, prior_het, prior_hom;
    uint32_t reserved[2];
} flx_svcall_options;
typedef struct flx_svcall_row {
    uint32_t cluster, type;
    int32_t ref;
    uint32_t pos_a_min, pos_a_max, q_min, q_median, q_max, alt_n, ref_n, span_n, gt, gq, qual, pl[3], pass;
} flx_svcall_row;
int  flx_svcall_host(const uint64_t* ref_lens, uint32_t n_refs, const flx_svcall_options* o, const flx_record* records, uint64_t n,
                     const uint32_t* cigar_words, uint64_t n_words, const flx_sv_cluster* clusters, uint64_t n_clusters, flx_svcall_row* rows,
                     uint64_t* n_rows);

/* The object: one span per counted record, added run by run, then the rows of the clusters that flx_sv_copy_clusters gave.
 *   - create: for a context's index (counted there: flx_ctx_destroy refuses while one is alive) or for reference lengths on
 *     hip_device; hip_device -1 is the host form, which touches nothing of the device and keeps the spans in host memory.
 *     initial_capacity: the spans the table holds before it first grows by doubling (0 takes 2^16; a test hook).
 *   - add_records / add_run: judged like flx_svcall_host's records (coverage's refusals and messages); a refused add leaves the object
 *     as it was. A run made without CIGARs is refused, with min_mapq also a run made without flx_output_options.mapq. Several host
 *     threads may add at once. More than 2^32 - 1 spans: FLX_ERR_CAPACITY. FLX_ERR_INTERNAL: a kernel found a record at odds with
 *     the host's judgement; the add is not counted.
 *   - absorb: `from`'s spans move into `into` (equal lengths and options, both unfinished, both on devices - which may differ - or
 *     both host forms); `from` is left empty.
 *   - finish is final: it judges the clusters as flx_svcall_host does (a refusal is FLX_ERR_INVALID and leaves the object unfinished
 *     and unchanged, so that a later finish with good clusters works), orders the spans and makes one row per DEL / INS cluster in
 *     the input's order. Behind it a further add, absorb or finish is FLX_ERR_INVALID. num_spans, num_rows and max_span (the longest
 *     span, which bounds every window) are 0 before it, and the copy calls are refused.
 *   - copy_spans: the spans [from, to) in (ref, rs, re) order; a stretch outside them is FLX_ERR_INVALID.
 *   - copy_rows: capacity is the number of rows `out` holds. capacity < num_rows: FLX_ERR_CAPACITY and nothing is written;
 *     otherwise exactly num_rows rows are written. out may be NULL only when there are no rows.
 *   - geometry: out = {the most blocks of an svcall_spans launch, the most blocks of an svcall_count launch, the waves of a block (a
 *     wave takes one record or one row at a time), the sort's tile in keys}. */
typedef struct flx_svcaller flx_svcaller;
typedef struct flx_svcall_span { int32_t ref; uint32_t rs, re, reserved; } flx_svcall_span;
int  flx_svcaller_create(flx_ctx* ctx, const flx_svcall_options* o, flx_svcaller** out);
int  flx_svcaller_create_for_lengths(int hip_device, const uint64_t* ref_lens, uint32_t n_refs, const flx_svcall_options* o,
                                     uint64_t initial_capacity, flx_svcaller** out);
void flx_svcaller_free(flx_svcaller* s);
int  flx_svcaller_add_records(flx_svcaller* s, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words);
int  flx_svcaller_add_run(flx_svcaller* s, const flx_run* run);
int  flx_svcaller_absorb(flx_svcaller* into, flx_svcaller* from);
int  flx_svcaller_finish(flx_svcaller* s, const flx_sv_cluster* clusters, uint64_t n_clusters);
uint64_t flx_svcaller_num_spans(const flx_svcaller* s);
uint64_t flx_svcaller_num_rows(const flx_svcaller* s);
uint32_t flx_svcaller_max_span(const flx_svcaller* s);
int  flx_svcaller_copy_spans(const flx_svcaller* s, uint64_t from, uint64_t to, flx_svcall_span* out);
int  flx_svcaller_copy_rows(const flx_svcaller* s, flx_svcall_row* out, uint64_t capacity);
int  flx_svcaller_geometry(uint32_t out[4]);

/* ------------------------------------------------------------------------------------------------ PAF output
 * Not floxer's. A PAF line carries no SEQ, QUAL or CIGAR but per record numbers that are reductions over its CIGAR words: a summary.
 * The rule (floxer_amd/csrc/flx_paf.hpp), for a record with flag & 4 clear and reference_id >= 0, words len << 4 | op with = 7, X 8,
 * I 1, D 2, S 4:
 *     lead / trail = the summed S words in front of the first / behind the last non-S word;
 *     matches, mismatches, ins_bases, del_bases = the summed lengths of the = X I D words;
 *     gap_opens = the I and D words that are the record's first word or whose predecessor has another op;
 *     ref_end = position + matches + mismatches + del_bases;
 *     query_start, query_end on the read as given: lead and read_len - trail, with flag & 16 trail and read_len - lead.
 *   - a record with flag & 4 or reference_id < 0 gets all zeros; secondary and supplementary records are summarised like any other;
 *   - refused (FLX_ERR_INVALID, on the host before any launch; `out` stays as it was): a mapped record without words (a without_cigar
 *     run), an op other than = X I D S, a zero-length word, a reference_id outside the list, a negative position, a span that ends
 *     behind its sequence, words outside the pool, an S word with non-S words on both sides, a read_index outside the reads,
 *     lead + matches + mismatches + ins_bases + trail != the read's length, no reference-consuming column, a sum of 2^31 or more;
 *   - flx_paf_summarize judges on the host, uploads one 24-byte job per record and the stretch of the word pool the records use, runs
 *     paf_summarise (floxer_amd/csrc/flx_paf.hip: one wave per record, 64 words per pass) and downloads 32 bytes per record. n == 0:
 *     FLX_OK without a launch. A record the kernel still finds in breach of the rule has 0xFFFFFFFF in every field and the call returns
 *     FLX_ERR_INTERNAL. The object owns its stream and its grow-only device buffers; a failed growth is FLX_ERR_NO_DEVICE and leaves
 *     the object as it was. Calls on one object may come from several host threads: the records are judged outside the object's lock,
 *     upload, launch and download are serialised inside it. hip_device = -1: no device is opened and the call applies the host rule;
 *   - flx_paf_summarize_host: the rule alone on the host, no device.
 * FLX_PAF_PROFILE (environment): every flx_paf_summarize prints its records, words, uploaded bytes, the kernel's device time and the
 * call's wall time to stderr.
 *
 * The writer is host-only and writes one line per mapped record in call order, the fields separated by tabs:
 *     qname qlen query_start query_end strand tname tlen position ref_end matches block mapq, block = matches + mismatches + ins_bases +
 *     del_bases, mapq 255 or, with mapq_from_records, flx_record.reserved (above 254: FLX_ERR_INVALID, as flx_sam_set_mapq has it),
 *     then tp:A:S for flag & 256 and tp:A:P otherwise (supplementary records are P, as in minimap2), NM:i: with num_errors, AS:i: when
 *     scores are given, de:f: the gap-compressed divergence (mismatches + gap_opens) / (matches + mismatches + gap_opens) rounded half
 *     up to four decimals in integers, cg:Z: with write_cigar (the record's own words as <len><op>, = and X kept, S included: minimap2's
 *     --eqx form), cs:Z: when cs_refs is given and the record's length there is above 0.
 * skip_secondary leaves out records with flag & 256; write_unmapped writes `qname qlen 0 0 * * 0 0 0 0 0 0` (minimap2's --paf-no-hit
 * form, no tags) for a record with flag & 4 or reference_id < 0, which otherwise produces no line. A call is formatted in full before
 * any byte of it is written: a refused call (a summary whose fields are all 0xFFFFFFFF, a summary without columns, a mapped record
 * outside the references, a cs byte outside [0-9:*+=acgtnACGTN-]) writes nothing. options NULL: all zero; the switches are 0 or 1 and
 * the reserved fields 0. */
typedef struct flx_paf flx_paf;
typedef struct flx_paf_summary { uint32_t query_start, query_end, ref_end, matches /* = */, mismatches /* X */, ins_bases, del_bases, gap_opens; } flx_paf_summary;
typedef struct flx_paf_options { uint32_t write_cigar, write_unmapped, mapq_from_records, skip_secondary; uint32_t reserved[4]; } flx_paf_options;
typedef struct flx_paf_writer flx_paf_writer;
int  flx_paf_create(int hip_device, flx_paf** out);
void flx_paf_free(flx_paf* p);
int  flx_paf_summarize(flx_paf* p, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words,
                       const uint64_t* read_offsets, uint64_t n_reads, const uint64_t* ref_lens, uint32_t n_refs, flx_paf_summary* out);
int  flx_paf_summarize_host(const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words,
                            const uint64_t* read_offsets, uint64_t n_reads, const uint64_t* ref_lens, uint32_t n_refs, flx_paf_summary* out);
int  flx_paf_open(const char* path, const char* const* ref_ids, const uint64_t* ref_lens, uint32_t n_refs, const flx_paf_options* o,
                  flx_paf_writer** out);
int  flx_paf_write(flx_paf_writer* w, const char* const* read_ids, const uint64_t* read_offsets, const flx_record* records, uint64_t n,
                   const uint32_t* cigar_words, const flx_paf_summary* summaries, const int32_t* scores /* may be NULL */,
                   const flx_md_ref* cs_refs /* may be NULL */, const uint8_t* cs_bytes);
int  flx_paf_close(flx_paf_writer* w);

uint64_t flx_run_num_records(const flx_run* run);
uint64_t flx_run_num_cigar_words(const flx_run* run);
int flx_run_copy(const flx_run* run, flx_record* records, uint32_t* cigar_words, uint8_t* skipped);
void flx_run_free(flx_run* run);

/* ------------------------------------------------------------------------------------------------ measurement
 * Per-kernel accounting (bench.py): when enabled every launch is bracketed with HIP events on the launch stream. */
typedef struct flx_kernel_stat {
    char name[32];
    uint64_t launches;
    double device_ms;            /* sum of hipEventElapsedTime over the launches */
    uint64_t algorithmic_bytes;  /* bytes the algorithm must move, summed over launches */
    uint64_t work_units;         /* word-steps / rank queries / locates, per kernel */
} flx_kernel_stat;
int flx_ctx_enable_kernel_timing(flx_ctx* ctx, int enable);
int flx_ctx_reset_kernel_stats(flx_ctx* ctx);
int flx_ctx_get_kernel_stats(flx_ctx* ctx, flx_kernel_stat* out, uint32_t* n /* in: capacity, out: count */);

/* Counters of the path since the context was made / they were reset (all batches of all host threads): how many seeds the device
 * handled by itself, how much of the requested DP work was run after de-duplication. Cheap, always on. */
typedef struct flx_path_counters {
    uint64_t seeds, seeds_with_anchors, seeds_excluded_by_hard_cap, seeds_selected_on_host, anchors, cursor_extensions;
    uint64_t inner_tests_requested, root_alignments_requested, root_alignments_found, records, reads;
    uint64_t search_reruns;      /* search launches repeated because a chunk's hits or queued subtrees outgrew their buffers */
    uint64_t reserved[4];        /* reserved[0]: records_dropped, the records flx_output_options left out (records counts those written);
                                    reserved[1]: partial records written (those of split reads included), reserved[2]: reads they rescued
                                    (flx_partial_options); reserved[3]: reads split (flx_split_options) */
} flx_path_counters;
int flx_ctx_get_path_counters(flx_ctx* ctx, flx_path_counters* out);
int flx_ctx_reset_path_counters(flx_ctx* ctx);

/* What the work sharing of the search kernel did, summed over every search launch (repeated ones included) of the context since it was
 * made or flx_ctx_reset_path_counters was called: the device's own counters of each launch, added up on the host when they come back
 * with the launch's other results. Which lane or wave takes a subtree depends on scheduling: the last three differ from run to run,
 * the results of the search never do. */
typedef struct flx_search_counters {
    uint64_t launches;           /* search launches */
    uint64_t subtrees_queued;    /* one-row subtrees queued for the walk against the text */
    uint64_t lane_handovers;     /* subtrees an idle lane took from a busy lane of its wave */
    uint64_t wave_handovers;     /* subtrees a wave handed to a wave that had run out of work */
    uint64_t walks_abandoned;    /* walks given up because their seed had passed the hard cap in another lane or wave */
    uint64_t reserved[3];
} flx_search_counters;
int flx_ctx_get_search_counters(flx_ctx* ctx, flx_search_counters* out);

/* The climb alone (a test hook for the kernels of the verification rounds, like flx_search_groups for K1): the reads' PEX trees as
 * flx_align_reads_resident plans them, the caller's anchors instead of a search's, then the rounds; no search, no interval pass, no
 * trace. anchors[i].read is the read's index in the batch; the anchors must come in (read, orientation) order, as a search leaves them.
 * out_status[i]: 0 = dead, 1 = at the root; out_node[i]: the inner node the anchor failed at, or the root's index (0xFFFFFFFF when the
 * anchor never had an inner node: direct_full_verification, or a tree of one node). Anchors enter alive and below the root; the states
 * a run never hands to the rounds (already dead, already at the root with a node to test) cannot be given. Refused with FLX_ERR_INVALID
 * before any launch: anchors out of order, a read that the input rules skip, a leaf outside the read's tree, a reference outside the
 * index, a position whose leaf (less its errors) does not lie inside the reference sequence.
 * options (NULL: all zero): driver 0 = the device rounds, 1 = the host rounds (per call; FLX_HOST_ROUNDS is not read).
 * out_requests (may be NULL): the call's flx_path_counters.inner_tests_requested - the device rounds count an anchor that is tested
 * alone again in its next round, the host rounds count every request once, so the difference of the two drivers on one input is the
 * number of anchors the device sent on alone. The context's counters are not touched. */
typedef struct flx_climb_anchor { uint32_t read, orientation, leaf, reference_id; uint64_t position; } flx_climb_anchor;
typedef struct flx_climb_options { uint32_t driver, reserved[3]; } flx_climb_options;
int flx_climb_anchors(flx_ctx* ctx, const flx_params* params, const flx_reads* reads, const flx_climb_anchor* anchors, uint64_t n_anchors,
                      const flx_climb_options* options, uint8_t* out_status, uint32_t* out_node, uint64_t* out_requests);

/* The tables a context derives from its image when it is made (a test hook for isa_kernel and filter_build_kernel, like flx_climb_anchors
 * for the rounds): read back from HBM as they are, nothing in the context changes. flx_ctx_derived_info: the presence filter's K and the
 * shortest string it answers for (both 0 without a filter), and which tables this context has (FLX_NO_DERIVED=1, FLX_FILTER_K=0 or a
 * device without room leave them out; the mirrored filter only with FLX_MIRRORED_FILTER=1).
 * flx_ctx_copy_derived: which = 0 the inverse suffix array (text_length u32: ISA[SA[row]] = row), 1 the presence filter, 2 the mirrored
 * filter (each (4^K + 63) / 64 u64 words; bit numbering in DESIGN.md section 3). bytes must be exactly the table's size; a table the
 * context does not have, another size, an unknown `which` or a null argument: FLX_ERR_INVALID with an error text, nothing copied. */
typedef struct flx_derived_info { uint32_t filter_k, filter_tmin, have_isa, have_filter, have_filter_mirrored, reserved[3]; } flx_derived_info;
int flx_ctx_derived_info(flx_ctx* ctx, flx_derived_info* out);
int flx_ctx_copy_derived(flx_ctx* ctx, int which, void* out, uint64_t bytes);

/* The hardware queues the library asked the HIP runtime for when it was loaded. The runtime spreads a process's streams over
 * GPU_MAX_HW_QUEUES hardware queues and kernels of streams that share a queue do not overlap, so at load the library writes
 * FLX_HW_QUEUES into that variable, over whatever is there: default 16 (also for a value that is no number), clamped to 4 .. 32;
 * FLX_HW_QUEUES=0 leaves the variable exactly as it was found. The runtime reads the variable when it initialises: a host program
 * that makes its first HIP call before it loads the library sets the variable itself.
 * requested (may be NULL): what the library wrote, 0 if it left the variable alone; found (may be NULL): the variable's value on
 * entry, -1 if it was unset. */
int flx_hw_queue_request(int* requested, int* found);

/* Do the lanes' streams overlap on the GPU (a test hook; nothing of a run's path is touched): on each of the first n_lanes lanes' own
 * streams an event, one kernel of one wave that runs a dependent integer chain of `iterations` steps (capped at 1 << 24) and reads
 * nothing, and a second event; all lanes are waited for. start_ms / stop_ms (n_lanes floats each): the events' times in ms behind a
 * reference event recorded first. Kernels of lanes that share a hardware queue show up one behind the other. The context must be
 * idle. n_lanes 0 or above the context's lanes, or a null argument: FLX_ERR_INVALID. */
int flx_ctx_lane_overlap(flx_ctx* ctx, uint32_t n_lanes, uint32_t iterations, float* start_ms, float* stop_ms);

/* ------------------------------------------------------------------------------------------------ statistics (--stats)
 * replaces statistics::search_and_alignment_statistics (include/statistics.hpp:24-172, src/lib/statistics.cpp): the reference's
 * count and eighteen histograms, same names, thresholds and renderings. input_hint: NULL / "real_nanopore" / "simulated"
 * (statistics.cpp:209-221). A context with a statistics object attached adds every read of every batch it aligns (the flx_stats
 * outlives that; not a configuration call: attach before the first batch). flx_stats_format: toml != 0 the TOML file of
 * format_statistics_as_toml, else the terminal entries of format_statistics_for_stdout separated by blank lines; len: in =
 * capacity, out = bytes needed incl. the terminating 0 (FLX_ERR_CAPACITY when too small). */
typedef struct flx_stats flx_stats;
int flx_stats_create(const char* input_hint, flx_stats** out);
void flx_stats_free(flx_stats* stats);
int flx_stats_merge(flx_stats* into, const flx_stats* other);
uint64_t flx_stats_num_queries(const flx_stats* stats);
int flx_stats_format(const flx_stats* stats, int toml, char* buf, uint64_t* len);
int flx_ctx_set_stats(flx_ctx* ctx, flx_stats* stats);

/* ------------------------------------------------------------------------------------------------ file boundary
 * FASTA/FASTQ in (input.cpp:36-148), SAM/BAM out (output.cpp:49-108, 197-212) — used by the floxer-compatible CLI. */
typedef struct flx_sam_writer flx_sam_writer;
int flx_sam_open(const char* path /* .sam or .bam */, const char* const* ref_ids, const uint64_t* ref_lens, uint32_t n_refs,
                 flx_sam_writer** out);
int flx_sam_write(flx_sam_writer* w, const char* const* read_ids, const uint8_t* read_pool, const uint64_t* read_offsets,
                  const char* const* quals, const flx_record* records, uint64_t n_records, const uint32_t* cigar_words);
/* flx_sam_write with an MD:Z tag behind NM:i on every mapped record i with md[i].length > 0 (its bytes: md_bytes + md[i].offset). Bytes
 * outside [0-9A-Z^] are refused with FLX_ERR_INVALID. md == NULL: exactly flx_sam_write. */
int flx_sam_write_tagged(flx_sam_writer* w, const char* const* read_ids, const uint8_t* read_pool, const uint64_t* read_offsets,
                         const char* const* quals, const flx_record* records, uint64_t n_records, const uint32_t* cigar_words,
                         const flx_md_ref* md, const uint8_t* md_bytes);
/* flx_sam_write_tagged with an AS:i tag behind NM / MD on every mapped record (scores[i], as flx_run_copy_scores gives them; ASi in BAM).
 * scores == NULL: exactly flx_sam_write_tagged. */
int flx_sam_write_scored(flx_sam_writer* w, const char* const* read_ids, const uint8_t* read_pool, const uint64_t* read_offsets,
                         const char* const* quals, const flx_record* records, uint64_t n_records, const uint32_t* cigar_words,
                         const flx_md_ref* md, const uint8_t* md_bytes, const int32_t* scores);
/* flx_sam_write_scored with a cs:Z tag behind NM / MD / AS and in front of SA on every mapped record i with cs_refs[i].length > 0 (its
 * bytes: cs_bytes + cs_refs[i].offset; csZ...\0 in BAM, where a string that repeats the previous record's is announced to the deflate
 * encoder as MD's is). Bytes outside [0-9:*+=acgtnACGTN-] are refused with FLX_ERR_INVALID. cs_refs == NULL: exactly
 * flx_sam_write_scored. */
int flx_sam_write_cs(flx_sam_writer* w, const char* const* read_ids, const uint8_t* read_pool, const uint64_t* read_offsets,
                     const char* const* quals, const flx_record* records, uint64_t n_records, const uint32_t* cigar_words,
                     const flx_md_ref* md, const uint8_t* md_bytes, const int32_t* scores, const flx_md_ref* cs_refs, const uint8_t* cs_bytes);
int flx_sam_close(flx_sam_writer* w);
/* record formatting and BGZF block compression of flx_sam_write on n_threads host threads (default 1; output bytes do not depend on it) */
int flx_sam_set_threads(flx_sam_writer* w, uint32_t n_threads);
/* MAPQ column: from_records = 0 (default) writes 255, "not available", as floxer does; != 0 writes records[i].reserved (what a run made
 * with flx_output_options.mapq stores there; a value above 254 makes flx_sam_write fail with FLX_ERR_INVALID) */
int flx_sam_set_mapq(flx_sam_writer* w, int from_records);
/* SA:Z tag (not floxer's): on != 0 gives every record of a read that has a flag-2048 record (the partial records of flx_partial_options)
 * the tag behind NM / MD (SAZ...\0 in BAM). It lists the read's other records in written order, each as
 * rname,pos,strand,CIGAR,mapQ,NM; with pos 1-based, strand + or -, the record's own CIGAR with runs of = and X merged into M (ops S, M,
 * I, D) and mapQ what the writer puts into that record's MAPQ column. A read's records must be contiguous within one flx_sam_write
 * call, as in every flx_run. Default off: then no byte changes. */
int flx_sam_set_sa(flx_sam_writer* w, int on);
/* A coordinate-sorted BAM (not floxer's), optionally with its BAI index <path>.bai (SAMv1 5.2). The writer owns a sort object
 * (flx_sort_create) on hip_device; -1 orders on the host, for tests and callers without a device. The setters and all four
 * flx_sam_write* calls work as on any writer. Call k of flx_sam_write* (from 0) adds its records to the sort with first_ordinal
 * k << 32, formats and deflates them in the key order that add returns, and appends the BGZF members to the spill file as run k: fewer
 * than 2^32 records per call. flx_sam_close writes the header with @HD VN:1.6 SO:coordinate, finishes the sort, streams its entries,
 * takes for every entry the next record of run ordinal >> 32 (every run is inflated in sequence), deflates the merged stream into
 * the output, writes the EOF block and the index, and removes the spill file, on failure as well. Records with equal reference,
 * position and strand keep the order they were written in. The output's bytes do not depend on flx_sam_set_threads.
 * The index: records consecutive in the file with the same reference and bin extend one chunk, anything else starts a new one (no
 * further merging); a chunk ends at the virtual offset of the first byte behind its last record (the next block's start when that
 * is a block's end); the linear index has ((max end - 1) >> 14) + 1 windows, an empty one repeats its predecessor (0 in front of
 * the first); bin 37450 holds the reference's first and last offset and its record counts; n_no_coor counts the unplaced records.
 * Refused up front: a path that does not end in .bam (FLX_ERR_INVALID), a spill file or an output that cannot be created (FLX_ERR_IO),
 * write_index with a sequence longer than 2^29 (FLX_ERR_INVALID; the message names it). */
int flx_sam_open_sorted(const char* path /* .bam only */, const char* spill_path, int hip_device, int write_index,
                        const char* const* ref_ids, const uint64_t* ref_lens, uint32_t n_refs, flx_sam_writer** out);

/* ------------------------------------------------------------------------------------------------ synthetic inputs
 * The reference's simulator (src/main/simulated_dataset.cpp:30-49, 81-223), multi-threaded and with a portable generator:
 * uniform genome over ACGT; reads = substrings of base_len with exactly floor(error_rate * base_len) distinct positions mutated
 * (mismatch / insertion / deletion uniformly), reverse-complemented with probability revcomp_fraction. Read r depends on
 * (seed, r) only. out_offsets has n_reads + 1 entries; out_chrom / out_pos / out_reverse (may be NULL) receive the truth. */
int flx_sim_genome(uint64_t length, uint64_t seed, uint8_t* out_ranks);
/* the same length of repeat-rich sequence (interspersed repeat families, tandem repeats, low complexity, runs of N, segmental
 * duplications: about half of the bases unique, as in a human genome): the workload floxer's caps -M / -m (search.cpp:190-272) exist for */
int flx_sim_genome_repeats(uint64_t length, uint64_t seed, uint8_t* out_ranks);
int flx_sim_reads(const uint8_t* genome_concat, const uint64_t* chrom_lens, uint32_t n_chrom, uint64_t n_reads, uint32_t base_len,
                  double error_rate, double revcomp_fraction, uint64_t seed, uint8_t* out_pool, uint64_t pool_capacity,
                  uint64_t* out_offsets, uint32_t* out_chrom, uint64_t* out_pos, uint8_t* out_reverse);

#ifdef __cplusplus
}
#endif
#endif /* FLOXER_AMD_H */
