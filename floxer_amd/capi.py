"""ctypes binding of libfloxer_amd.so (include/floxer_amd.h). The library holds the whole path (HIP kernels + C++ host);
this module only marshals numpy arrays. There is no CPU fallback: without the built library or without a GPU every
device entry point raises FloxerError."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FLX_LIBRARY") or os.path.join(_HERE, "libfloxer_amd.so")      # (FLX_LIBRARY: another build of the library, for A/B runs on one box)

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)


class FloxerError(RuntimeError):
    pass


class PexNode(C.Structure):
    _fields_ = [("parent_id", C.c_uint32), ("from_", C.c_uint32), ("to", C.c_uint32), ("num_errors", C.c_uint32)]


class Seed(C.Structure):
    _fields_ = [("seq_offset", C.c_uint64), ("length", C.c_uint32), ("num_errors", C.c_uint32), ("pex_leaf_index", C.c_uint32),
                ("reserved", C.c_uint32)]


class SearchConfig(C.Structure):
    _fields_ = [("max_num_anchors_hard", C.c_uint64), ("max_num_anchors_soft", C.c_uint64), ("anchor_group_order", C.c_int32),
                ("anchor_choice_strategy", C.c_int32), ("erase_useless_anchors", C.c_int32), ("reserved", C.c_int32)]


class Anchor(C.Structure):
    _fields_ = [("seed_index", C.c_uint32), ("pex_leaf_index", C.c_uint32), ("reference_id", C.c_uint32), ("num_errors", C.c_uint32),
                ("reference_position", C.c_uint64)]


class SeedStats(C.Structure):
    _fields_ = [("num_kept_useful_anchors", C.c_uint32), ("num_kept_raw_anchors", C.c_uint32),
                ("num_excluded_raw_anchors_by_soft_cap", C.c_uint32), ("fully_excluded", C.c_uint32)]


class HitGroup(C.Structure):
    _fields_ = [("seed_index", C.c_uint32), ("lb", C.c_uint32), ("len", C.c_uint32), ("num_errors", C.c_uint32)]


class AlignJob(C.Structure):
    _fields_ = [("ref_offset", C.c_uint64), ("query_offset", C.c_uint64), ("ref_length", C.c_uint32), ("query_length", C.c_uint32),
                ("num_allowed_errors", C.c_uint32), ("mode", C.c_uint32)]


class AlignShape(C.Structure):
    _fields_ = [("words_per_lane", C.c_uint32), ("lanes_per_job", C.c_uint32), ("queue", C.c_uint32)]


class AlignResult(C.Structure):
    _fields_ = [("exists", C.c_uint32), ("num_errors", C.c_uint32), ("begin", C.c_uint64), ("cigar_offset", C.c_uint64),
                ("cigar_length", C.c_uint32), ("reserved", C.c_uint32)]


class Params(C.Structure):
    _fields_ = [("query_error_probability", C.c_double), ("query_num_errors", C.c_uint64), ("pex_seed_num_errors", C.c_uint64),
                ("search", SearchConfig), ("seed_sampling_step_size", C.c_uint64), ("bottom_up_pex_tree_building", C.c_int32),
                ("use_interval_optimization", C.c_int32), ("extra_verification_ratio", C.c_double),
                ("direct_full_verification", C.c_int32), ("without_cigar", C.c_int32),
                ("num_anchors_per_verification_task", C.c_uint64)]


class Record(C.Structure):
    _fields_ = [("read_index", C.c_uint64), ("flag", C.c_uint32), ("reference_id", C.c_int32), ("position", C.c_int32),
                ("num_errors", C.c_uint32), ("cigar_offset", C.c_uint64), ("cigar_length", C.c_uint32), ("reserved", C.c_uint32)]


class OutputOptions(C.Structure):
    _fields_ = [("drop_duplicates", C.c_uint32), ("mapq", C.c_uint32), ("max_alignments_per_read", C.c_uint64),
                ("reserved2", C.c_uint64 * 2)]


class TagOptions(C.Structure):
    _fields_ = [("md", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class PartialOptions(C.Structure):
    _fields_ = [("enable", C.c_uint32), ("min_query_span", C.c_uint32), ("max_records", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class ExtendOptions(C.Structure):
    _fields_ = [("enable", C.c_uint32), ("error_weight", C.c_uint32), ("x_drop", C.c_uint32), ("max_errors", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class RunOptions(C.Structure):
    _fields_ = [("output", C.POINTER(OutputOptions)), ("tags", C.POINTER(TagOptions)), ("partial", C.POINTER(PartialOptions)),
                ("extend", C.POINTER(ExtendOptions)), ("reserved", C.c_void_p * 4)]


class SplitOptions(C.Structure):
    _fields_ = [("enable", C.c_uint32), ("error_weight", C.c_uint32), ("x_drop", C.c_uint32), ("min_tail_rows", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class GapOptions(C.Structure):
    _fields_ = [("left_align", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class LeftAlignJob(C.Structure):
    _fields_ = [("cigar_offset", C.c_uint64), ("cigar_length", C.c_uint32), ("reserved", C.c_uint32), ("ref_offset", C.c_uint64),
                ("ref_length", C.c_uint32), ("begin", C.c_uint32), ("query_offset", C.c_uint64), ("query_length", C.c_uint32),
                ("reserved2", C.c_uint32)]


class CigarRef(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint32), ("reserved", C.c_uint32)]


class RealignOptions(C.Structure):
    _fields_ = [("enable", C.c_uint32), ("match", C.c_uint32), ("mismatch", C.c_uint32), ("gap_open", C.c_uint32), ("gap_extend", C.c_uint32),
                ("band", C.c_uint32), ("reserved", C.c_uint32 * 2)]


RealignJob = LeftAlignJob


class RealignResult(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint32), ("num_errors", C.c_uint32), ("score", C.c_int32), ("diag_lo", C.c_int32),
                ("diag_hi", C.c_int32), ("kept", C.c_uint32)]


class RealignCounters(C.Structure):
    _fields_ = [("paths_realigned", C.c_uint64), ("paths_changed", C.c_uint64), ("paths_kept", C.c_uint64), ("reserved", C.c_uint64 * 5)]


class CsOptions(C.Structure):
    _fields_ = [("form", C.c_uint32), ("reserved", C.c_uint32 * 7)]


CsJob = LeftAlignJob


class CoverageOptions(C.Structure):
    _fields_ = [("count_deletions", C.c_uint32), ("count_secondary", C.c_uint32), ("min_mapq", C.c_uint32), ("report_zero", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class DepthRun(C.Structure):
    _fields_ = [("reference_id", C.c_int32), ("depth", C.c_uint32), ("start", C.c_uint64), ("end", C.c_uint64)]


class DepthWindow(C.Structure):
    _fields_ = [("reference_id", C.c_int32), ("max_depth", C.c_uint32), ("start", C.c_uint64), ("end", C.c_uint64), ("depth_sum", C.c_uint64),
                ("covered", C.c_uint64)]


class PileupOptions(C.Structure):
    _fields_ = [("count_secondary", C.c_uint32), ("min_mapq", C.c_uint32), ("min_depth", C.c_uint32), ("min_count", C.c_uint32),
                ("min_permille", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class PileupSite(C.Structure):
    _fields_ = [("reference_id", C.c_int32), ("position", C.c_uint32), ("depth", C.c_uint32), ("del_", C.c_uint32), ("ins", C.c_uint32),
                ("alt", C.c_uint32 * 4), ("reserved", C.c_uint32)]


class SvOptions(C.Structure):
    _fields_ = [("min_length", C.c_uint32), ("max_distance", C.c_uint32), ("min_support", C.c_uint32), ("count_secondary", C.c_uint32),
                ("min_mapq", C.c_uint32), ("reserved", C.c_uint32 * 3), ("initial_capacity", C.c_uint64)]


class SvSignature(C.Structure):
    _fields_ = [("type", C.c_uint32), ("side_a", C.c_uint32), ("side_b", C.c_uint32), ("reserved", C.c_uint32), ("ref_a", C.c_int32),
                ("ref_b", C.c_int32), ("pos_a", C.c_uint32), ("q", C.c_uint32)]


class SvCluster(C.Structure):
    _fields_ = [("type", C.c_uint32), ("side_a", C.c_uint32), ("side_b", C.c_uint32), ("support", C.c_uint32), ("ref_a", C.c_int32),
                ("ref_b", C.c_int32), ("pos_a_min", C.c_uint32), ("pos_a_max", C.c_uint32), ("q_min", C.c_uint32), ("q_median", C.c_uint32),
                ("q_max", C.c_uint32), ("reserved", C.c_uint32)]


class ErrprofOptions(C.Structure):
    _fields_ = [("count_secondary", C.c_uint32), ("min_mapq", C.c_uint32), ("flush_threshold", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class ConsensusOptions(C.Structure):
    _fields_ = [("count_secondary", C.c_uint32), ("min_mapq", C.c_uint32), ("min_depth", C.c_uint32), ("min_count", C.c_uint32),
                ("min_permille", C.c_uint32), ("mask_low_depth", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class ConsensusChange(C.Structure):
    _fields_ = [("reference_id", C.c_int32), ("position", C.c_uint32), ("kind", C.c_uint32), ("ref_rank", C.c_uint32), ("alt_rank", C.c_uint32),
                ("length", C.c_uint32), ("count", C.c_uint32), ("cov", C.c_uint32), ("letters", C.c_uint64)]


class ConsensusAllele(C.Structure):
    _fields_ = [("reference_id", C.c_int32), ("position", C.c_uint32), ("length", C.c_uint32), ("count", C.c_uint32), ("letters", C.c_uint64)]


class VariantsOptions(C.Structure):
    _fields_ = [("count_secondary", C.c_uint32), ("min_mapq", C.c_uint32), ("min_depth", C.c_uint32), ("min_qual", C.c_uint32), ("max_del", C.c_uint32),
                ("cost_match", C.c_uint32), ("cost_mismatch", C.c_uint32), ("cost_het", C.c_uint32), ("prior_het", C.c_uint32), ("prior_hom", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


class Variant(C.Structure):
    _fields_ = [("reference_id", C.c_int32), ("position", C.c_uint32), ("kind", C.c_uint32), ("ref_rank", C.c_uint32), ("alt_rank", C.c_uint32),
                ("length", C.c_uint32), ("ref_count", C.c_uint32), ("alt_count", C.c_uint32), ("cov", C.c_uint32), ("gt", C.c_uint32), ("gq", C.c_uint32),
                ("qual", C.c_uint32), ("pl", C.c_uint32 * 3), ("reserved", C.c_uint32), ("letters", C.c_uint64)]


class VariantAllele(C.Structure):
    _fields_ = [("reference_id", C.c_int32), ("position", C.c_uint32), ("kind", C.c_uint32), ("length", C.c_uint32), ("count", C.c_uint32),
                ("reserved", C.c_uint32), ("letters", C.c_uint64)]


class PhaseOptions(C.Structure):
    _fields_ = [("count_secondary", C.c_uint32), ("min_mapq", C.c_uint32), ("min_link", C.c_uint32), ("min_margin", C.c_uint32), ("refine_rounds", C.c_uint32),
                ("skip_refine", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class PhaseSite(C.Structure):
    _fields_ = [("reference_id", C.c_int32), ("position", C.c_uint32), ("kind", C.c_uint32), ("alt_rank", C.c_uint32), ("length", C.c_uint32), ("reserved", C.c_uint32),
                ("letters", C.c_uint64)]


class PhaseResult(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("phase_set", "phased", "phase", "cis", "trans", "keep", "swap", "reserved")]


class PhaseTag(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("add", "read", "hap", "phase_set", "h1", "h2", "n_slots", "reserved")]


class SvcallOptions(C.Structure):
    _fields_ = [("count_secondary", C.c_uint32), ("min_mapq", C.c_uint32), ("flank", C.c_uint32), ("min_depth", C.c_uint32), ("min_qual", C.c_uint32),
                ("cost_match", C.c_uint32), ("cost_mismatch", C.c_uint32), ("cost_het", C.c_uint32), ("prior_het", C.c_uint32), ("prior_hom", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


class SvcallRow(C.Structure):
    _fields_ = [("cluster", C.c_uint32), ("type", C.c_uint32), ("ref", C.c_int32), ("pos_a_min", C.c_uint32), ("pos_a_max", C.c_uint32), ("q_min", C.c_uint32),
                ("q_median", C.c_uint32), ("q_max", C.c_uint32), ("alt_n", C.c_uint32), ("ref_n", C.c_uint32), ("span_n", C.c_uint32), ("gt", C.c_uint32),
                ("gq", C.c_uint32), ("qual", C.c_uint32), ("pl", C.c_uint32 * 3), ("pass", C.c_uint32)]


class SvcallSpan(C.Structure):
    _fields_ = [("ref", C.c_int32), ("rs", C.c_uint32), ("re", C.c_uint32), ("reserved", C.c_uint32)]


# flx_errprof_table: its sections in their fixed order, u64 each
ERRPROF_SECTIONS = (("PAIR_EQ", 36), ("PAIR_X", 36), ("INS_LEN", 64), ("DEL_LEN", 64), ("INS_LETTER", 6), ("DEL_LETTER", 6), ("HP_DEL", 34), ("HP_INS", 34),
                    ("POS_MATCH", 100), ("POS_MISMATCH", 100), ("POS_INS", 100), ("POS_CLIP", 100), ("POS_DEL", 100), ("EQ_RUN", 256), ("IDENTITY", 101),
                    ("TOTALS", 8), ("reserved", 7))


class ErrprofTable(C.Structure):
    _fields_ = [(name, C.c_uint64 * n) for name, n in ERRPROF_SECTIONS]


class SortOptions(C.Structure):
    _fields_ = [("initial_capacity", C.c_uint64), ("tile_keys", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class SortEntry(C.Structure):
    _fields_ = [("ordinal", C.c_uint64), ("reference_id", C.c_int32), ("position", C.c_int32), ("end", C.c_uint32), ("flag", C.c_uint32)]


class PafSummary(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("query_start", "query_end", "ref_end", "matches", "mismatches", "ins_bases", "del_bases", "gap_opens")]


class PafOptions(C.Structure):
    _fields_ = [("write_cigar", C.c_uint32), ("write_unmapped", C.c_uint32), ("mapq_from_records", C.c_uint32), ("skip_secondary", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class TailJob(C.Structure):
    _fields_ = [("cigar_offset", C.c_uint64), ("cigar_length", C.c_uint32), ("error_weight", C.c_uint32), ("x_drop", C.c_uint32),
                ("min_tail_rows", C.c_uint32)]


class TailResult(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("left_rows", "left_cols", "left_errors", "left_words", "right_rows", "right_cols", "right_errors",
                                          "right_words")]


class ExtendJob(C.Structure):
    _fields_ = [("text_pos", C.c_uint64), ("q_pos", C.c_uint64), ("ref_limit", C.c_uint32), ("row_limit", C.c_uint32),
                ("direction", C.c_int32), ("error_weight", C.c_uint32), ("x_drop", C.c_uint32), ("max_errors", C.c_uint32)]


class ExtendResult(C.Structure):
    _fields_ = [("rows", C.c_uint32), ("cols", C.c_uint32), ("errors", C.c_uint32), ("stop_reason", C.c_uint32)]


class PartialCandidate(C.Structure):
    _fields_ = [("read_index", C.c_uint64), ("q_from", C.c_uint32), ("q_to", C.c_uint32), ("orientation", C.c_uint32),
                ("reference_id", C.c_int32), ("start", C.c_uint64), ("nm", C.c_uint32), ("cigar_length", C.c_uint32),
                ("cigar_offset", C.c_uint64)]


class MdRef(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint32), ("reserved", C.c_uint32)]


class PathCounters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("seeds", "seeds_with_anchors", "seeds_excluded_by_hard_cap", "seeds_selected_on_host", "anchors",
                                          "cursor_extensions", "inner_tests_requested", "root_alignments_requested",
                                          "root_alignments_found", "records", "reads", "search_reruns")] + [("reserved", C.c_uint64 * 4)]


class SearchCounters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("launches", "subtrees_queued", "lane_handovers", "wave_handovers", "walks_abandoned")] + [("reserved", C.c_uint64 * 3)]


class ClimbAnchor(C.Structure):
    _fields_ = [("read", C.c_uint32), ("orientation", C.c_uint32), ("leaf", C.c_uint32), ("reference_id", C.c_uint32), ("position", C.c_uint64)]


class ClimbOptions(C.Structure):
    _fields_ = [("driver", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class DerivedInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("filter_k", "filter_tmin", "have_isa", "have_filter", "have_filter_mirrored")] + [("reserved", C.c_uint32 * 3)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_uint64), ("device_ms", C.c_double), ("algorithmic_bytes", C.c_uint64),
                ("work_units", C.c_uint64)]


# every symbol include/floxer_amd.h declares (tests check that the library exports all of them)
EXPORTED = [
    "flx_last_error", "flx_version", "flx_ceil_div", "flx_floating_point_error_aware_ceil", "flx_saturate_value_to_int32_max",
    "flx_chars_to_rank_sequence", "flx_reverse_complement_rank", "flx_pex_tree_build", "flx_index_build", "flx_index_build_on_device", "flx_index_save",
    "flx_index_load", "flx_index_free", "flx_index_text_length", "flx_index_num_references", "flx_index_device_bytes", "flx_index_derived_device_bytes",
    "flx_index_copy_sa", "flx_index_copy_sa_u32", "flx_index_copy_bwt", "flx_ctx_create", "flx_ctx_destroy", "flx_ctx_set_stream", "flx_search_seeds",
    "flx_search_groups", "flx_align_batch", "flx_params_default", "flx_align_reads", "flx_reads_upload", "flx_reads_free",
    "flx_align_reads_resident", "flx_run_num_records",
    "flx_run_num_cigar_words", "flx_run_copy", "flx_run_free", "flx_ctx_enable_kernel_timing", "flx_ctx_reset_kernel_stats",
    "flx_ctx_get_kernel_stats", "flx_sam_open", "flx_sam_write", "flx_sam_close", "flx_sim_genome", "flx_sim_genome_repeats", "flx_sim_reads", "flx_ctx_get_path_counters",
    "flx_ctx_reset_path_counters", "flx_stats_create", "flx_stats_free", "flx_stats_merge", "flx_stats_num_queries", "flx_stats_format",
    "flx_ctx_set_stats", "flx_device_count", "flx_index_matches_reference", "flx_sam_set_threads", "flx_index_image_layout",
    "flx_index_image_upload", "flx_index_meta_export", "flx_index_meta_import", "flx_ctx_create_on_image",
    "flx_align_reads_with_options", "flx_align_reads_resident_with_options", "flx_select_records", "flx_assign_mapq", "flx_sam_set_mapq",
    "flx_align_reads_with_tags", "flx_align_reads_resident_with_tags", "flx_run_num_md_bytes", "flx_run_copy_md", "flx_align_batch_md",
    "flx_sam_write_tagged", "flx_align_reads_opt", "flx_align_reads_resident_opt", "flx_choose_partials", "flx_partial_mapq",
    "flx_extend_batch", "flx_sam_set_sa", "flx_align_reads_split", "flx_align_reads_resident_split", "flx_cigar_tails", "flx_cigar_tails_batch",
    "flx_align_shapes", "flx_align_reads_gaps", "flx_align_reads_resident_gaps", "flx_align_batch_gaps", "flx_left_align", "flx_left_align_batch",
    "flx_realign", "flx_realign_batch", "flx_align_batch_realign", "flx_ctx_get_realign_counters", "flx_align_reads_realign",
    "flx_align_reads_resident_realign", "flx_run_copy_scores", "flx_sam_write_scored",
    "flx_ctx_get_search_counters", "flx_climb_anchors", "flx_ctx_derived_info", "flx_ctx_copy_derived",
    "flx_hw_queue_request", "flx_ctx_lane_overlap",
    "flx_align_reads_cs", "flx_align_reads_resident_cs", "flx_run_num_cs_bytes", "flx_run_copy_cs", "flx_align_batch_cs", "flx_cs", "flx_cs_batch",
    "flx_sam_write_cs",
    "flx_coverage_create", "flx_coverage_create_for_lengths", "flx_coverage_free", "flx_coverage_add_run", "flx_coverage_add_records",
    "flx_coverage_absorb", "flx_coverage_finish", "flx_coverage_num_runs", "flx_coverage_copy_runs", "flx_coverage_num_windows",
    "flx_coverage_copy_windows", "flx_coverage_copy_depth", "flx_coverage_geometry", "flx_coverage_host",
    "flx_pileup_create", "flx_pileup_create_for_lengths", "flx_pileup_free", "flx_pileup_add_records", "flx_pileup_add_run",
    "flx_pileup_add_run_resident", "flx_pileup_absorb", "flx_pileup_finish", "flx_pileup_num_sites", "flx_pileup_copy_sites",
    "flx_pileup_copy_counts", "flx_pileup_host", "flx_pileup_sites_host",
    "flx_sort_create", "flx_sort_free", "flx_sort_add_records", "flx_sort_add_run", "flx_sort_finish", "flx_sort_num_records", "flx_sort_copy",
    "flx_sort_geometry", "flx_sort_host", "flx_sam_open_sorted",
    "flx_paf_create", "flx_paf_free", "flx_paf_summarize", "flx_paf_summarize_host", "flx_paf_open", "flx_paf_write", "flx_paf_close",
    "flx_sv_create", "flx_sv_create_for_lengths", "flx_sv_free", "flx_sv_add_records", "flx_sv_add_run", "flx_sv_absorb", "flx_sv_finish",
    "flx_sv_num_signatures", "flx_sv_copy_signatures", "flx_sv_num_clusters", "flx_sv_copy_clusters", "flx_sv_host", "flx_sv_clusters_host",
    "flx_errprof_create", "flx_errprof_create_for_text", "flx_errprof_free", "flx_errprof_add_records", "flx_errprof_add_run",
    "flx_errprof_add_run_resident", "flx_errprof_absorb", "flx_errprof_copy", "flx_errprof_host",
    "flx_consensus_create", "flx_consensus_create_for_text", "flx_consensus_free", "flx_consensus_add_records", "flx_consensus_add_run",
    "flx_consensus_add_run_resident", "flx_consensus_finish", "flx_consensus_num_letters", "flx_consensus_copy_letters",
    "flx_consensus_num_changes", "flx_consensus_copy_changes", "flx_consensus_num_alleles", "flx_consensus_copy_alleles",
    "flx_consensus_geometry", "flx_consensus_host",
    "flx_variants_create", "flx_variants_create_for_text", "flx_variants_free", "flx_variants_add_records", "flx_variants_add_run",
    "flx_variants_add_run_resident", "flx_variants_finish", "flx_variants_num_rows", "flx_variants_copy_rows", "flx_variants_num_alleles",
    "flx_variants_copy_alleles", "flx_variants_geometry", "flx_variants_genotype", "flx_variants_host",
    "flx_phase_create", "flx_phase_create_for_text", "flx_phase_free", "flx_phase_add_records", "flx_phase_add_run", "flx_phase_add_run_resident",
    "flx_phase_finish", "flx_phase_num_sites", "flx_phase_copy_results", "flx_phase_num_tags", "flx_phase_copy_tags", "flx_phase_geometry", "flx_phase_host",
    "flx_svcall_host",
    "flx_svcaller_create", "flx_svcaller_create_for_lengths", "flx_svcaller_free", "flx_svcaller_add_records", "flx_svcaller_add_run", "flx_svcaller_absorb",
    "flx_svcaller_finish", "flx_svcaller_num_spans", "flx_svcaller_num_rows", "flx_svcaller_max_span", "flx_svcaller_copy_spans", "flx_svcaller_copy_rows",
    "flx_svcaller_geometry",
    "flx_grid_caps",
]

_lib = None


def _share_torchs_hip_runtime():
    """One HIP runtime per process. A ROCm build of PyTorch brings its own libamdhip64.so (soname libamdhip64.so.7, like the system's)
    and looks it up by path, so a process that loads this library first and torch later ends up with two runtimes, and the second
    one cannot attach to the GPU (KFD gives a process one VM: AMDKFD_IOC_ACQUIRE_VM fails, torch reports "No HIP GPUs are
    available"). Loading torch's copy first makes the dynamic loader hand the same copy to this library (it asks for the soname)
    and to torch whenever it comes. Nothing is imported; FLX_SYSTEM_HIP=1 keeps the system's runtime (then import torch never, or
    before floxer_amd's first call)."""
    if os.environ.get("FLX_SYSTEM_HIP") == "1" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(path):
        C.CDLL(path, mode=C.RTLD_GLOBAL)


def hip_runtime_paths():
    """the libamdhip64 copies mapped into this process (one, unless something went wrong)"""
    with open("/proc/self/maps") as f:
        return sorted({line.split()[-1] for line in f if "libamdhip64" in line})


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FloxerError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(floxer_amd has no CPU fallback)")
    _share_torchs_hip_runtime()
    L = C.CDLL(LIB_PATH)
    # (the library writes its hardware-queue request into the process's environment when it is loaded, flx_hw_queue_request; os.environ is
    # Python's copy from start-up, which child processes inherit: it follows)
    getenv = C.CDLL(None).getenv
    getenv.restype, getenv.argtypes = C.c_char_p, [C.c_char_p]
    value = getenv(b"GPU_MAX_HW_QUEUES")
    if value is None:
        os.environ.pop("GPU_MAX_HW_QUEUES", None)
    else:
        os.environ["GPU_MAX_HW_QUEUES"] = value.decode()
    L.flx_last_error.restype = C.c_char_p
    L.flx_version.restype = C.c_char_p
    L.flx_ceil_div.restype = C.c_uint64
    L.flx_ceil_div.argtypes = [C.c_uint64, C.c_uint64]
    L.flx_floating_point_error_aware_ceil.restype = C.c_uint64
    L.flx_floating_point_error_aware_ceil.argtypes = [C.c_double]
    L.flx_saturate_value_to_int32_max.restype = C.c_int32
    L.flx_saturate_value_to_int32_max.argtypes = [C.c_uint64]
    L.flx_chars_to_rank_sequence.argtypes = [C.c_char_p, C.c_uint64, u8p]
    L.flx_reverse_complement_rank.argtypes = [u8p, C.c_uint64, u8p]
    L.flx_pex_tree_build.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(PexNode), C.c_uint64, u64p, u64p]
    L.flx_index_build.argtypes = [u8p, u64p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.flx_index_build_on_device.argtypes = [C.c_int, u8p, u64p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.flx_index_save.argtypes = [C.c_void_p, C.c_char_p]
    L.flx_index_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.flx_index_free.argtypes = [C.c_void_p]
    L.flx_index_text_length.restype = C.c_uint64
    L.flx_index_text_length.argtypes = [C.c_void_p]
    L.flx_index_num_references.restype = C.c_uint32
    L.flx_index_num_references.argtypes = [C.c_void_p]
    L.flx_index_device_bytes.restype = C.c_uint64
    L.flx_index_device_bytes.argtypes = [C.c_void_p]
    L.flx_index_derived_device_bytes.restype = C.c_uint64
    L.flx_index_derived_device_bytes.argtypes = [C.c_void_p]
    L.flx_index_copy_sa.argtypes = [C.c_void_p, u64p]
    L.flx_index_copy_sa_u32.argtypes = [C.c_void_p, u32p]
    L.flx_index_copy_bwt.argtypes = [C.c_void_p, C.c_int, u8p]
    L.flx_ctx_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    L.flx_ctx_destroy.argtypes = [C.c_void_p]
    L.flx_index_image_layout.argtypes = [C.c_void_p, u64p]
    L.flx_index_image_upload.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.flx_index_meta_export.argtypes = [C.c_void_p, u8p, u64p]
    L.flx_index_meta_import.argtypes = [u8p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.flx_ctx_create_on_image.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p), u64p, C.POINTER(C.c_void_p)]
    L.flx_ctx_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.flx_search_seeds.argtypes = [C.c_void_p, u8p, C.c_uint64, C.POINTER(Seed), C.c_uint64, C.POINTER(SearchConfig),
                                   C.POINTER(Anchor), u64p, C.POINTER(SeedStats)]
    L.flx_search_groups.argtypes = [C.c_void_p, u8p, C.c_uint64, C.POINTER(Seed), C.c_uint64, C.c_uint64, C.POINTER(HitGroup), u64p]
    L.flx_align_batch.argtypes = [C.c_void_p, u8p, C.c_uint64, u8p, C.c_uint64, C.POINTER(AlignJob), C.c_uint64,
                                  C.POINTER(AlignResult), u32p, u64p]
    L.flx_align_shapes.argtypes = [C.POINTER(AlignJob), C.c_uint64, C.POINTER(AlignShape)]
    L.flx_params_default.argtypes = [C.POINTER(Params)]
    L.flx_align_reads.argtypes = [C.c_void_p, C.POINTER(Params), u8p, u64p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.flx_reads_upload.argtypes = [C.c_void_p, u8p, u64p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.flx_reads_free.argtypes = [C.c_void_p]
    L.flx_align_reads_resident.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.POINTER(C.c_void_p)]
    L.flx_align_reads_with_options.argtypes = [C.c_void_p, C.POINTER(Params), u8p, u64p, C.c_uint64, C.POINTER(OutputOptions),
                                               C.POINTER(C.c_void_p)]
    L.flx_align_reads_resident_with_options.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.POINTER(OutputOptions),
                                                        C.POINTER(C.c_void_p)]
    L.flx_align_reads_with_tags.argtypes = [C.c_void_p, C.POINTER(Params), u8p, u64p, C.c_uint64, C.POINTER(OutputOptions),
                                            C.POINTER(TagOptions), C.POINTER(C.c_void_p)]
    L.flx_align_reads_resident_with_tags.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.POINTER(OutputOptions),
                                                     C.POINTER(TagOptions), C.POINTER(C.c_void_p)]
    L.flx_align_reads_opt.argtypes = [C.c_void_p, C.POINTER(Params), u8p, u64p, C.c_uint64, C.POINTER(RunOptions), C.POINTER(C.c_void_p)]
    L.flx_align_reads_resident_opt.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.POINTER(RunOptions), C.POINTER(C.c_void_p)]
    L.flx_align_reads_split.argtypes = [C.c_void_p, C.POINTER(Params), u8p, u64p, C.c_uint64, C.POINTER(RunOptions), C.POINTER(SplitOptions),
                                        C.POINTER(C.c_void_p)]
    L.flx_align_reads_resident_split.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.POINTER(RunOptions), C.POINTER(SplitOptions),
                                                 C.POINTER(C.c_void_p)]
    L.flx_align_reads_gaps.argtypes = [C.c_void_p, C.POINTER(Params), u8p, u64p, C.c_uint64, C.POINTER(RunOptions), C.POINTER(SplitOptions),
                                       C.POINTER(GapOptions), C.POINTER(C.c_void_p)]
    L.flx_align_reads_resident_gaps.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.POINTER(RunOptions), C.POINTER(SplitOptions),
                                                C.POINTER(GapOptions), C.POINTER(C.c_void_p)]
    L.flx_align_batch_gaps.argtypes = [C.c_void_p, u8p, C.c_uint64, u8p, C.c_uint64, C.POINTER(AlignJob), C.c_uint64,
                                       C.POINTER(AlignResult), u32p, u64p, C.POINTER(MdRef), u8p, u64p, C.POINTER(GapOptions)]
    L.flx_left_align.argtypes = [u8p, C.c_uint64, u8p, C.c_uint64, u32p, C.c_uint64, C.POINTER(LeftAlignJob), C.c_uint64, u32p, u64p,
                                 C.POINTER(CigarRef)]
    L.flx_left_align_batch.argtypes = [C.c_void_p] + L.flx_left_align.argtypes
    L.flx_realign.argtypes = [u8p, C.c_uint64, u8p, C.c_uint64, u32p, C.c_uint64, C.POINTER(RealignJob), C.c_uint64, C.POINTER(RealignOptions), u32p, u64p,
                              C.POINTER(RealignResult)]
    L.flx_realign_batch.argtypes = [C.c_void_p] + L.flx_realign.argtypes
    L.flx_align_batch_realign.argtypes = L.flx_align_batch_gaps.argtypes + [C.POINTER(RealignOptions), C.POINTER(C.c_int32)]
    L.flx_ctx_get_realign_counters.argtypes = [C.c_void_p, C.POINTER(RealignCounters)]
    L.flx_align_reads_realign.argtypes = L.flx_align_reads_gaps.argtypes[:-1] + [C.POINTER(RealignOptions), C.POINTER(C.c_void_p)]
    L.flx_align_reads_resident_realign.argtypes = L.flx_align_reads_resident_gaps.argtypes[:-1] + [C.POINTER(RealignOptions), C.POINTER(C.c_void_p)]
    L.flx_run_copy_scores.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.flx_align_reads_cs.argtypes = L.flx_align_reads_realign.argtypes[:-1] + [C.POINTER(CsOptions), C.POINTER(C.c_void_p)]
    L.flx_align_reads_resident_cs.argtypes = L.flx_align_reads_resident_realign.argtypes[:-1] + [C.POINTER(CsOptions), C.POINTER(C.c_void_p)]
    L.flx_run_num_cs_bytes.restype = C.c_uint64
    L.flx_run_num_cs_bytes.argtypes = [C.c_void_p]
    L.flx_run_copy_cs.argtypes = [C.c_void_p, C.POINTER(MdRef), u8p]
    L.flx_align_batch_cs.argtypes = L.flx_align_batch_realign.argtypes + [C.POINTER(CsOptions), C.POINTER(MdRef), u8p, u64p]
    L.flx_cs.argtypes = [u8p, C.c_uint64, u8p, C.c_uint64, u32p, C.c_uint64, C.POINTER(CsJob), C.c_uint64, C.POINTER(CsOptions), u8p, u64p,
                         C.POINTER(MdRef)]
    L.flx_cs_batch.argtypes = [C.c_void_p] + L.flx_cs.argtypes
    L.flx_coverage_create.argtypes = [C.c_void_p, C.POINTER(CoverageOptions), C.POINTER(C.c_void_p)]
    L.flx_coverage_create_for_lengths.argtypes = [C.c_int, u64p, C.c_uint32, C.POINTER(CoverageOptions), C.POINTER(C.c_void_p)]
    L.flx_coverage_free.restype = None
    L.flx_coverage_free.argtypes = [C.c_void_p]
    L.flx_coverage_add_run.argtypes = [C.c_void_p, C.c_void_p]
    L.flx_coverage_add_records.argtypes = [C.c_void_p, C.POINTER(Record), C.c_uint64, u32p, C.c_uint64]
    L.flx_coverage_absorb.argtypes = [C.c_void_p, C.c_void_p]
    L.flx_coverage_finish.argtypes = [C.c_void_p]
    L.flx_coverage_num_runs.restype = C.c_uint64
    L.flx_coverage_num_runs.argtypes = [C.c_void_p]
    L.flx_coverage_copy_runs.argtypes = [C.c_void_p, C.POINTER(DepthRun), C.c_uint64]
    L.flx_coverage_num_windows.restype = C.c_uint64
    L.flx_coverage_num_windows.argtypes = [C.c_void_p, C.c_uint64]
    L.flx_coverage_copy_windows.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(DepthWindow), C.c_uint64]
    L.flx_coverage_copy_depth.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, u32p]
    L.flx_coverage_geometry.argtypes = [u32p]
    L.flx_coverage_host.argtypes = [u64p, C.c_uint32, C.POINTER(CoverageOptions), C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u32p]
    L.flx_sort_create.argtypes = [C.c_int, C.c_uint32, C.POINTER(SortOptions), C.POINTER(C.c_void_p)]
    L.flx_sort_free.restype = None
    L.flx_sort_free.argtypes = [C.c_void_p]
    L.flx_sort_add_records.argtypes = [C.c_void_p, C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, C.c_uint64, u32p]
    L.flx_sort_add_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, u32p]
    L.flx_sort_finish.argtypes = [C.c_void_p]
    L.flx_sort_num_records.restype = C.c_uint64
    L.flx_sort_num_records.argtypes = [C.c_void_p]
    L.flx_sort_copy.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(SortEntry)]
    L.flx_sort_geometry.argtypes = [u32p]
    L.flx_grid_caps.argtypes = [u32p]
    L.flx_sort_host.argtypes = [C.c_uint32, C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u64p, C.POINTER(SortEntry)]
    L.flx_pileup_create.argtypes = [C.c_void_p, C.POINTER(PileupOptions), C.POINTER(C.c_void_p)]
    L.flx_pileup_create_for_lengths.argtypes = [C.c_int, u64p, C.c_uint32, C.POINTER(PileupOptions), C.POINTER(C.c_void_p)]
    L.flx_pileup_free.restype = None
    L.flx_pileup_free.argtypes = [C.c_void_p]
    L.flx_pileup_add_records.argtypes = [C.c_void_p, C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u8p, u64p, C.c_uint64]
    L.flx_pileup_add_run.argtypes = [C.c_void_p, C.c_void_p, u8p, u64p, C.c_uint64]
    L.flx_pileup_add_run_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.flx_pileup_absorb.argtypes = [C.c_void_p, C.c_void_p]
    L.flx_pileup_finish.argtypes = [C.c_void_p]
    L.flx_pileup_num_sites.restype = C.c_uint64
    L.flx_pileup_num_sites.argtypes = [C.c_void_p]
    L.flx_pileup_copy_sites.argtypes = [C.c_void_p, C.POINTER(PileupSite), C.c_uint64]
    L.flx_pileup_copy_counts.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, u32p]
    L.flx_pileup_host.argtypes = [u64p, C.c_uint32, C.POINTER(PileupOptions), C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u8p, u64p, C.c_uint64, u32p]
    L.flx_pileup_sites_host.argtypes = [u64p, C.c_uint32, C.POINTER(PileupOptions), u32p, C.POINTER(PileupSite), u64p]
    L.flx_sv_create.argtypes = [C.c_void_p, C.POINTER(SvOptions), C.POINTER(C.c_void_p)]
    L.flx_sv_create_for_lengths.argtypes = [C.c_int, u64p, C.c_uint32, C.POINTER(SvOptions), C.POINTER(C.c_void_p)]
    L.flx_sv_free.restype = None
    L.flx_sv_free.argtypes = [C.c_void_p]
    L.flx_sv_add_records.argtypes = [C.c_void_p, C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u64p, C.c_uint64]
    L.flx_sv_add_run.argtypes = [C.c_void_p, C.c_void_p, u64p, C.c_uint64]
    L.flx_sv_absorb.argtypes = [C.c_void_p, C.c_void_p]
    L.flx_sv_finish.argtypes = [C.c_void_p]
    L.flx_sv_num_signatures.restype = C.c_uint64
    L.flx_sv_num_signatures.argtypes = [C.c_void_p]
    L.flx_sv_copy_signatures.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(SvSignature)]
    L.flx_sv_num_clusters.restype = C.c_uint64
    L.flx_sv_num_clusters.argtypes = [C.c_void_p]
    L.flx_sv_copy_clusters.argtypes = [C.c_void_p, C.POINTER(SvCluster), C.c_uint64]
    L.flx_sv_host.argtypes = [u64p, C.c_uint32, C.POINTER(SvOptions), C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u64p, C.c_uint64,
                              C.POINTER(SvSignature), u64p]
    L.flx_sv_clusters_host.argtypes = [C.POINTER(SvOptions), C.POINTER(SvSignature), C.c_uint64, C.POINTER(SvCluster), u64p]
    L.flx_errprof_create.argtypes = [C.c_void_p, C.POINTER(ErrprofOptions), C.POINTER(C.c_void_p)]
    L.flx_errprof_create_for_text.argtypes = [C.c_int, u8p, u64p, C.c_uint32, C.POINTER(ErrprofOptions), C.POINTER(C.c_void_p)]
    L.flx_errprof_free.restype = None
    L.flx_errprof_free.argtypes = [C.c_void_p]
    L.flx_errprof_add_records.argtypes = [C.c_void_p, C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u8p, u64p, C.c_uint64]
    L.flx_errprof_add_run.argtypes = [C.c_void_p, C.c_void_p, u8p, u64p, C.c_uint64]
    L.flx_errprof_add_run_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.flx_errprof_absorb.argtypes = [C.c_void_p, C.c_void_p]
    L.flx_errprof_copy.argtypes = [C.c_void_p, C.POINTER(ErrprofTable)]
    L.flx_errprof_host.argtypes = [u8p, u64p, C.c_uint32, C.POINTER(ErrprofOptions), C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u8p, u64p, C.c_uint64,
                                   C.POINTER(ErrprofTable)]
    L.flx_consensus_create.argtypes = [C.c_void_p, C.POINTER(ConsensusOptions), C.POINTER(C.c_void_p)]
    L.flx_consensus_create_for_text.argtypes = [C.c_int, u8p, u64p, C.c_uint32, C.POINTER(ConsensusOptions), C.POINTER(C.c_void_p)]
    L.flx_consensus_free.restype = None
    L.flx_consensus_free.argtypes = [C.c_void_p]
    L.flx_consensus_add_records.argtypes = [C.c_void_p, C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u8p, u64p, C.c_uint64]
    L.flx_consensus_add_run.argtypes = [C.c_void_p, C.c_void_p, u8p, u64p, C.c_uint64]
    L.flx_consensus_add_run_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.flx_consensus_finish.argtypes = [C.c_void_p]
    L.flx_consensus_num_letters.restype = C.c_uint64
    L.flx_consensus_num_letters.argtypes = [C.c_void_p, C.c_uint32]
    L.flx_consensus_copy_letters.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint64]
    L.flx_consensus_num_changes.restype = C.c_uint64
    L.flx_consensus_num_changes.argtypes = [C.c_void_p]
    L.flx_consensus_copy_changes.argtypes = [C.c_void_p, C.POINTER(ConsensusChange), C.c_uint64]
    L.flx_consensus_num_alleles.restype = C.c_uint64
    L.flx_consensus_num_alleles.argtypes = [C.c_void_p]
    L.flx_consensus_copy_alleles.argtypes = [C.c_void_p, C.POINTER(ConsensusAllele), C.c_uint64]
    L.flx_consensus_geometry.argtypes = [u32p]
    L.flx_consensus_host.argtypes = [u8p, u64p, C.c_uint32, C.POINTER(ConsensusOptions), C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u8p, u64p, C.c_uint64,
                                     u64p, C.c_char_p, u64p, C.POINTER(ConsensusChange), u64p, C.POINTER(ConsensusAllele), u64p]
    L.flx_variants_create.argtypes = [C.c_void_p, C.POINTER(VariantsOptions), C.POINTER(C.c_void_p)]
    L.flx_variants_create_for_text.argtypes = [C.c_int, u8p, u64p, C.c_uint32, C.POINTER(VariantsOptions), C.POINTER(C.c_void_p)]
    L.flx_variants_free.restype = None
    L.flx_variants_free.argtypes = [C.c_void_p]
    L.flx_variants_add_records.argtypes = [C.c_void_p, C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u8p, u64p, C.c_uint64]
    L.flx_variants_add_run.argtypes = [C.c_void_p, C.c_void_p, u8p, u64p, C.c_uint64]
    L.flx_variants_add_run_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.flx_variants_finish.argtypes = [C.c_void_p]
    L.flx_variants_num_rows.restype = C.c_uint64
    L.flx_variants_num_rows.argtypes = [C.c_void_p]
    L.flx_variants_copy_rows.argtypes = [C.c_void_p, C.POINTER(Variant), C.c_uint64]
    L.flx_variants_num_alleles.restype = C.c_uint64
    L.flx_variants_num_alleles.argtypes = [C.c_void_p]
    L.flx_variants_copy_alleles.argtypes = [C.c_void_p, C.POINTER(VariantAllele), C.c_uint64]
    L.flx_variants_geometry.argtypes = [u32p]
    L.flx_variants_genotype.argtypes = [C.POINTER(VariantsOptions), C.c_uint64, C.c_uint64, C.c_uint64, u32p]
    L.flx_variants_host.argtypes = [u8p, u64p, C.c_uint32, C.POINTER(VariantsOptions), C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u8p, u64p, C.c_uint64,
                                    C.POINTER(Variant), u64p, C.POINTER(VariantAllele), u64p]
    L.flx_phase_create.argtypes = [C.c_void_p, C.POINTER(PhaseOptions), C.POINTER(PhaseSite), C.c_uint64, C.POINTER(C.c_void_p)]
    L.flx_phase_create_for_text.argtypes = [C.c_int, u8p, u64p, C.c_uint32, C.POINTER(PhaseOptions), C.POINTER(PhaseSite), C.c_uint64, C.POINTER(C.c_void_p)]
    L.flx_phase_free.restype = None
    L.flx_phase_free.argtypes = [C.c_void_p]
    L.flx_phase_add_records.argtypes = [C.c_void_p, C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u8p, u64p, C.c_uint64]
    L.flx_phase_add_run.argtypes = [C.c_void_p, C.c_void_p, u8p, u64p, C.c_uint64]
    L.flx_phase_add_run_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.flx_phase_finish.argtypes = [C.c_void_p]
    L.flx_phase_num_sites.restype = C.c_uint64
    L.flx_phase_num_sites.argtypes = [C.c_void_p]
    L.flx_phase_copy_results.argtypes = [C.c_void_p, C.POINTER(PhaseResult), C.c_uint64]
    L.flx_phase_num_tags.restype = C.c_uint64
    L.flx_phase_num_tags.argtypes = [C.c_void_p]
    L.flx_phase_copy_tags.argtypes = [C.c_void_p, C.POINTER(PhaseTag), C.c_uint64]
    L.flx_phase_geometry.argtypes = [u32p]
    L.flx_phase_host.argtypes = [u8p, u64p, C.c_uint32, C.POINTER(PhaseOptions), C.POINTER(PhaseSite), C.c_uint64, C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u8p, u64p,
                                 C.c_uint64, C.POINTER(PhaseResult), C.POINTER(PhaseTag), u64p]
    L.flx_svcall_host.argtypes = [u64p, C.c_uint32, C.POINTER(SvcallOptions), C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, C.POINTER(SvCluster), C.c_uint64,
                                  C.POINTER(SvcallRow), u64p]
    L.flx_svcaller_create.argtypes = [C.c_void_p, C.POINTER(SvcallOptions), C.POINTER(C.c_void_p)]
    L.flx_svcaller_create_for_lengths.argtypes = [C.c_int, u64p, C.c_uint32, C.POINTER(SvcallOptions), C.c_uint64, C.POINTER(C.c_void_p)]
    L.flx_svcaller_free.restype = None
    L.flx_svcaller_free.argtypes = [C.c_void_p]
    L.flx_svcaller_add_records.argtypes = [C.c_void_p, C.POINTER(Record), C.c_uint64, u32p, C.c_uint64]
    L.flx_svcaller_add_run.argtypes = [C.c_void_p, C.c_void_p]
    L.flx_svcaller_absorb.argtypes = [C.c_void_p, C.c_void_p]
    L.flx_svcaller_finish.argtypes = [C.c_void_p, C.POINTER(SvCluster), C.c_uint64]
    L.flx_svcaller_num_spans.restype = C.c_uint64
    L.flx_svcaller_num_spans.argtypes = [C.c_void_p]
    L.flx_svcaller_num_rows.restype = C.c_uint64
    L.flx_svcaller_num_rows.argtypes = [C.c_void_p]
    L.flx_svcaller_max_span.restype = C.c_uint32
    L.flx_svcaller_max_span.argtypes = [C.c_void_p]
    L.flx_svcaller_copy_spans.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(SvcallSpan)]
    L.flx_svcaller_copy_rows.argtypes = [C.c_void_p, C.POINTER(SvcallRow), C.c_uint64]
    L.flx_svcaller_geometry.argtypes = [u32p]
    L.flx_paf_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.flx_paf_free.restype = None
    L.flx_paf_free.argtypes = [C.c_void_p]
    L.flx_paf_summarize.argtypes = [C.c_void_p, C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u64p, C.c_uint64, u64p, C.c_uint32, C.POINTER(PafSummary)]
    L.flx_paf_summarize_host.argtypes = [C.POINTER(Record), C.c_uint64, u32p, C.c_uint64, u64p, C.c_uint64, u64p, C.c_uint32, C.POINTER(PafSummary)]
    L.flx_paf_open.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), u64p, C.c_uint32, C.POINTER(PafOptions), C.POINTER(C.c_void_p)]
    L.flx_paf_write.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), u64p, C.POINTER(Record), C.c_uint64, u32p, C.POINTER(PafSummary), C.POINTER(C.c_int32),
                                C.POINTER(MdRef), u8p]
    L.flx_paf_close.argtypes = [C.c_void_p]
    L.flx_cigar_tails.argtypes = [u32p, C.c_uint64, C.POINTER(TailJob), C.c_uint64, C.POINTER(TailResult)]
    L.flx_cigar_tails_batch.argtypes = [C.c_void_p, u32p, C.c_uint64, C.POINTER(TailJob), C.c_uint64, C.POINTER(TailResult)]
    L.flx_choose_partials.argtypes = [C.POINTER(PartialCandidate), C.c_uint64, u32p, C.POINTER(PartialOptions), C.POINTER(C.c_int32)]
    L.flx_partial_mapq.argtypes = [C.POINTER(PartialCandidate), C.c_uint64, u32p, C.POINTER(C.c_int32), u8p]
    L.flx_run_num_md_bytes.restype = C.c_uint64
    L.flx_run_num_md_bytes.argtypes = [C.c_void_p]
    L.flx_run_copy_md.argtypes = [C.c_void_p, C.POINTER(MdRef), u8p]
    L.flx_align_batch_md.argtypes = [C.c_void_p, u8p, C.c_uint64, u8p, C.c_uint64, C.POINTER(AlignJob), C.c_uint64,
                                     C.POINTER(AlignResult), u32p, u64p, C.POINTER(MdRef), u8p, u64p]
    L.flx_sam_write_tagged.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), u8p, u64p, C.POINTER(C.c_char_p), C.POINTER(Record), C.c_uint64, u32p,
                                       C.POINTER(MdRef), u8p]
    L.flx_sam_write_scored.argtypes = L.flx_sam_write_tagged.argtypes + [C.POINTER(C.c_int32)]
    L.flx_sam_write_cs.argtypes = L.flx_sam_write_scored.argtypes + [C.POINTER(MdRef), u8p]
    L.flx_select_records.argtypes = [C.POINTER(Record), C.c_uint64, u32p, C.POINTER(OutputOptions), u8p]
    L.flx_assign_mapq.argtypes = [C.POINTER(Record), C.c_uint64, u32p, u64p, u8p]
    L.flx_run_num_records.restype = C.c_uint64
    L.flx_run_num_records.argtypes = [C.c_void_p]
    L.flx_run_num_cigar_words.restype = C.c_uint64
    L.flx_run_num_cigar_words.argtypes = [C.c_void_p]
    L.flx_run_copy.argtypes = [C.c_void_p, C.POINTER(Record), u32p, u8p]
    L.flx_run_free.argtypes = [C.c_void_p]
    L.flx_ctx_enable_kernel_timing.argtypes = [C.c_void_p, C.c_int]
    L.flx_ctx_reset_kernel_stats.argtypes = [C.c_void_p]
    L.flx_ctx_get_kernel_stats.argtypes = [C.c_void_p, C.POINTER(KernelStat), u32p]
    L.flx_sam_open.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), u64p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.flx_sam_write.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), u8p, u64p, C.POINTER(C.c_char_p), C.POINTER(Record), C.c_uint64, u32p]
    L.flx_sam_close.argtypes = [C.c_void_p]
    L.flx_sam_open_sorted.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_char_p), u64p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.flx_stats_create.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.flx_stats_free.argtypes = [C.c_void_p]
    L.flx_stats_merge.argtypes = [C.c_void_p, C.c_void_p]
    L.flx_stats_num_queries.restype = C.c_uint64
    L.flx_stats_num_queries.argtypes = [C.c_void_p]
    L.flx_stats_format.argtypes = [C.c_void_p, C.c_int, C.c_char_p, u64p]
    L.flx_ctx_set_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.flx_device_count.restype = C.c_int
    L.flx_index_matches_reference.argtypes = [C.c_void_p, u8p, u64p, C.c_uint32]
    L.flx_sam_set_threads.argtypes = [C.c_void_p, C.c_uint32]
    L.flx_sam_set_mapq.argtypes = [C.c_void_p, C.c_int]
    L.flx_sam_set_sa.argtypes = [C.c_void_p, C.c_int]
    L.flx_extend_batch.argtypes = [C.c_void_p, u8p, C.c_uint64, u8p, C.c_uint64, C.POINTER(ExtendJob), C.c_uint64, C.POINTER(ExtendResult)]
    L.flx_ctx_get_path_counters.argtypes = [C.c_void_p, C.POINTER(PathCounters)]
    L.flx_ctx_reset_path_counters.argtypes = [C.c_void_p]
    L.flx_ctx_get_search_counters.argtypes = [C.c_void_p, C.POINTER(SearchCounters)]
    L.flx_climb_anchors.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(ClimbOptions), u8p, u32p, u64p]
    L.flx_ctx_derived_info.argtypes = [C.c_void_p, C.POINTER(DerivedInfo)]
    L.flx_ctx_copy_derived.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
    L.flx_hw_queue_request.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.flx_ctx_lane_overlap.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.flx_sim_genome.argtypes = [C.c_uint64, C.c_uint64, u8p]
    L.flx_sim_genome_repeats.argtypes = [C.c_uint64, C.c_uint64, u8p]
    L.flx_sim_reads.argtypes = [u8p, u64p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_double, C.c_double, C.c_uint64, u8p, C.c_uint64,
                                u64p, u32p, u64p, u8p]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise FloxerError(f"floxer_amd error {rc}: {lib().flx_last_error().decode()}")


def ptr(a, t):
    return a.ctypes.data_as(t)


def as_u8(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint8))
