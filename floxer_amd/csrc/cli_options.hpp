// The command line's options. Ids, defaults and validators of floxer's own options follow include/floxer_cli.hpp:41-70 and
// src/lib/floxer_cli.cpp:173-435; every option has one row in the table of cli_options.cpp, which parses, prints --help and dumps.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

struct Options {
    std::string reference, queries, output, index, logfile;
    bool has_reference = false, has_queries = false, has_output = false;
    bool console_debug_logs = false;
    bool has_query_errors = false, has_error_probability = false;
    uint64_t query_errors = 0;
    double error_probability = NAN;
    uint64_t seed_errors = 2, max_anchors_hard = 500, max_anchors_soft = 50;
    std::string anchor_group_order = "count_first", anchor_choice_strategy = "round_robin";
    uint64_t seed_sampling_step_size = 1;
    bool dont_erase_useless_anchors = false, bottom_up_pex_tree = false, interval_optimization = false;
    double extra_verification_ratio = 0.05;
    bool direct_full_verification = false;
    uint64_t num_anchors_per_task = 3000;
    bool without_cigar = false;
    uint64_t threads = 1, timeout = 0;
    bool has_timeout = false;
    std::string stats, stats_input_hint;
    std::string devices;
    bool drop_duplicate_alignments = false;
    uint64_t max_alignments = 0;                  // 0: no cap
    bool mapping_quality = false;
    bool md_tag = false;
    bool cs_tag = false, cs_tag_long = false;
    bool partial_alignments = false;
    uint64_t partial_min_span = 0, partial_max = 0;   // 0: the library's defaults
    bool partial_extend = false, sa_tag = false;
    uint64_t partial_extend_weight = 0, partial_extend_xdrop = 0, partial_extend_max_errors = 0;   // 0: the library's defaults
    bool split_tails = false;
    uint64_t split_tails_weight = 0, split_tails_xdrop = 0, split_tails_min_rows = 0;               // 0: the library's defaults
    bool left_align_indels = false;
    bool realign_affine = false;
    uint64_t realign_match = 0, realign_mismatch = 0, realign_gap_open = 0, realign_gap_extend = 0, realign_band = 0;   // 0: the library's defaults
    std::string coverage, coverage_summary, coverage_windows;      // output files of the depth track; empty: not written
    uint64_t coverage_window = 0, coverage_min_mapq = 0;
    bool coverage_deletions = false, coverage_secondary = false, coverage_zero = false;
    bool wants_coverage() const { return !coverage.empty() || !coverage_summary.empty() || !coverage_windows.empty(); }
    std::string pileup;                                           // output file of the variant-site table; empty: not written
    uint64_t pileup_min_depth = 0, pileup_min_count = 0, pileup_min_mapq = 0;      // 0: the library's defaults
    double pileup_min_fraction = 0;                               // in (0, 1]; 0: the library's default
    bool pileup_secondary = false;
    std::string sv;                                               // output file of the structural-variant cluster table; empty: not written
    uint64_t sv_min_length = 0, sv_max_distance = 0, sv_min_support = 0, sv_min_mapq = 0;      // 0: the library's defaults
    bool sv_secondary = false;
    std::string error_profile;                                    // output file of the error profile; empty: not written
    uint64_t error_profile_min_mapq = 0;
    bool error_profile_secondary = false;
    bool sort_by_coordinate = false, bam_index = false;           // a coordinate-sorted BAM (flx_sam_open_sorted) and its BAI index
    std::string sort_tmp;                                         // the spill file's directory; empty: the output's
    std::string paf;                                              // the PAF output; empty: not written
    bool paf_cigar = false, paf_unmapped = false, paf_skip_secondary = false;
};

struct CliError { std::string msg; };

// The options of a command line; throws CliError. -h/--help and --version print to stderr and exit(0) from here.
Options parse_cli(int argc, char** argv);

// One "long-id=value" line per row of the option table: flags as 0 or 1, unset texts empty (FLX_CLI_PARSE_ONLY=options)
void dump_options(Options const& o, FILE* to);
