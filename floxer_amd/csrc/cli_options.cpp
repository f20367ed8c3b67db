#include "cli_options.hpp"

#include <unistd.h>

#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "../../include/floxer_amd.h"

namespace {

// One row per option: its ids, the note --help prints, the member of Options it fills and what is checked on the way. A row names one
// member: a flag sets its bool, a text takes the value as it stands, a count goes through parse_u64 and a real through parse_double,
// both followed by the range check where the row has a range. `seen` is set whenever the option occurs; `special` runs in place of
// store() for the few rows that check something else (and call store() themselves).
struct OptDef;
using Special = void (*)(OptDef const&, Options&, std::string const& value);
struct OptDef {
    char short_id;                          // 0: long spelling only
    const char* long_id;
    const char* note;                       // printed by --help; may be null
    bool Options::* flag = nullptr;
    std::string Options::* text = nullptr;
    uint64_t Options::* count = nullptr;
    double Options::* real = nullptr;
    double lo = 0, hi = 0;                  // the inclusive range of a count or real; hi 0: none
    bool Options::* seen = nullptr;
    Special special = nullptr;
    OptDef range(double lo_, double hi_) const { OptDef d = *this; d.lo = lo_; d.hi = hi_; return d; }
    OptDef sets(bool Options::* m) const { OptDef d = *this; d.seen = m; return d; }
    OptDef with(Special s) const { OptDef d = *this; d.special = s; return d; }
};
OptDef flag(char s, const char* l, bool Options::* m, const char* note = nullptr) { OptDef d{s, l, note}; d.flag = m; return d; }
OptDef text(char s, const char* l, std::string Options::* m, const char* note = nullptr) { OptDef d{s, l, note}; d.text = m; return d; }
OptDef count(char s, const char* l, uint64_t Options::* m, const char* note = nullptr) { OptDef d{s, l, note}; d.count = m; return d; }
OptDef real(char s, const char* l, double Options::* m, const char* note = nullptr) { OptDef d{s, l, note}; d.real = m; return d; }

uint64_t parse_u64(std::string const& name, std::string const& v) {
    char* end = nullptr;
    if (v.empty() || v[0] == '-') throw CliError{"Value parse failed for --" + name + ": Argument " + v + " could not be parsed as type unsigned integer."};
    unsigned long long const x = strtoull(v.c_str(), &end, 10);
    if (*end) throw CliError{"Value parse failed for --" + name + ": Argument " + v + " could not be parsed as type unsigned integer."};
    return x;
}
double parse_double(std::string const& name, std::string const& v) {
    char* end = nullptr;
    double const x = strtod(v.c_str(), &end);
    if (v.empty() || *end) throw CliError{"Value parse failed for --" + name + ": Argument " + v + " could not be parsed as type double."};
    return x;
}
void range_check(std::string const& name, double v, double lo, double hi) {
    if (v < lo || v > hi) throw CliError{"Validation failed for option --" + name + ": Value " + std::to_string(v) + " is not in range [" + std::to_string(lo) + "," + std::to_string(hi) + "]."};
}

void store(OptDef const& d, Options& o, std::string const& v) {
    if (d.flag) o.*d.flag = true;
    else if (d.text) o.*d.text = v;
    else if (d.count) { o.*d.count = parse_u64(d.long_id, v); if (d.hi) range_check(d.long_id, (double)(o.*d.count), d.lo, d.hi); }
    else { o.*d.real = parse_double(d.long_id, v); if (d.hi) range_check(d.long_id, o.*d.real, d.lo, d.hi); }
    if (d.seen) o.*d.seen = true;
}
void at_least_one(OptDef const& d, Options& o, std::string const& v) {
    store(d, o, v);
    if (o.*d.count < 1) throw CliError{std::string("Validation failed for option --") + d.long_id + ": must be at least 1."};
}
void one_of(OptDef const& d, Options& o, std::string const& v, std::initializer_list<const char*> allowed) {
    std::string list;
    for (const char* a : allowed) list += std::string(list.empty() ? "" : ",") + a;
    if (std::find(allowed.begin(), allowed.end(), v) == allowed.end()) throw CliError{std::string("Validation failed for option --") + d.long_id + ": Value " + v + " is not one of [" + list + "]."};
    store(d, o, v);
}
void group_order(OptDef const& d, Options& o, std::string const& v) { one_of(d, o, v, {"count_first", "errors_first", "none"}); }
void choice_strategy(OptDef const& d, Options& o, std::string const& v) { one_of(d, o, v, {"round_robin", "full_groups", "first_reported"}); }
void input_hint(OptDef const& d, Options& o, std::string const& v) { one_of(d, o, v, {"real_nanopore", "simulated"}); }
void fraction(OptDef const& d, Options& o, std::string const& v) {
    store(d, o, v);
    if (!(o.*d.real > 0.0 && o.*d.real <= 1.0)) throw CliError{std::string("Validation failed for option --") + d.long_id + ": Value " + v + " is not in (0, 1]."};
}
void directory(OptDef const& d, Options& o, std::string const& v) {
    store(d, o, v);
    if (v.empty()) throw CliError{std::string("Validation failed for option --") + d.long_id + ": the directory's name is empty."};
}

using O = Options;
const OptDef OPTS[] = {
    text('r', "reference", &O::reference).sets(&O::has_reference), text('q', "queries", &O::queries).sets(&O::has_queries),
    text('o', "output", &O::output).sets(&O::has_output), text('i', "index", &O::index), text('l', "logfile", &O::logfile),
    flag('c', "console-debug-logs", &O::console_debug_logs),
    count('e', "query-errors", &O::query_errors).range(0, 4096).sets(&O::has_query_errors),
    real('p', "error-probability", &O::error_probability).range(0.00001, 0.99999).sets(&O::has_error_probability),
    count('s', "seed-errors", &O::seed_errors).range(0, 3),
    count('M', "max-anchors-hard", &O::max_anchors_hard), count('m', "max-anchors-soft", &O::max_anchors_soft),
    text('g', "anchor-group-order", &O::anchor_group_order).with(group_order),
    text('y', "anchor-choice-strategy", &O::anchor_choice_strategy).with(choice_strategy),
    count('C', "seed-sampling-step-size", &O::seed_sampling_step_size), flag('E', "dont-erase-useless-anchors", &O::dont_erase_useless_anchors),
    flag('b', "bottom-up-pex-tree", &O::bottom_up_pex_tree), flag('I', "interval-optimization", &O::interval_optimization),
    real('v', "extra-verification-ratio", &O::extra_verification_ratio), flag('d', "direct-full-verification", &O::direct_full_verification),
    count('u', "num-anchors-per-task", &O::num_anchors_per_task).with(at_least_one), flag('w', "without-cigar", &O::without_cigar),
    count('t', "threads", &O::threads).range(1, 4096), count('x', "timeout", &O::timeout).sets(&O::has_timeout),
    text('S', "stats", &O::stats), text('H', "stats-input-hint", &O::stats_input_hint).with(input_hint),
    // not in the reference: the HIP devices to run on ("0", "0-7", "0,2,4", "all"; default: FLX_DEVICES, else device 0)
    text('G', "devices", &O::devices),
    // not in the reference either: output options (flx_output_options); without them every alignment verification found is written
    flag('D', "drop-duplicate-alignments", &O::drop_duplicate_alignments), count('N', "max-alignments", &O::max_alignments).with(at_least_one),
    // nor this one: MAPQ from the read's distinct loci (flx_output_options.mapq, flx_mapq.hpp) instead of floxer's 255
    flag('Q', "mapping-quality", &O::mapping_quality, "not floxer's: MAPQ from the read's distinct loci within its error budget instead of 255 (0..60; computed before -D / -N drop records)"),
    // nor this one: an MD:Z tag on every mapped record (flx_tag_options.md), built on the GPU next to the CIGARs
    flag(0, "md-tag", &O::md_tag, "not floxer's: MD:Z tag (reference bases at mismatches and deletions) on every mapped record; not with -w"),
    // nor these: minimap2's cs:Z difference string on every mapped record (flx_cs_options), built on the GPU behind the MD strings
    flag(0, "cs-tag", &O::cs_tag, "not floxer's: cs:Z tag, short form (both sequences' letters at mismatches, insertions and deletions) on every mapped record; not with -w or --cs-tag-long"),
    flag(0, "cs-tag-long", &O::cs_tag_long, "not floxer's: cs:Z tag, long form (the matched letters as well) on every mapped record; not with -w or --cs-tag"),
    // nor these: soft-clipped partial alignments, primary + supplementary, for reads that would be unmapped (flx_partial_options, flx_partial.hpp)
    flag(0, "partial-alignments", &O::partial_alignments, "not floxer's: a read without a full alignment gets its largest verified parts as soft-clipped records (primary, then flag 2048); not with -w"),
    count(0, "partial-min-span", &O::partial_min_span, "not floxer's: the fewest query bases of a partial alignment (default 1000)").range(1, 100000),
    count(0, "partial-max", &O::partial_max, "not floxer's: the most partial records of a read (default 4)").range(1, 65535),
    // nor these: the partial records' ends extended to the break (flx_extend_options) and the SA:Z tag that ties a read's records together
    flag(0, "partial-extend", &O::partial_extend, "not floxer's: extend both ends of every partial record to the break (x-drop extension on the GPU); needs --partial-alignments"),
    count(0, "partial-extend-weight", &O::partial_extend_weight, "not floxer's: rows one more error must gain for the extension to go on (default 4); needs --partial-extend").range(1, 65535),
    count(0, "partial-extend-xdrop", &O::partial_extend_xdrop, "not floxer's: the extension stops once its score fell this far below its maximum (default 100); needs --partial-extend").range(1, 1073741824),
    count(0, "partial-extend-max-errors", &O::partial_extend_max_errors, "not floxer's: the most errors of one extension (default 1024, at most 4093); needs --partial-extend").range(1, 4093),
    flag(0, "sa-tag", &O::sa_tag, "not floxer's: SA:Z tag on the records of every read that got supplementary records; needs --partial-alignments"),
    // nor these: reads mapped in full whose primary carries a chimeric tail are split into a clipped primary and supplementaries (flx_split_options)
    flag(0, "split-tails", &O::split_tails, "not floxer's: split a read mapped in full whose primary ends in a chimeric tail (clipped primary + supplementaries); needs --partial-alignments and -N 1, not with -w"),
    count(0, "split-tails-weight", &O::split_tails_weight, "not floxer's: rows one error costs in the tail score (default 4); needs --split-tails").range(1, 65535),
    count(0, "split-tails-xdrop", &O::split_tails_xdrop, "not floxer's: a tail exists once the score fell this far below its maximum (default 100); needs --split-tails").range(1, 1073741824),
    count(0, "split-tails-min-rows", &O::split_tails_min_rows, "not floxer's: the fewest query bases of a tail (default 100); needs --split-tails").range(1, 524287),
    // nor this: every CIGAR's gaps moved to the first copy of a homopolymer or repeat instead of the last (flx_gap_options)
    flag(0, "left-align-indels", &O::left_align_indels, "opt-in, not floxer's: left-align the indels of every CIGAR (on the GPU behind the traceback; MD and split tails follow), as VCF, minimap2 and bwa do; not with -w"),
    // nor these: every traced path realigned under affine gap costs inside a band around it, and its score written as AS:i (flx_realign_options)
    flag(0, "realign-affine", &O::realign_affine, "opt-in, not floxer's: realign every CIGAR under affine gap costs (on the GPU behind the traceback; NM, MD and everything that judges NM follow) and write AS:i; not with -w"),
    count(0, "realign-match", &O::realign_match, "not floxer's: the score of a match (default 2, at most 255); needs --realign-affine").range(1, 255),
    count(0, "realign-mismatch", &O::realign_mismatch, "not floxer's: the cost of a mismatch (default 4, at most 255); needs --realign-affine").range(1, 255),
    count(0, "realign-gap-open", &O::realign_gap_open, "not floxer's: the cost of opening a gap (default 4, at most 255); needs --realign-affine").range(1, 255),
    count(0, "realign-gap-extend", &O::realign_gap_extend, "not floxer's: the cost of every gap column (default 2, at most 255); needs --realign-affine").range(1, 255),
    count(0, "realign-band", &O::realign_band, "not floxer's: the diagonals added on either side of the path's own (default 16, at most 1024); needs --realign-affine").range(1, 1024),
    // nor these: depth of coverage, accumulated on the GPU from every batch's records (flx_coverage, flx_coverage.hpp)
    text(0, "coverage", &O::coverage, "not floxer's: depth of coverage as a bedGraph file (name, start, end, depth; 0-based, half-open; <file.bedgraph>); not with -w"),
    text(0, "coverage-summary", &O::coverage_summary, "not floxer's: one line per reference sequence (name, length, covered, depth_sum, max_depth; <file.tsv>); not with -w"),
    text(0, "coverage-windows", &O::coverage_windows, "not floxer's: depth per window (name, start, end, depth_sum, covered, max_depth; <file.tsv>); needs --coverage-window, not with -w"),
    count(0, "coverage-window", &O::coverage_window, "not floxer's: the window size of --coverage-windows (at least 1)").with(at_least_one),
    flag(0, "coverage-deletions", &O::coverage_deletions, "not floxer's: deleted reference bases count as covered (samtools depth -J); needs one of the coverage outputs"),
    flag(0, "coverage-secondary", &O::coverage_secondary, "not floxer's: secondary records (flag 256) count too; needs one of the coverage outputs"),
    flag(0, "coverage-zero", &O::coverage_zero, "not floxer's: --coverage lists the stretches of depth 0 as well; needs one of the coverage outputs"),
    count(0, "coverage-min-mapq", &O::coverage_min_mapq, "not floxer's: only records of at least this mapping quality count (1..254); needs -Q and one of the coverage outputs").range(1, 254),
    // nor these: per-position allele counts and the table of candidate variant sites, accumulated on the GPU (flx_pileup, flx_pileup.hpp)
    text(0, "pileup", &O::pileup, "not floxer's: candidate variant sites, one line each (name, position, reference letter, depth, A, C, G, T, del, ins; the position is 1-based, as mpileup and VCF have it; <file.tsv>); exact counts, no variant calls; not with -w"),
    count(0, "pileup-min-depth", &O::pileup_min_depth, "not floxer's: a site needs at least this many records over it, deletions included (default 4, a convention fitted to nothing); needs --pileup").range(1, 4294967295.0),
    count(0, "pileup-min-count", &O::pileup_min_count, "not floxer's: a site needs at least this many records for its largest of A, C, G, T, del, ins (default 2, a convention fitted to nothing); needs --pileup").range(1, 4294967295.0),
    real(0, "pileup-min-fraction", &O::pileup_min_fraction, "not floxer's: and that count must be at least this fraction of the records over it, in (0, 1] (default 0.2, a convention fitted to nothing); needs --pileup").with(fraction),
    flag(0, "pileup-secondary", &O::pileup_secondary, "not floxer's: secondary records (flag 256) count too; needs --pileup"),
    count(0, "pileup-min-mapq", &O::pileup_min_mapq, "not floxer's: only records of at least this mapping quality count (1..254); needs -Q and --pileup").range(1, 254),
    // nor these: structural-variant signatures (long deletions, long insertions, split junctions), sorted and clustered on the GPU (flx_sv, flx_sv.hpp)
    text(0, "sv-signatures", &O::sv, "not floxer's: clusters of structural-variant signatures, one line each (type DEL / INS / BND, name a, first and last position a, side a, name b, smallest, median and largest q, side b, support; positions are 1-based; q is a length for DEL and INS and a 1-based position for BND; sides are L / R for BND and . otherwise; <file.tsv>); exact counts of records, no variant calls: use -D -N 1; not with -w"),
    count(0, "sv-min-length", &O::sv_min_length, "not floxer's: a D or I word is a signature from this length on (default 50, a convention fitted to nothing); needs --sv-signatures").range(1, 268435455.0),
    count(0, "sv-max-distance", &O::sv_max_distance, "not floxer's: neighbours of one cluster lie at most this far apart, in position and in q (default 100, a convention fitted to nothing); needs --sv-signatures").range(1, 4294967295.0),
    count(0, "sv-min-support", &O::sv_min_support, "not floxer's: a cluster is written from this many records on (default 2, a convention fitted to nothing); needs --sv-signatures").range(1, 4294967295.0),
    flag(0, "sv-secondary", &O::sv_secondary, "not floxer's: secondary records (flag 256) count too, for DEL and INS (they never form junctions); needs --sv-signatures"),
    count(0, "sv-min-mapq", &O::sv_min_mapq, "not floxer's: only records of at least this mapping quality count (1..254); needs -Q and --sv-signatures").range(1, 254),
    // nor these: the error profile of the alignments, summed on the GPU (flx_errprof, flx_errprof.hpp)
    text(0, "error-profile", &O::error_profile, "not floxer's: how the reads err, one counter per line (section, keys, count: which letter is read as which, insertion and deletion lengths and their homopolymer context, errors by position in the read, identities, error-free stretches) and summary lines with the error rate in ppm, the figure to hold against --error-probability; <file.tsv>; exact counts of records: use -D -N 1; not with -w"),
    flag(0, "error-profile-secondary", &O::error_profile_secondary, "not floxer's: secondary records (flag 256) count too; needs --error-profile"),
    count(0, "error-profile-min-mapq", &O::error_profile_min_mapq, "not floxer's: only records of at least this mapping quality count (1..254); needs -Q and --error-profile").range(1, 254),
    // nor these: the output in coordinate order, its keys sorted on the GPU (flx_sort, flx_sort.hpp), and its BAI index
    flag(0, "sort-by-coordinate", &O::sort_by_coordinate, "not floxer's: write the records in coordinate order (reference, position, strand; unmapped last) with @HD SO:coordinate; needs a .bam output"),
    flag(0, "bam-index", &O::bam_index, "not floxer's: write the BAI index <output>.bai as well; needs --sort-by-coordinate"),
    text(0, "sort-tmp", &O::sort_tmp, "not floxer's: the directory of the sort's spill file (default: the output's directory); needs --sort-by-coordinate").with(directory),
    // nor these: the mappings as PAF lines, their per-record numbers reduced on the GPU from the CIGARs (flx_paf, flx_paf.hpp)
    text(0, "paf", &O::paf, "not floxer's: one PAF line per mapped record (tp, NM, de and, with --realign-affine, -Q, --cs-tag or --cs-tag-long, AS, the MAPQ column and cs; <file.paf>); with it -o/--output may be left out; not with -w"),
    flag(0, "paf-cigar", &O::paf_cigar, "not floxer's: a cg:Z tag with the record's CIGAR (= and X kept, as minimap2 --eqx writes it); needs --paf"),
    flag(0, "paf-unmapped", &O::paf_unmapped, "not floxer's: a line for every unmapped read as well (minimap2's --paf-no-hit form); needs --paf"),
    flag(0, "paf-skip-secondary", &O::paf_skip_secondary, "not floxer's: secondary records (flag 256) produce no PAF line; needs --paf"),
};

void print_help() {
    fprintf(stderr, "floxer (MI355X-native path) - usage: ./floxer --reference hg38.fasta --queries reads.fastq --error-probability 0.07 --output mapped_reads.bam\n");
    for (auto const& d : OPTS) {
        if (d.short_id) fprintf(stderr, "  -%c, ", d.short_id);
        else fprintf(stderr, "      ");
        fprintf(stderr, "--%s%s%s%s\n", d.long_id, d.flag ? "" : " <value>", d.note ? "    " : "", d.note ? d.note : "");
    }
}

bool ends_with(std::string const& s, std::string const& suf) { return s.size() >= suf.size() && s.compare(s.size() - suf.size(), suf.size(), suf) == 0; }
bool has_ext(std::string const& path, std::vector<std::string> const& exts, bool allow_gz) {
    for (auto const& e : exts) {
        if (ends_with(path, "." + e)) return true;
        if (allow_gz && ends_with(path, "." + e + ".gz")) return true;
    }
    return false;
}
// (by permission, not by opening: opening and closing a FIFO would break the pipe under its writer before the reader gets to it)
bool file_readable(std::string const& p) { return access(p.c_str(), R_OK) == 0; }

// What the rows cannot check one by one. The messages are hand-worded, and the order decides which one a doubly wrong command line gets.
void cross_check(Options const& o) {
    // ---- the required options and their files
    if (!o.has_reference) throw CliError{"Option -r/--reference is required but not set."};
    if (!o.has_queries) throw CliError{"Option -q/--queries is required but not set."};
    if (!o.has_output && o.paf.empty()) throw CliError{"Option -o/--output is required but not set."};      // (a PAF output alone is an output)
    if (!has_ext(o.reference, {"fa", "fasta", "fna", "ffn", "fas", "faa", "mpfa", "frn"}, true)) throw CliError{"Validation failed for option -r/--reference: Expected one of the following valid extensions: [fa,fasta,fna,ffn,fas,faa,mpfa,frn](.gz)."};
    if (!file_readable(o.reference)) throw CliError{"Validation failed for option -r/--reference: The file " + o.reference + " does not exist!"};
    if (!has_ext(o.queries, {"fq", "fastq"}, true)) throw CliError{"Validation failed for option -q/--queries: Expected one of the following valid extensions: [fq,fastq](.gz)."};
    if (!file_readable(o.queries)) throw CliError{"Validation failed for option -q/--queries: The file " + o.queries + " does not exist!"};
    if (o.has_output && !has_ext(o.output, {"bam", "sam"}, false)) throw CliError{"Validation failed for option -o/--output: Expected one of the following valid extensions: [bam,sam]."};
    // ---- floxer's own cross validation, floxer_cli.cpp:173-204
    if (!o.has_query_errors && !o.has_error_probability) throw CliError{"Either a fixed number of errors in the query or an error probability must be given."};
    if (!o.has_error_probability && o.query_errors < o.seed_errors)
        throw CliError{"The number of errors per query (" + std::to_string(o.query_errors) + ") must be greater or equal than the number of errors in the PEX tree leaves (" + std::to_string(o.seed_errors) + ")."};
    if (o.max_anchors_hard < o.max_anchors_soft)
        throw CliError{"The hard maximum number of anchors (" + std::to_string(o.max_anchors_hard) + ") should not be smaller than the soft maximum number of anchors (" + std::to_string(o.max_anchors_soft) + ")."};
    if (o.seed_sampling_step_size == 0) throw CliError{"Validation failed for option --seed-sampling-step-size: must be at least 1."};
    // ---- MD and cs tags
    if (o.md_tag && o.without_cigar) throw CliError{"The option --md-tag needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (o.cs_tag && o.cs_tag_long) throw CliError{"The options --cs-tag and --cs-tag-long select one form of the same tag and cannot be combined."};
    if ((o.cs_tag || o.cs_tag_long) && o.without_cigar) throw CliError{"The options --cs-tag and --cs-tag-long need the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    // ---- partial alignments, their extension and the SA tag
    if (o.partial_alignments && o.without_cigar) throw CliError{"The option --partial-alignments needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (!o.partial_alignments && (o.partial_min_span || o.partial_max)) throw CliError{"The options --partial-min-span and --partial-max need --partial-alignments."};
    if (o.partial_extend && !o.partial_alignments) throw CliError{"The option --partial-extend needs --partial-alignments."};
    if (!o.partial_extend && (o.partial_extend_weight || o.partial_extend_xdrop || o.partial_extend_max_errors))
        throw CliError{"The options --partial-extend-weight, --partial-extend-xdrop and --partial-extend-max-errors need --partial-extend."};
    if (o.sa_tag && !o.partial_alignments) throw CliError{"The option --sa-tag needs --partial-alignments."};
    // ---- split tails
    if (o.split_tails && !o.partial_alignments) throw CliError{"The option --split-tails needs --partial-alignments."};
    if (o.split_tails && o.max_alignments != 1) throw CliError{"The option --split-tails judges the primary alignment and needs -N/--max-alignments 1."};
    if (o.split_tails && o.without_cigar) throw CliError{"The option --split-tails needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (!o.split_tails && (o.split_tails_weight || o.split_tails_xdrop || o.split_tails_min_rows))
        throw CliError{"The options --split-tails-weight, --split-tails-xdrop and --split-tails-min-rows need --split-tails."};
    // ---- left-aligned indels and the affine realignment
    if (o.left_align_indels && o.without_cigar) throw CliError{"The option --left-align-indels needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (o.realign_affine && o.without_cigar) throw CliError{"The option --realign-affine needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (!o.realign_affine && (o.realign_match || o.realign_mismatch || o.realign_gap_open || o.realign_gap_extend || o.realign_band))
        throw CliError{"The options --realign-match, --realign-mismatch, --realign-gap-open, --realign-gap-extend and --realign-band need --realign-affine."};
    if (o.realign_affine) {
        // (the library's rule, stated here so that it is refused with the other options and before the index is read)
        uint64_t const a = o.realign_match ? o.realign_match : 2, b = o.realign_mismatch ? o.realign_mismatch : 4, go = o.realign_gap_open ? o.realign_gap_open : 4,
                       ge = o.realign_gap_extend ? o.realign_gap_extend : 2;
        if (std::max(a + b, go + ge + a) > 8 * std::min(a + b, go + ge))
            throw CliError{"The realign scores are too far apart: max(match + mismatch, gap-open + gap-extend + match) must not exceed 8 times min(match + mismatch, gap-open + gap-extend)."};
    }
    // ---- coverage
    if (o.wants_coverage() && o.without_cigar) throw CliError{"The options --coverage, --coverage-summary and --coverage-windows need the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (!o.wants_coverage() && (o.coverage_deletions || o.coverage_secondary || o.coverage_zero || o.coverage_min_mapq || o.coverage_window))
        throw CliError{"The options --coverage-deletions, --coverage-secondary, --coverage-zero, --coverage-min-mapq and --coverage-window need one of --coverage, --coverage-summary and --coverage-windows."};
    if (o.coverage_min_mapq && !o.mapping_quality) throw CliError{"The option --coverage-min-mapq judges the records' mapping quality and needs -Q/--mapping-quality."};
    if (o.coverage_windows.empty() != (o.coverage_window == 0)) throw CliError{"The options --coverage-windows and --coverage-window need each other."};
    if (!o.coverage.empty() && !has_ext(o.coverage, {"bedgraph"}, false)) throw CliError{"Validation failed for option --coverage: Expected one of the following valid extensions: [bedgraph]."};
    if (!o.coverage_summary.empty() && !has_ext(o.coverage_summary, {"tsv"}, false)) throw CliError{"Validation failed for option --coverage-summary: Expected one of the following valid extensions: [tsv]."};
    if (!o.coverage_windows.empty() && !has_ext(o.coverage_windows, {"tsv"}, false)) throw CliError{"Validation failed for option --coverage-windows: Expected one of the following valid extensions: [tsv]."};
    // ---- pileup
    if (!o.pileup.empty() && o.without_cigar) throw CliError{"The option --pileup needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (o.pileup.empty() && (o.pileup_min_depth || o.pileup_min_count || o.pileup_min_fraction || o.pileup_secondary || o.pileup_min_mapq))
        throw CliError{"The options --pileup-min-depth, --pileup-min-count, --pileup-min-fraction, --pileup-secondary and --pileup-min-mapq need --pileup."};
    if (o.pileup_min_mapq && !o.mapping_quality) throw CliError{"The option --pileup-min-mapq judges the records' mapping quality and needs -Q/--mapping-quality."};
    if (!o.pileup.empty() && !has_ext(o.pileup, {"tsv"}, false)) throw CliError{"Validation failed for option --pileup: Expected one of the following valid extensions: [tsv]."};
    // ---- structural-variant signatures
    if (!o.sv.empty() && o.without_cigar) throw CliError{"The option --sv-signatures needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (o.sv.empty() && (o.sv_min_length || o.sv_max_distance || o.sv_min_support || o.sv_secondary || o.sv_min_mapq))
        throw CliError{"The options --sv-min-length, --sv-max-distance, --sv-min-support, --sv-secondary and --sv-min-mapq need --sv-signatures."};
    if (o.sv_min_mapq && !o.mapping_quality) throw CliError{"The option --sv-min-mapq judges the records' mapping quality and needs -Q/--mapping-quality."};
    if (!o.sv.empty() && !has_ext(o.sv, {"tsv"}, false)) throw CliError{"Validation failed for option --sv-signatures: Expected one of the following valid extensions: [tsv]."};
    // ---- error profile
    if (!o.error_profile.empty() && o.without_cigar) throw CliError{"The option --error-profile needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (o.error_profile.empty() && (o.error_profile_secondary || o.error_profile_min_mapq)) throw CliError{"The options --error-profile-secondary and --error-profile-min-mapq need --error-profile."};
    if (o.error_profile_min_mapq && !o.mapping_quality) throw CliError{"The option --error-profile-min-mapq judges the records' mapping quality and needs -Q/--mapping-quality."};
    if (!o.error_profile.empty() && !has_ext(o.error_profile, {"tsv"}, false)) throw CliError{"Validation failed for option --error-profile: Expected one of the following valid extensions: [tsv]."};
    // ---- sorted BAM
    if (!o.sort_by_coordinate && (o.bam_index || !o.sort_tmp.empty())) throw CliError{"The options --bam-index and --sort-tmp need --sort-by-coordinate."};
    if (o.sort_by_coordinate && !has_ext(o.output, {"bam"}, false)) throw CliError{"The option --sort-by-coordinate writes BAM and needs an -o/--output that ends in .bam."};
    // ---- PAF
    if (!o.paf.empty() && o.without_cigar) throw CliError{"The option --paf needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (o.paf.empty() && (o.paf_cigar || o.paf_unmapped || o.paf_skip_secondary)) throw CliError{"The options --paf-cigar, --paf-unmapped and --paf-skip-secondary need --paf."};
    if (!o.paf.empty() && !has_ext(o.paf, {"paf"}, false)) throw CliError{"Validation failed for option --paf: Expected one of the following valid extensions: [paf]."};
}

}  // namespace

Options parse_cli(int argc, char** argv) {
    Options o;
    for (int a = 1; a < argc; ++a) {
        std::string arg = argv[a];
        const OptDef* def = nullptr;
        std::string value;
        bool has_inline = false;
        if (arg.size() > 2 && arg[0] == '-' && arg[1] == '-') {
            std::string name = arg.substr(2);
            size_t const eq = name.find('=');
            if (eq != std::string::npos) { value = name.substr(eq + 1); name = name.substr(0, eq); has_inline = true; }
            for (auto const& d : OPTS) if (name == d.long_id) def = &d;
        } else if (arg.size() == 2 && arg[0] == '-') {
            for (auto const& d : OPTS) if (d.short_id && arg[1] == d.short_id) def = &d;
        }
        if (arg == "-h" || arg == "--help") { print_help(); exit(0); }
        if (arg == "--version") { fprintf(stderr, "%s\n", flx_version()); exit(0); }
        if (!def) throw CliError{"Unknown option " + arg + ". In case this is meant to be a non-option/argument/parameter, please specify the start of non-options with '--'."};
        if (!def->flag && !has_inline) {
            if (a + 1 >= argc) throw CliError{std::string("Missing value for option --") + def->long_id};
            value = argv[++a];
        }
        (def->special ? def->special : store)(*def, o, value);
    }
    cross_check(o);
    return o;
}

void dump_options(Options const& o, FILE* to) {
    for (auto const& d : OPTS) {
        if (d.flag) fprintf(to, "%s=%d\n", d.long_id, o.*d.flag ? 1 : 0);
        else if (d.text) fprintf(to, "%s=%s\n", d.long_id, (o.*d.text).c_str());
        else if (d.count) fprintf(to, "%s=%llu\n", d.long_id, (unsigned long long)(o.*d.count));
        else fprintf(to, "%s=%g\n", d.long_id, std::isnan(o.*d.real) ? 0.0 : o.*d.real);
    }
}
