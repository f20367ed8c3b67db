// floxer-compatible command line over libfloxer_amd (drop-in for the process boundary):
//   ./floxer --reference ref.fa --queries reads.fq --error-probability 0.08 --output out.bam   (README.md:35)
// Options, short ids, defaults and validators follow include/floxer_cli.hpp:41-70 and src/lib/floxer_cli.cpp:173-435;
// main() follows src/main/floxer.cpp:35-195. Diagnostics go to stderr only, stdout stays empty
// (floxer_whole_program_via_cli_test.cpp:125-126); exit code 0 on success, 255 (-1) on any error.
#include <zlib.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <future>
#include <memory>
#include <string>
#include <sys/stat.h>
#include <fcntl.h>
#include <unistd.h>
#include <cerrno>
#include <thread>
#include <vector>

#include "../../include/floxer_amd.h"

namespace {

bool g_debug = false;
FILE* g_logfile = nullptr;

void log_line(const char* level, const char* fmt, ...) {
    char buf[4096];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    bool const is_debug = strcmp(level, "debug") == 0;
    if (!is_debug || g_debug) fprintf(stderr, "[floxer] [%s] %s\n", level, buf);
    if (g_logfile) { fprintf(g_logfile, "[%s] %s\n", level, buf); fflush(g_logfile); }
}

struct Options {
    std::string reference, queries, output, index, logfile;
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
    uint64_t pileup_min_depth = 0, pileup_min_count = 0, pileup_min_permille = 0, pileup_min_mapq = 0;      // 0: the library's defaults
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

struct OptDef { char short_id; const char* long_id; bool flag; const char* note = nullptr; };   // short_id 0: long spelling only; note: printed by --help
const OptDef OPTS[] = {
    {'r', "reference", false}, {'q', "queries", false}, {'o', "output", false}, {'i', "index", false}, {'l', "logfile", false},
    {'c', "console-debug-logs", true}, {'e', "query-errors", false}, {'p', "error-probability", false}, {'s', "seed-errors", false},
    {'M', "max-anchors-hard", false}, {'m', "max-anchors-soft", false}, {'g', "anchor-group-order", false},
    {'y', "anchor-choice-strategy", false}, {'C', "seed-sampling-step-size", false}, {'E', "dont-erase-useless-anchors", true},
    {'b', "bottom-up-pex-tree", true}, {'I', "interval-optimization", true}, {'v', "extra-verification-ratio", false},
    {'d', "direct-full-verification", true}, {'u', "num-anchors-per-task", false}, {'w', "without-cigar", true}, {'t', "threads", false},
    {'x', "timeout", false}, {'S', "stats", false}, {'H', "stats-input-hint", false},
    // not in the reference: the HIP devices to run on ("0", "0-7", "0,2,4", "all"; default: FLX_DEVICES, else device 0)
    {'G', "devices", false},
    // not in the reference either: output options (flx_output_options); without them every alignment verification found is written
    {'D', "drop-duplicate-alignments", true}, {'N', "max-alignments", false},
    // nor this one: MAPQ from the read's distinct loci (flx_output_options.mapq, flx_mapq.hpp) instead of floxer's 255
    {'Q', "mapping-quality", true, "not floxer's: MAPQ from the read's distinct loci within its error budget instead of 255 (0..60; computed before -D / -N drop records)"},
    // nor this one: an MD:Z tag on every mapped record (flx_tag_options.md), built on the GPU next to the CIGARs
    {0, "md-tag", true, "not floxer's: MD:Z tag (reference bases at mismatches and deletions) on every mapped record; not with -w"},
    // nor these: minimap2's cs:Z difference string on every mapped record (flx_cs_options), built on the GPU behind the MD strings
    {0, "cs-tag", true, "not floxer's: cs:Z tag, short form (both sequences' letters at mismatches, insertions and deletions) on every mapped record; not with -w or --cs-tag-long"},
    {0, "cs-tag-long", true, "not floxer's: cs:Z tag, long form (the matched letters as well) on every mapped record; not with -w or --cs-tag"},
    // nor these: soft-clipped partial alignments, primary + supplementary, for reads that would be unmapped (flx_partial_options, flx_partial.hpp)
    {0, "partial-alignments", true, "not floxer's: a read without a full alignment gets its largest verified parts as soft-clipped records (primary, then flag 2048); not with -w"},
    {0, "partial-min-span", false, "not floxer's: the fewest query bases of a partial alignment (default 1000)"},
    {0, "partial-max", false, "not floxer's: the most partial records of a read (default 4)"},
    // nor these: the partial records' ends extended to the break (flx_extend_options) and the SA:Z tag that ties a read's records together
    {0, "partial-extend", true, "not floxer's: extend both ends of every partial record to the break (x-drop extension on the GPU); needs --partial-alignments"},
    {0, "partial-extend-weight", false, "not floxer's: rows one more error must gain for the extension to go on (default 4); needs --partial-extend"},
    {0, "partial-extend-xdrop", false, "not floxer's: the extension stops once its score fell this far below its maximum (default 100); needs --partial-extend"},
    {0, "partial-extend-max-errors", false, "not floxer's: the most errors of one extension (default 1024, at most 4093); needs --partial-extend"},
    {0, "sa-tag", true, "not floxer's: SA:Z tag on the records of every read that got supplementary records; needs --partial-alignments"},
    // nor these: reads mapped in full whose primary carries a chimeric tail are split into a clipped primary and supplementaries (flx_split_options)
    {0, "split-tails", true, "not floxer's: split a read mapped in full whose primary ends in a chimeric tail (clipped primary + supplementaries); needs --partial-alignments and -N 1, not with -w"},
    {0, "split-tails-weight", false, "not floxer's: rows one error costs in the tail score (default 4); needs --split-tails"},
    {0, "split-tails-xdrop", false, "not floxer's: a tail exists once the score fell this far below its maximum (default 100); needs --split-tails"},
    {0, "split-tails-min-rows", false, "not floxer's: the fewest query bases of a tail (default 100); needs --split-tails"},
    // nor this: every CIGAR's gaps moved to the first copy of a homopolymer or repeat instead of the last (flx_gap_options)
    {0, "left-align-indels", true, "opt-in, not floxer's: left-align the indels of every CIGAR (on the GPU behind the traceback; MD and split tails follow), as VCF, minimap2 and bwa do; not with -w"},
    // nor these: every traced path realigned under affine gap costs inside a band around it, and its score written as AS:i (flx_realign_options)
    {0, "realign-affine", true, "opt-in, not floxer's: realign every CIGAR under affine gap costs (on the GPU behind the traceback; NM, MD and everything that judges NM follow) and write AS:i; not with -w"},
    {0, "realign-match", false, "not floxer's: the score of a match (default 2, at most 255); needs --realign-affine"},
    {0, "realign-mismatch", false, "not floxer's: the cost of a mismatch (default 4, at most 255); needs --realign-affine"},
    {0, "realign-gap-open", false, "not floxer's: the cost of opening a gap (default 4, at most 255); needs --realign-affine"},
    {0, "realign-gap-extend", false, "not floxer's: the cost of every gap column (default 2, at most 255); needs --realign-affine"},
    {0, "realign-band", false, "not floxer's: the diagonals added on either side of the path's own (default 16, at most 1024); needs --realign-affine"},
    // nor these: depth of coverage, accumulated on the GPU from every batch's records (flx_coverage, flx_coverage.hpp)
    {0, "coverage", false, "not floxer's: depth of coverage as a bedGraph file (name, start, end, depth; 0-based, half-open; <file.bedgraph>); not with -w"},
    {0, "coverage-summary", false, "not floxer's: one line per reference sequence (name, length, covered, depth_sum, max_depth; <file.tsv>); not with -w"},
    {0, "coverage-windows", false, "not floxer's: depth per window (name, start, end, depth_sum, covered, max_depth; <file.tsv>); needs --coverage-window, not with -w"},
    {0, "coverage-window", false, "not floxer's: the window size of --coverage-windows (at least 1)"},
    {0, "coverage-deletions", true, "not floxer's: deleted reference bases count as covered (samtools depth -J); needs one of the coverage outputs"},
    {0, "coverage-secondary", true, "not floxer's: secondary records (flag 256) count too; needs one of the coverage outputs"},
    {0, "coverage-zero", true, "not floxer's: --coverage lists the stretches of depth 0 as well; needs one of the coverage outputs"},
    {0, "coverage-min-mapq", false, "not floxer's: only records of at least this mapping quality count (1..254); needs -Q and one of the coverage outputs"},
    // nor these: per-position allele counts and the table of candidate variant sites, accumulated on the GPU (flx_pileup, flx_pileup.hpp)
    {0, "pileup", false, "not floxer's: candidate variant sites, one line each (name, position, reference letter, depth, A, C, G, T, del, ins; the position is 1-based, as mpileup and VCF have it; <file.tsv>); exact counts, no variant calls; not with -w"},
    {0, "pileup-min-depth", false, "not floxer's: a site needs at least this many records over it, deletions included (default 4, a convention fitted to nothing); needs --pileup"},
    {0, "pileup-min-count", false, "not floxer's: a site needs at least this many records for its largest of A, C, G, T, del, ins (default 2, a convention fitted to nothing); needs --pileup"},
    {0, "pileup-min-fraction", false, "not floxer's: and that count must be at least this fraction of the records over it, in (0, 1] (default 0.2, a convention fitted to nothing); needs --pileup"},
    {0, "pileup-secondary", true, "not floxer's: secondary records (flag 256) count too; needs --pileup"},
    {0, "pileup-min-mapq", false, "not floxer's: only records of at least this mapping quality count (1..254); needs -Q and --pileup"},
    // nor these: structural-variant signatures (long deletions, long insertions, split junctions), sorted and clustered on the GPU (flx_sv, flx_sv.hpp)
    {0, "sv-signatures", false, "not floxer's: clusters of structural-variant signatures, one line each (type DEL / INS / BND, name a, first and last position a, side a, name b, smallest, median and largest q, side b, support; positions are 1-based; q is a length for DEL and INS and a 1-based position for BND; sides are L / R for BND and . otherwise; <file.tsv>); exact counts of records, no variant calls: use -D -N 1; not with -w"},
    {0, "sv-min-length", false, "not floxer's: a D or I word is a signature from this length on (default 50, a convention fitted to nothing); needs --sv-signatures"},
    {0, "sv-max-distance", false, "not floxer's: neighbours of one cluster lie at most this far apart, in position and in q (default 100, a convention fitted to nothing); needs --sv-signatures"},
    {0, "sv-min-support", false, "not floxer's: a cluster is written from this many records on (default 2, a convention fitted to nothing); needs --sv-signatures"},
    {0, "sv-secondary", true, "not floxer's: secondary records (flag 256) count too, for DEL and INS (they never form junctions); needs --sv-signatures"},
    {0, "sv-min-mapq", false, "not floxer's: only records of at least this mapping quality count (1..254); needs -Q and --sv-signatures"},
    // nor these: the error profile of the alignments, summed on the GPU (flx_errprof, flx_errprof.hpp)
    {0, "error-profile", false, "not floxer's: how the reads err, one counter per line (section, keys, count: which letter is read as which, insertion and deletion lengths and their homopolymer context, errors by position in the read, identities, error-free stretches) and summary lines with the error rate in ppm, the figure to hold against --error-probability; <file.tsv>; exact counts of records: use -D -N 1; not with -w"},
    {0, "error-profile-secondary", true, "not floxer's: secondary records (flag 256) count too; needs --error-profile"},
    {0, "error-profile-min-mapq", false, "not floxer's: only records of at least this mapping quality count (1..254); needs -Q and --error-profile"},
    // nor these: the output in coordinate order, its keys sorted on the GPU (flx_sort, flx_sort.hpp), and its BAI index
    {0, "sort-by-coordinate", true, "not floxer's: write the records in coordinate order (reference, position, strand; unmapped last) with @HD SO:coordinate; needs a .bam output"},
    {0, "bam-index", true, "not floxer's: write the BAI index <output>.bai as well; needs --sort-by-coordinate"},
    {0, "sort-tmp", false, "not floxer's: the directory of the sort's spill file (default: the output's directory); needs --sort-by-coordinate"},
    // nor these: the mappings as PAF lines, their per-record numbers reduced on the GPU from the CIGARs (flx_paf, flx_paf.hpp)
    {0, "paf", false, "not floxer's: one PAF line per mapped record (tp, NM, de and, with --realign-affine, -Q, --cs-tag or --cs-tag-long, AS, the MAPQ column and cs; <file.paf>); with it -o/--output may be left out; not with -w"},
    {0, "paf-cigar", true, "not floxer's: a cg:Z tag with the record's CIGAR (= and X kept, as minimap2 --eqx writes it); needs --paf"},
    {0, "paf-unmapped", true, "not floxer's: a line for every unmapped read as well (minimap2's --paf-no-hit form); needs --paf"},
    {0, "paf-skip-secondary", true, "not floxer's: secondary records (flag 256) produce no PAF line; needs --paf"},
};

struct CliError { std::string msg; };

bool ends_with(std::string const& s, std::string const& suf) { return s.size() >= suf.size() && s.compare(s.size() - suf.size(), suf.size(), suf) == 0; }
bool has_ext(std::string const& path, std::vector<std::string> const& exts, bool allow_gz) {
    for (auto const& e : exts) {
        if (ends_with(path, "." + e)) return true;
        if (allow_gz && ends_with(path, "." + e + ".gz")) return true;
    }
    return false;
}
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
// (by permission, not by opening: opening and closing a FIFO would break the pipe under its writer before the reader gets to it)
bool file_readable(std::string const& p) { return access(p.c_str(), R_OK) == 0; }

Options parse_cli(int argc, char** argv) {
    Options o;
    bool seen_ref = false, seen_q = false, seen_out = false;
    for (int a = 1; a < argc; ++a) {
        std::string arg = argv[a];
        const OptDef* def = nullptr;
        std::string inline_value;
        bool has_inline = false;
        if (arg.size() > 2 && arg[0] == '-' && arg[1] == '-') {
            std::string name = arg.substr(2);
            size_t const eq = name.find('=');
            if (eq != std::string::npos) { inline_value = name.substr(eq + 1); name = name.substr(0, eq); has_inline = true; }
            for (auto const& d : OPTS) if (name == d.long_id) def = &d;
        } else if (arg.size() == 2 && arg[0] == '-') {
            for (auto const& d : OPTS) if (d.short_id && arg[1] == d.short_id) def = &d;
        }
        if (arg == "-h" || arg == "--help") {
            fprintf(stderr, "floxer (MI355X-native path) - usage: ./floxer --reference hg38.fasta --queries reads.fastq --error-probability 0.07 --output mapped_reads.bam\n");
            for (auto const& d : OPTS) {
                if (d.short_id) fprintf(stderr, "  -%c, ", d.short_id);
                else fprintf(stderr, "      ");
                fprintf(stderr, "--%s%s%s%s\n", d.long_id, d.flag ? "" : " <value>", d.note ? "    " : "", d.note ? d.note : "");
            }
            exit(0);
        }
        if (arg == "--version") { fprintf(stderr, "%s\n", flx_version()); exit(0); }
        if (!def) throw CliError{"Unknown option " + arg + ". In case this is meant to be a non-option/argument/parameter, please specify the start of non-options with '--'."};
        std::string value;
        if (!def->flag) {
            if (has_inline) value = inline_value;
            else { if (a + 1 >= argc) throw CliError{std::string("Missing value for option --") + def->long_id}; value = argv[++a]; }
        }
        std::string const n = def->long_id;
        if (n == "reference") { o.reference = value; seen_ref = true; }
        else if (n == "queries") { o.queries = value; seen_q = true; }
        else if (n == "output") { o.output = value; seen_out = true; }
        else if (n == "index") o.index = value;
        else if (n == "logfile") o.logfile = value;
        else if (n == "console-debug-logs") o.console_debug_logs = true;
        else if (n == "query-errors") { o.query_errors = parse_u64(n, value); range_check(n, (double)o.query_errors, 0, 4096); o.has_query_errors = true; }
        else if (n == "error-probability") { o.error_probability = parse_double(n, value); range_check(n, o.error_probability, 0.00001, 0.99999); o.has_error_probability = true; }
        else if (n == "seed-errors") { o.seed_errors = parse_u64(n, value); range_check(n, (double)o.seed_errors, 0, 3); }
        else if (n == "max-anchors-hard") o.max_anchors_hard = parse_u64(n, value);
        else if (n == "max-anchors-soft") o.max_anchors_soft = parse_u64(n, value);
        else if (n == "anchor-group-order") {
            if (value != "count_first" && value != "errors_first" && value != "none") throw CliError{"Validation failed for option --" + n + ": Value " + value + " is not one of [count_first,errors_first,none]."};
            o.anchor_group_order = value;
        } else if (n == "anchor-choice-strategy") {
            if (value != "round_robin" && value != "full_groups" && value != "first_reported") throw CliError{"Validation failed for option --" + n + ": Value " + value + " is not one of [round_robin,full_groups,first_reported]."};
            o.anchor_choice_strategy = value;
        } else if (n == "seed-sampling-step-size") o.seed_sampling_step_size = parse_u64(n, value);
        else if (n == "dont-erase-useless-anchors") o.dont_erase_useless_anchors = true;
        else if (n == "bottom-up-pex-tree") o.bottom_up_pex_tree = true;
        else if (n == "interval-optimization") o.interval_optimization = true;
        else if (n == "extra-verification-ratio") o.extra_verification_ratio = parse_double(n, value);
        else if (n == "direct-full-verification") o.direct_full_verification = true;
        else if (n == "num-anchors-per-task") { o.num_anchors_per_task = parse_u64(n, value); if (o.num_anchors_per_task < 1) throw CliError{"Validation failed for option --" + n + ": must be at least 1."}; }
        else if (n == "without-cigar") o.without_cigar = true;
        else if (n == "threads") { o.threads = parse_u64(n, value); range_check(n, (double)o.threads, 1, 4096); }
        else if (n == "timeout") { o.timeout = parse_u64(n, value); o.has_timeout = true; }
        else if (n == "stats") o.stats = value;
        else if (n == "devices") o.devices = value;
        else if (n == "drop-duplicate-alignments") o.drop_duplicate_alignments = true;
        else if (n == "mapping-quality") o.mapping_quality = true;
        else if (n == "md-tag") o.md_tag = true;
        else if (n == "cs-tag") o.cs_tag = true;
        else if (n == "cs-tag-long") o.cs_tag_long = true;
        else if (n == "partial-alignments") o.partial_alignments = true;
        else if (n == "partial-min-span") { o.partial_min_span = parse_u64(n, value); range_check(n, (double)o.partial_min_span, 1, 100000); }
        else if (n == "partial-max") { o.partial_max = parse_u64(n, value); range_check(n, (double)o.partial_max, 1, 65535); }
        else if (n == "partial-extend") o.partial_extend = true;
        else if (n == "partial-extend-weight") { o.partial_extend_weight = parse_u64(n, value); range_check(n, (double)o.partial_extend_weight, 1, 65535); }
        else if (n == "partial-extend-xdrop") { o.partial_extend_xdrop = parse_u64(n, value); range_check(n, (double)o.partial_extend_xdrop, 1, 1073741824); }
        else if (n == "partial-extend-max-errors") { o.partial_extend_max_errors = parse_u64(n, value); range_check(n, (double)o.partial_extend_max_errors, 1, 4093); }
        else if (n == "sa-tag") o.sa_tag = true;
        else if (n == "split-tails") o.split_tails = true;
        else if (n == "left-align-indels") o.left_align_indels = true;
        else if (n == "realign-affine") o.realign_affine = true;
        else if (n == "realign-match") { o.realign_match = parse_u64(n, value); range_check(n, (double)o.realign_match, 1, 255); }
        else if (n == "realign-mismatch") { o.realign_mismatch = parse_u64(n, value); range_check(n, (double)o.realign_mismatch, 1, 255); }
        else if (n == "realign-gap-open") { o.realign_gap_open = parse_u64(n, value); range_check(n, (double)o.realign_gap_open, 1, 255); }
        else if (n == "realign-gap-extend") { o.realign_gap_extend = parse_u64(n, value); range_check(n, (double)o.realign_gap_extend, 1, 255); }
        else if (n == "realign-band") { o.realign_band = parse_u64(n, value); range_check(n, (double)o.realign_band, 1, 1024); }
        else if (n == "split-tails-weight") { o.split_tails_weight = parse_u64(n, value); range_check(n, (double)o.split_tails_weight, 1, 65535); }
        else if (n == "split-tails-xdrop") { o.split_tails_xdrop = parse_u64(n, value); range_check(n, (double)o.split_tails_xdrop, 1, 1073741824); }
        else if (n == "split-tails-min-rows") { o.split_tails_min_rows = parse_u64(n, value); range_check(n, (double)o.split_tails_min_rows, 1, 524287); }
        else if (n == "coverage") o.coverage = value;
        else if (n == "coverage-summary") o.coverage_summary = value;
        else if (n == "coverage-windows") o.coverage_windows = value;
        else if (n == "coverage-window") { o.coverage_window = parse_u64(n, value); if (o.coverage_window < 1) throw CliError{"Validation failed for option --" + n + ": must be at least 1."}; }
        else if (n == "coverage-deletions") o.coverage_deletions = true;
        else if (n == "coverage-secondary") o.coverage_secondary = true;
        else if (n == "coverage-zero") o.coverage_zero = true;
        else if (n == "coverage-min-mapq") { o.coverage_min_mapq = parse_u64(n, value); range_check(n, (double)o.coverage_min_mapq, 1, 254); }
        else if (n == "pileup") o.pileup = value;
        else if (n == "pileup-min-depth") { o.pileup_min_depth = parse_u64(n, value); range_check(n, (double)o.pileup_min_depth, 1, 4294967295.0); }
        else if (n == "pileup-min-count") { o.pileup_min_count = parse_u64(n, value); range_check(n, (double)o.pileup_min_count, 1, 4294967295.0); }
        else if (n == "pileup-min-fraction") {
            double const f = parse_double(n, value);
            if (!(f > 0.0 && f <= 1.0)) throw CliError{"Validation failed for option --" + n + ": Value " + value + " is not in (0, 1]."};
            o.pileup_min_permille = std::max<uint64_t>(1, flx_floating_point_error_aware_ceil(f * 1000.0));
        }
        else if (n == "pileup-secondary") o.pileup_secondary = true;
        else if (n == "sv-signatures") o.sv = value;
        else if (n == "sv-min-length") { o.sv_min_length = parse_u64(n, value); range_check(n, (double)o.sv_min_length, 1, 268435455.0); }
        else if (n == "sv-max-distance") { o.sv_max_distance = parse_u64(n, value); range_check(n, (double)o.sv_max_distance, 1, 4294967295.0); }
        else if (n == "sv-min-support") { o.sv_min_support = parse_u64(n, value); range_check(n, (double)o.sv_min_support, 1, 4294967295.0); }
        else if (n == "sv-secondary") o.sv_secondary = true;
        else if (n == "sv-min-mapq") { o.sv_min_mapq = parse_u64(n, value); range_check(n, (double)o.sv_min_mapq, 1, 254); }
        else if (n == "error-profile") o.error_profile = value;
        else if (n == "error-profile-secondary") o.error_profile_secondary = true;
        else if (n == "error-profile-min-mapq") { o.error_profile_min_mapq = parse_u64(n, value); range_check(n, (double)o.error_profile_min_mapq, 1, 254); }
        else if (n == "sort-by-coordinate") o.sort_by_coordinate = true;
        else if (n == "bam-index") o.bam_index = true;
        else if (n == "sort-tmp") { o.sort_tmp = value; if (value.empty()) throw CliError{"Validation failed for option --" + n + ": the directory's name is empty."}; }
        else if (n == "paf") o.paf = value;
        else if (n == "paf-cigar") o.paf_cigar = true;
        else if (n == "paf-unmapped") o.paf_unmapped = true;
        else if (n == "paf-skip-secondary") o.paf_skip_secondary = true;
        else if (n == "pileup-min-mapq") { o.pileup_min_mapq = parse_u64(n, value); range_check(n, (double)o.pileup_min_mapq, 1, 254); }
        else if (n == "max-alignments") { o.max_alignments = parse_u64(n, value); if (o.max_alignments < 1) throw CliError{"Validation failed for option --" + n + ": must be at least 1."}; }
        else if (n == "stats-input-hint") {
            if (value != "real_nanopore" && value != "simulated") throw CliError{"Validation failed for option --" + n + ": Value " + value + " is not one of [real_nanopore,simulated]."};
            o.stats_input_hint = value;
        }
    }
    if (!seen_ref) throw CliError{"Option -r/--reference is required but not set."};
    if (!seen_q) throw CliError{"Option -q/--queries is required but not set."};
    if (!seen_out && o.paf.empty()) throw CliError{"Option -o/--output is required but not set."};      // (a PAF output alone is an output)
    if (!has_ext(o.reference, {"fa", "fasta", "fna", "ffn", "fas", "faa", "mpfa", "frn"}, true)) throw CliError{"Validation failed for option -r/--reference: Expected one of the following valid extensions: [fa,fasta,fna,ffn,fas,faa,mpfa,frn](.gz)."};
    if (!file_readable(o.reference)) throw CliError{"Validation failed for option -r/--reference: The file " + o.reference + " does not exist!"};
    if (!has_ext(o.queries, {"fq", "fastq"}, true)) throw CliError{"Validation failed for option -q/--queries: Expected one of the following valid extensions: [fq,fastq](.gz)."};
    if (!file_readable(o.queries)) throw CliError{"Validation failed for option -q/--queries: The file " + o.queries + " does not exist!"};
    if (seen_out && !has_ext(o.output, {"bam", "sam"}, false)) throw CliError{"Validation failed for option -o/--output: Expected one of the following valid extensions: [bam,sam]."};
    // cross validation, floxer_cli.cpp:173-204
    if (!o.has_query_errors && !o.has_error_probability) throw CliError{"Either a fixed number of errors in the query or an error probability must be given."};
    if (!o.has_error_probability && o.query_errors < o.seed_errors)
        throw CliError{"The number of errors per query (" + std::to_string(o.query_errors) + ") must be greater or equal than the number of errors in the PEX tree leaves (" + std::to_string(o.seed_errors) + ")."};
    if (o.max_anchors_hard < o.max_anchors_soft)
        throw CliError{"The hard maximum number of anchors (" + std::to_string(o.max_anchors_hard) + ") should not be smaller than the soft maximum number of anchors (" + std::to_string(o.max_anchors_soft) + ")."};
    if (o.seed_sampling_step_size == 0) throw CliError{"Validation failed for option --seed-sampling-step-size: must be at least 1."};
    if (o.md_tag && o.without_cigar) throw CliError{"The option --md-tag needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (o.cs_tag && o.cs_tag_long) throw CliError{"The options --cs-tag and --cs-tag-long select one form of the same tag and cannot be combined."};
    if ((o.cs_tag || o.cs_tag_long) && o.without_cigar) throw CliError{"The options --cs-tag and --cs-tag-long need the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (o.partial_alignments && o.without_cigar) throw CliError{"The option --partial-alignments needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (!o.partial_alignments && (o.partial_min_span || o.partial_max)) throw CliError{"The options --partial-min-span and --partial-max need --partial-alignments."};
    if (o.partial_extend && !o.partial_alignments) throw CliError{"The option --partial-extend needs --partial-alignments."};
    if (!o.partial_extend && (o.partial_extend_weight || o.partial_extend_xdrop || o.partial_extend_max_errors))
        throw CliError{"The options --partial-extend-weight, --partial-extend-xdrop and --partial-extend-max-errors need --partial-extend."};
    if (o.sa_tag && !o.partial_alignments) throw CliError{"The option --sa-tag needs --partial-alignments."};
    if (o.split_tails && !o.partial_alignments) throw CliError{"The option --split-tails needs --partial-alignments."};
    if (o.split_tails && o.max_alignments != 1) throw CliError{"The option --split-tails judges the primary alignment and needs -N/--max-alignments 1."};
    if (o.split_tails && o.without_cigar) throw CliError{"The option --split-tails needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (!o.split_tails && (o.split_tails_weight || o.split_tails_xdrop || o.split_tails_min_rows))
        throw CliError{"The options --split-tails-weight, --split-tails-xdrop and --split-tails-min-rows need --split-tails."};
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
    if (o.wants_coverage() && o.without_cigar) throw CliError{"The options --coverage, --coverage-summary and --coverage-windows need the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (!o.wants_coverage() && (o.coverage_deletions || o.coverage_secondary || o.coverage_zero || o.coverage_min_mapq || o.coverage_window))
        throw CliError{"The options --coverage-deletions, --coverage-secondary, --coverage-zero, --coverage-min-mapq and --coverage-window need one of --coverage, --coverage-summary and --coverage-windows."};
    if (o.coverage_min_mapq && !o.mapping_quality) throw CliError{"The option --coverage-min-mapq judges the records' mapping quality and needs -Q/--mapping-quality."};
    if (o.coverage_windows.empty() != (o.coverage_window == 0)) throw CliError{"The options --coverage-windows and --coverage-window need each other."};
    if (!o.coverage.empty() && !has_ext(o.coverage, {"bedgraph"}, false)) throw CliError{"Validation failed for option --coverage: Expected one of the following valid extensions: [bedgraph]."};
    if (!o.coverage_summary.empty() && !has_ext(o.coverage_summary, {"tsv"}, false)) throw CliError{"Validation failed for option --coverage-summary: Expected one of the following valid extensions: [tsv]."};
    if (!o.coverage_windows.empty() && !has_ext(o.coverage_windows, {"tsv"}, false)) throw CliError{"Validation failed for option --coverage-windows: Expected one of the following valid extensions: [tsv]."};
    if (!o.pileup.empty() && o.without_cigar) throw CliError{"The option --pileup needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (o.pileup.empty() && (o.pileup_min_depth || o.pileup_min_count || o.pileup_min_permille || o.pileup_secondary || o.pileup_min_mapq))
        throw CliError{"The options --pileup-min-depth, --pileup-min-count, --pileup-min-fraction, --pileup-secondary and --pileup-min-mapq need --pileup."};
    if (o.pileup_min_mapq && !o.mapping_quality) throw CliError{"The option --pileup-min-mapq judges the records' mapping quality and needs -Q/--mapping-quality."};
    if (!o.pileup.empty() && !has_ext(o.pileup, {"tsv"}, false)) throw CliError{"Validation failed for option --pileup: Expected one of the following valid extensions: [tsv]."};
    if (!o.sv.empty() && o.without_cigar) throw CliError{"The option --sv-signatures needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (o.sv.empty() && (o.sv_min_length || o.sv_max_distance || o.sv_min_support || o.sv_secondary || o.sv_min_mapq))
        throw CliError{"The options --sv-min-length, --sv-max-distance, --sv-min-support, --sv-secondary and --sv-min-mapq need --sv-signatures."};
    if (o.sv_min_mapq && !o.mapping_quality) throw CliError{"The option --sv-min-mapq judges the records' mapping quality and needs -Q/--mapping-quality."};
    if (!o.sv.empty() && !has_ext(o.sv, {"tsv"}, false)) throw CliError{"Validation failed for option --sv-signatures: Expected one of the following valid extensions: [tsv]."};
    if (!o.error_profile.empty() && o.without_cigar) throw CliError{"The option --error-profile needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (o.error_profile.empty() && (o.error_profile_secondary || o.error_profile_min_mapq)) throw CliError{"The options --error-profile-secondary and --error-profile-min-mapq need --error-profile."};
    if (o.error_profile_min_mapq && !o.mapping_quality) throw CliError{"The option --error-profile-min-mapq judges the records' mapping quality and needs -Q/--mapping-quality."};
    if (!o.error_profile.empty() && !has_ext(o.error_profile, {"tsv"}, false)) throw CliError{"Validation failed for option --error-profile: Expected one of the following valid extensions: [tsv]."};
    if (!o.sort_by_coordinate && (o.bam_index || !o.sort_tmp.empty())) throw CliError{"The options --bam-index and --sort-tmp need --sort-by-coordinate."};
    if (o.sort_by_coordinate && !has_ext(o.output, {"bam"}, false)) throw CliError{"The option --sort-by-coordinate writes BAM and needs an -o/--output that ends in .bam."};
    if (!o.paf.empty() && o.without_cigar) throw CliError{"The option --paf needs the alignments' CIGARs and cannot be combined with -w/--without-cigar."};
    if (o.paf.empty() && (o.paf_cigar || o.paf_unmapped || o.paf_skip_secondary)) throw CliError{"The options --paf-cigar, --paf-unmapped and --paf-skip-secondary need --paf."};
    if (!o.paf.empty() && !has_ext(o.paf, {"paf"}, false)) throw CliError{"Validation failed for option --paf: Expected one of the following valid extensions: [paf]."};
    return o;
}

// ---------------------------------------------------------------- FASTA / FASTQ (plain or gz), input.cpp:36-148
struct LineReader {
    gzFile f;
    std::vector<char> buf;
    explicit LineReader(const char* path) : f(gzopen(path, "rb")), buf(1 << 16) { if (f) gzbuffer(f, 1 << 20); }
    ~LineReader() { if (f) gzclose(f); }
    bool getline(std::string& out) {
        out.clear();
        while (true) {
            if (!gzgets(f, buf.data(), (int)buf.size())) return !out.empty();
            size_t const n = strlen(buf.data());
            out.append(buf.data(), n);
            if (n && out.back() == '\n') { out.pop_back(); if (!out.empty() && out.back() == '\r') out.pop_back(); return true; }
        }
    }
};

std::string record_id(std::string const& tag) { return tag.substr(0, tag.find(' ')); }     // input.cpp:161-163

struct Reference { std::vector<std::string> ids; std::vector<uint64_t> lens; std::vector<uint8_t> pool; };

bool read_references(std::string const& path, Reference& ref, std::string& err) {
    LineReader in(path.c_str());
    if (!in.f) { err = "cannot open " + path; return false; }
    std::string line, id, seq;
    bool have = false;
    auto flush = [&]() {
        if (!have) return;
        if (seq.empty()) { log_line("warning", "The record %s in the reference file has an empty sequence and will be skipped.", id.c_str()); return; }
        ref.ids.push_back(id);
        ref.lens.push_back(seq.size());
        size_t const off = ref.pool.size();
        ref.pool.resize(off + seq.size());
        flx_chars_to_rank_sequence(seq.data(), seq.size(), ref.pool.data() + off);
        log_line("debug", "read reference, id: %s, length %zu", id.c_str(), seq.size());
    };
    while (in.getline(line)) {
        if (!line.empty() && line[0] == '>') { flush(); id = record_id(line.substr(1)); seq.clear(); have = true; }
        else if (have) seq += line;
    }
    flush();
    if (ref.ids.empty()) { err = "The reference file is empty, which is not allowed."; return false; }
    return true;
}

// ---------------------------------------------------------------- FASTQ, block-parallel (input.cpp:83-148)
// The file is read (and, for .gz, inflated: one gzip stream is serial) in blocks by the calling thread; everything after that is
// parallel over the records of a batch: line boundaries, ids, rank encoding. A batch keeps its raw text: ids and qualities are
// pointers into it (terminated in place), so nothing is copied per record.
unsigned io_threads(uint64_t cli_threads) {
    if (const char* env = getenv("FLX_IO_THREADS")) { unsigned const v = (unsigned)strtoul(env, nullptr, 10); if (v) return std::min(v, 64u); }
    unsigned const hw = std::max(1u, std::thread::hardware_concurrency());
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::max<uint64_t>(cli_threads, std::min(hw, 8u)), 64));
}
template <class F>
void parallel_for(size_t n, unsigned threads, F&& body) {      // body(first, last) on disjoint ranges
    unsigned const t = (unsigned)std::min<size_t>(threads, std::max<size_t>(1, n / 256));
    if (t <= 1) { body((size_t)0, n); return; }
    std::vector<std::thread> pool;
    for (unsigned i = 0; i < t; ++i) pool.emplace_back([&, i] { body(n * i / t, n * (i + 1) / t); });
    for (auto& th : pool) th.join();
}

// std::vector<char> value-initialises what resize() adds: 16 MB of zeroes in front of every 16-MB read. This allocator leaves it alone.
template <class T>
struct DefaultInit : std::allocator<T> {
    template <class U> struct rebind { using other = DefaultInit<U>; };
    template <class U> void construct(U* p) noexcept(std::is_nothrow_default_constructible<U>::value) { ::new (static_cast<void*>(p)) U; }
    template <class U, class... A> void construct(U* p, A&&... a) { ::new (static_cast<void*>(p)) U(std::forward<A>(a)...); }
};

struct ReadBatch {
    std::vector<char, DefaultInit<char>> raw;   // the batch's FASTQ text; ids / quals point into it
    std::vector<size_t> nl;                     // line ends of the text (FastqReader::next_text), four per record
    size_t n_rec = 0;                           // records the text holds
    std::vector<const char*> ids, quals;
    std::vector<uint8_t> pool;
    std::vector<uint64_t> offsets{0};
    size_t size() const { return ids.size(); }
};

struct FastqReader {
    gzFile f = nullptr;                         // gzip input
    int fd = -1;                                // plain input: read() straight into the batch's text (zlib's transparent mode copies every byte twice more)
    std::vector<char, DefaultInit<char>> carry; // text behind the last complete record of the previous batch
    bool eof = false;
    unsigned threads;
    size_t file_pos = 0, last_batch_bytes = 0;  // plain input: where the next read starts; the text the last batch took
    double s_read = 0, s_scan = 0, s_records = 0; // seconds spent reading, finding line ends, and on the records (FLX_CLI_PROFILE)
    static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    FastqReader(const char* path, unsigned threads_) : threads(threads_) {
        int const probe = open(path, O_RDONLY);
        if (probe < 0) return;
        // the pread path needs a file that can be read at an offset; a FIFO, /dev/stdin or a socket (plain or gzip: the reference reads a
        // pipe named *.fastq through an ifstream just as well) goes through zlib, whose transparent mode passes plain text through
        struct stat st;
        if (fstat(probe, &st) != 0 || !S_ISREG(st.st_mode)) {
            f = gzdopen(probe, "rb");
            if (f) gzbuffer(f, 1 << 20); else close(probe);
            return;
        }
        unsigned char magic[2] = {0, 0};
        ssize_t const got = pread(probe, magic, 2, 0);
        if (got == 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
            close(probe);
            f = gzopen(path, "rb");
            if (f) gzbuffer(f, 1 << 20);
        } else fd = probe;
    }
    ~FastqReader() { if (f) gzclose(f); if (fd >= 0) close(fd); }
    bool is_open() const { return f != nullptr || fd >= 0; }

    // the next batch of up to max_reads records; false at the end of the file or on a malformed record (err set)
    bool next(ReadBatch& b, size_t max_reads, std::string& err) {
        if (!next_text(b, max_reads, err)) return false;
        double const t_records = now_s();
        bool const ok = parse_records(b, threads, err);
        s_records += now_s() - t_records;
        return ok;
    }
    // Stage one, the reader's own thread: the text of the next batch (whole records) and its line ends. Stage two (parse_records) needs
    // nothing but the batch: the CLI runs it in the batch's task, next to the other batches' alignment, so that the one thread that has to
    // read the file in order does nothing else (it was the bound of the CLI with -I: 2.9 of 3.4 s).
    bool next_text(ReadBatch& b, size_t max_reads, std::string& err) {
        // (a recycled batch keeps its buffers: 330 MB of text and 165 MB of ranks per 16384 reads of 10 kb are not faulted in again)
        b.ids.clear(); b.quals.clear(); b.pool.clear(); b.offsets.assign(1, 0);
        auto& raw = b.raw;
        raw.clear();
        raw.insert(raw.end(), carry.begin(), carry.end());
        carry.clear();
        // ---- read until the text holds max_reads records (4 lines each) or the file ends
        size_t lines = 0, scanned = 0;
        std::vector<size_t>& nl = b.nl;         // positions of the line ends
        nl.clear();
        b.n_rec = 0;
        auto scan = [&]() {                     // line ends of raw[scanned, size): pieces of at least 8 MB, one thread each
            double const t_scan = now_s();
            size_t const lo = scanned, hi = raw.size();
            unsigned const t = (unsigned)std::min<size_t>(std::max(1u, threads), std::max<size_t>(1, (hi - lo) >> 23));
            std::vector<std::vector<size_t>> found(t);
            auto piece = [&](unsigned i) {
                size_t at = lo + (hi - lo) * i / t;
                size_t const end = lo + (hi - lo) * (i + 1) / t;
                while (at < end) {
                    const char* p = (const char*)memchr(raw.data() + at, '\n', end - at);
                    if (!p) break;
                    found[i].push_back((size_t)(p - raw.data()));
                    at = (size_t)(p - raw.data()) + 1;
                }
            };
            std::vector<std::thread> pool;
            for (unsigned i = 1; i < t; ++i) pool.emplace_back(piece, i);
            piece(0);
            for (auto& th : pool) th.join();
            for (auto const& v : found) { nl.insert(nl.end(), v.begin(), v.end()); lines += v.size(); }
            scanned = hi;
            s_scan += now_s() - t_scan;
        };
        scan();
        while (!eof && lines < 4 * max_reads) {
            // plain input: as much as the last batch took (and a little more) in one go, the pieces read by several threads (pread);
            // gzip input: 16 MB at a time through zlib
            size_t const at = raw.size(), want = f ? (size_t)16 << 20 : std::max<size_t>((size_t)16 << 20, last_batch_bytes > at ? last_batch_bytes - at + (1u << 20) : (size_t)16 << 20);
            double const t_read = now_s();
            raw.resize(at + want);
            long got;
            if (f) got = gzread(f, raw.data() + at, (unsigned)want);
            else {
                unsigned const t = (unsigned)std::min<size_t>(std::max(1u, threads), std::max<size_t>(1, want >> 24));      // >= 16 MB per thread
                std::vector<long> part(t, 0);
                std::vector<std::thread> pool;
                auto piece = [&](unsigned i) {
                    size_t const lo = want * i / t, hi = want * (i + 1) / t;
                    size_t done = 0;
                    while (lo + done < hi) {
                        ssize_t const r = pread(fd, raw.data() + at + lo + done, hi - lo - done, (off_t)(file_pos + lo + done));
                        if (r < 0) { if (errno == EINTR) continue; part[i] = -1; return; }
                        if (r == 0) break;
                        done += (size_t)r;
                    }
                    part[i] = (long)done;
                };
                for (unsigned i = 1; i < t; ++i) pool.emplace_back(piece, i);
                piece(0);
                for (auto& th : pool) th.join();
                got = 0;
                for (unsigned i = 0; i < t && got >= 0; ++i) {
                    if (part[i] < 0) got = -1;
                    else { got += part[i]; if ((size_t)part[i] < want * (i + 1) / t - want * i / t) break; }      // a short piece: the file ends inside it
                }
                if (got > 0) file_pos += (size_t)got;
            }
            if (got < 0) { err = "read error on the query file"; return false; }
            raw.resize(at + (size_t)got);
            s_read += now_s() - t_read;
            if (f && (size_t)got < want) {
                // a short read is the end of the data only when zlib agrees (a truncated .gz ends with Z_BUF_ERROR / Z_DATA_ERROR)
                int zerr = Z_OK;
                (void)gzerror(f, &zerr);
                if (zerr != Z_OK && zerr != Z_STREAM_END) { err = "the query file is truncated or corrupt (gzip stream error)"; return false; }
                eof = true;
            }
            if (!f && got == 0) eof = true;
            scan();
        }
        if (eof && !raw.empty() && raw.back() != '\n') { nl.push_back(raw.size()); raw.push_back('\n'); ++lines; }   // last line without a line end
        // blank lines at the very end of the file are not records
        while (eof && lines % 4 != 0 && lines > 0 && nl.size() >= 1 && (lines == 1 ? nl[0] == 0 : nl[lines - 1] == nl[lines - 2] + 1)) { nl.pop_back(); --lines; }
        size_t n_rec = std::min(lines / 4, max_reads);
        if (eof && lines % 4 != 0 && lines / 4 < max_reads) { err = "truncated FASTQ record at the end of the query file"; return false; }
        size_t const used = n_rec ? nl[4 * n_rec - 1] + 1 : 0;
        carry.assign(raw.begin() + (long)used, raw.end());
        raw.resize(used);
        last_batch_bytes = used;
        if (n_rec == 0) return false;
        b.n_rec = n_rec;
        return true;
    }
    // Stage two: ids, sequences (rank-encoded into the batch's pool) and qualities of the batch's records; false on a malformed record
    static bool parse_records(ReadBatch& b, unsigned threads, std::string& err) {
        auto& raw = b.raw;
        std::vector<size_t> const& nl = b.nl;
        size_t const n_rec = b.n_rec;
        // ---- records: id (up to the first blank, input.cpp:161-163), sequence, quality; terminated in place
        struct Rec { size_t id, seq, seq_len, qual; bool keep; };
        std::vector<Rec> recs(n_rec);
        std::atomic<bool> bad{false}, bad_qual{false};
        parallel_for(n_rec, threads, [&](size_t r0, size_t r1) {
            for (size_t r = r0; r < r1; ++r) {
                size_t const l0 = r ? nl[4 * r - 1] + 1 : 0, e0 = nl[4 * r], l1 = e0 + 1, e1 = nl[4 * r + 1], l3 = nl[4 * r + 2] + 1, e3 = nl[4 * r + 3];
                if (raw[l0] != '@' || raw[nl[4 * r + 1] + 1] != '+') { bad = true; continue; }
                size_t id_end = e0;
                if (id_end > l0 && raw[id_end - 1] == '\r') --id_end;
                for (size_t i = l0 + 1; i < id_end; ++i) if (raw[i] == ' ') { id_end = i; break; }
                raw[id_end] = 0;
                size_t s_end = e1, q_end = e3;
                if (s_end > l1 && raw[s_end - 1] == '\r') --s_end;
                if (q_end > l3 && raw[q_end - 1] == '\r') --q_end;
                raw[q_end] = 0;
                if (q_end - l3 != s_end - l1) { bad_qual = true; continue; }             // input.cpp:137 asserts qual.size() == seq.size()
                recs[r] = Rec{l0 + 1, l1, s_end - l1, l3, true};
            }
        });
        if (bad) { err = "malformed FASTQ record in the query file"; return false; }
        if (bad_qual) { err = "a FASTQ record's sequence and quality differ in length"; return false; }
        for (auto& rc : recs) {                 // the reference's filters on the way in (input.cpp:95-110)
            if (rc.seq_len == 0) { log_line("warning", "The record %s in the query file has an empty sequence and will be skipped.", raw.data() + rc.id); rc.keep = false; }
            else if (rc.seq_len > 100000) { log_line("warning", "skipping too large query: %s", raw.data() + rc.id); rc.keep = false; }
        }
        recs.erase(std::remove_if(recs.begin(), recs.end(), [](Rec const& x) { return !x.keep; }), recs.end());
        b.ids.resize(recs.size());
        b.quals.resize(recs.size());
        b.offsets.assign(recs.size() + 1, 0);
        for (size_t r = 0; r < recs.size(); ++r) b.offsets[r + 1] = b.offsets[r] + recs[r].seq_len;
        b.pool.resize(b.offsets.back() + 1);
        parallel_for(recs.size(), threads, [&](size_t r0, size_t r1) {
            for (size_t r = r0; r < r1; ++r) {
                b.ids[r] = raw.data() + recs[r].id;
                b.quals[r] = raw.data() + recs[r].qual;
                flx_chars_to_rank_sequence(raw.data() + recs[r].seq, recs[r].seq_len, b.pool.data() + b.offsets[r]);
            }
        });
        return true;
    }
};

std::vector<int> parse_devices(std::string spec, int n_available, std::string& err) {
    std::vector<int> out;
    if (spec.empty()) if (const char* env = getenv("FLX_DEVICES")) spec = env;
    if (spec.empty()) { if (const char* env = getenv("FLX_DEVICE")) spec = env; }
    if (spec.empty()) return {0};
    if (spec == "all") { for (int d = 0; d < n_available; ++d) out.push_back(d); return out; }
    size_t at = 0;
    while (at <= spec.size()) {
        size_t const comma = spec.find(',', at);
        std::string const part = spec.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
        size_t const dash = part.find('-');
        char* end = nullptr;
        long const lo = strtol(part.c_str(), &end, 10);
        long hi = lo;
        if (dash != std::string::npos) hi = strtol(part.c_str() + dash + 1, &end, 10);
        if (part.empty() || *end || lo < 0 || hi < lo) { err = "cannot parse the device list " + spec; return {}; }
        for (long d = lo; d <= hi; ++d) out.push_back((int)d);
        if (comma == std::string::npos) break;
        at = comma + 1;
    }
    for (int d : out) if (d >= n_available) { err = "device " + std::to_string(d) + " of the device list does not exist (" + std::to_string(n_available) + " HIP devices)"; return {}; }
    return out;
}

// the depth track's files: every device's accumulator summed into the first, finished there, and its runs and windows written as text
bool write_coverage(Options const& o, std::vector<flx_coverage*> const& covs, std::vector<std::string> const& names) {
    for (size_t i = 1; i < covs.size(); ++i)
        if (flx_coverage_absorb(covs[0], covs[i]) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
    flx_coverage* const cov = covs[0];
    if (flx_coverage_finish(cov) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
    auto open_out = [](std::string const& path) {
        FILE* f = fopen(path.c_str(), "w");
        if (!f) log_line("error", "cannot open output file: %s", path.c_str());
        return f;
    };
    auto windows_of = [&](uint64_t w, std::vector<flx_depth_window>& out) {
        out.resize(flx_coverage_num_windows(cov, w));
        if (flx_coverage_copy_windows(cov, w, out.data(), out.size()) == FLX_OK) return true;
        log_line("error", "%s", flx_last_error());
        return false;
    };
    bool ok = true;
    if (!o.coverage.empty()) {
        std::vector<flx_depth_run> runs(flx_coverage_num_runs(cov));
        if (flx_coverage_copy_runs(cov, runs.data(), runs.size()) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
        FILE* f = open_out(o.coverage);
        if (!f) return false;
        for (auto const& r : runs) fprintf(f, "%s\t%llu\t%llu\t%u\n", names[(size_t)r.reference_id].c_str(), (unsigned long long)r.start, (unsigned long long)r.end, r.depth);
        ok = fclose(f) == 0 && ok;
    }
    if (!o.coverage_summary.empty()) {
        std::vector<flx_depth_window> win;
        if (!windows_of(0, win)) return false;
        FILE* f = open_out(o.coverage_summary);
        if (!f) return false;
        for (auto const& w : win) fprintf(f, "%s\t%llu\t%llu\t%llu\t%u\n", names[(size_t)w.reference_id].c_str(), (unsigned long long)w.end, (unsigned long long)w.covered, (unsigned long long)w.depth_sum, w.max_depth);
        ok = fclose(f) == 0 && ok;
    }
    if (!o.coverage_windows.empty()) {
        std::vector<flx_depth_window> win;
        if (!windows_of(o.coverage_window, win)) return false;
        FILE* f = open_out(o.coverage_windows);
        if (!f) return false;
        for (auto const& w : win)
            fprintf(f, "%s\t%llu\t%llu\t%llu\t%llu\t%u\n", names[(size_t)w.reference_id].c_str(), (unsigned long long)w.start, (unsigned long long)w.end, (unsigned long long)w.depth_sum, (unsigned long long)w.covered, w.max_depth);
        ok = fclose(f) == 0 && ok;
    }
    if (!ok) log_line("error", "write error on a coverage output");
    return ok;
}

// the variant-site table: every device's accumulator summed into the first, finished there, and its sites written as text with the
// reference letter from the sequences read here (ranks 1..4 are ACGT, anything else N) and the position 1-based
bool write_pileup(Options const& o, std::vector<flx_pileup*> const& piles, Reference const& ref) {
    for (size_t i = 1; i < piles.size(); ++i)
        if (flx_pileup_absorb(piles[0], piles[i]) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
    flx_pileup* const pile = piles[0];
    if (flx_pileup_finish(pile) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
    std::vector<flx_pileup_site> sites(flx_pileup_num_sites(pile));
    if (flx_pileup_copy_sites(pile, sites.data(), sites.size()) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
    std::vector<uint64_t> starts(ref.lens.size() + 1, 0);
    for (size_t r = 0; r < ref.lens.size(); ++r) starts[r + 1] = starts[r] + ref.lens[r];
    FILE* f = fopen(o.pileup.c_str(), "w");
    if (!f) { log_line("error", "cannot open output file: %s", o.pileup.c_str()); return false; }
    for (auto const& s : sites) {
        uint8_t const rank = ref.pool[starts[(size_t)s.reference_id] + s.position];
        fprintf(f, "%s\t%llu\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", ref.ids[(size_t)s.reference_id].c_str(), (unsigned long long)s.position + 1,
                rank >= 1 && rank <= 4 ? "ACGT"[rank - 1] : 'N', s.depth, s.alt[0], s.alt[1], s.alt[2], s.alt[3], s.del, s.ins);
    }
    if (fclose(f) != 0) { log_line("error", "write error on the pileup output"); return false; }
    return true;
}

// the error profile: every device's table summed into the first and written as text, one line per counter in the table's fixed order
// (section, keys, count; zero counters too, so the file's shape never changes), then the summary lines. Letters: . for rank 0, then A C G T N.
bool write_error_profile(Options const& o, std::vector<flx_errprof*> const& profs) {
    for (size_t i = 1; i < profs.size(); ++i)
        if (flx_errprof_absorb(profs[0], profs[i]) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
    flx_errprof_table t;
    if (flx_errprof_copy(profs[0], &t) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
    FILE* f = fopen(o.error_profile.c_str(), "w");
    if (!f) { log_line("error", "cannot open output file: %s", o.error_profile.c_str()); return false; }
    static const char letter[6] = {'.', 'A', 'C', 'G', 'T', 'N'};
    auto const u = [](uint64_t v) { return (unsigned long long)v; };
    auto const pairs = [&](const char* name, const uint64_t* v) {
        for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) fprintf(f, "%s\t%c\t%c\t%llu\n", name, letter[a], letter[b], u(v[a * 6 + b]));
    };
    // keys first .. first + n - 1; the last key is `last` when given ("64+"), the one before it `before_last` ("32+" in front of "mixed")
    auto const numbered = [&](const char* name, const uint64_t* v, int n, int first, const char* last = nullptr, const char* before_last = nullptr) {
        for (int i = 0; i < n; ++i) {
            if (last && i == n - 1) fprintf(f, "%s\t%s\t%llu\n", name, last, u(v[i]));
            else if (before_last && i == n - 2) fprintf(f, "%s\t%s\t%llu\n", name, before_last, u(v[i]));
            else fprintf(f, "%s\t%d\t%llu\n", name, first + i, u(v[i]));
        }
    };
    auto const letters = [&](const char* name, const uint64_t* v) { for (int a = 0; a < 6; ++a) fprintf(f, "%s\t%c\t%llu\n", name, letter[a], u(v[a])); };
    pairs("PAIR_EQ", t.pair_eq);
    pairs("PAIR_X", t.pair_x);
    numbered("INS_LEN", t.ins_len, 64, 1, "64+");
    numbered("DEL_LEN", t.del_len, 64, 1, "64+");
    letters("INS_LETTER", t.ins_letter);
    letters("DEL_LETTER", t.del_letter);
    numbered("HP_DEL", t.hp_del, 34, 0, "mixed", "32+");
    numbered("HP_INS", t.hp_ins, 34, 0, "mixed", "32+");
    numbered("POS_MATCH", t.pos_match, 100, 0);
    numbered("POS_MISMATCH", t.pos_mismatch, 100, 0);
    numbered("POS_INS", t.pos_ins, 100, 0);
    numbered("POS_CLIP", t.pos_clip, 100, 0);
    numbered("POS_DEL", t.pos_del, 100, 0);
    numbered("EQ_RUN", t.eq_run, 256, 1, "256+");
    numbered("IDENTITY", t.identity, 101, 0);
    static const char* const totals[8] = {"records", "matches", "mismatches", "ins_events", "ins_bases", "del_events", "del_bases", "clip_bases"};
    for (int i = 0; i < 8; ++i) fprintf(f, "TOTALS\t%s\t%llu\n", totals[i], u(t.totals[i]));
    uint64_t const matches = t.totals[1], mismatches = t.totals[2], ins = t.totals[4], del = t.totals[6], columns = matches + mismatches + ins + del;
    auto const ppm = [&](uint64_t v) { return columns ? u((uint64_t)((unsigned __int128)v * 1000000u / columns)) : 0ull; };
    uint64_t unequal = 0;
    for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) if (a != b) unequal += t.pair_eq[a * 6 + b];
    fprintf(f, "summary\tcolumns\t%llu\nsummary\terror_rate_ppm\t%llu\nsummary\tmismatch_ppm\t%llu\nsummary\tinsertion_ppm\t%llu\nsummary\tdeletion_ppm\t%llu\nsummary\teq_columns_unequal\t%llu\n",
            u(columns), ppm(mismatches + ins + del), ppm(mismatches), ppm(ins), ppm(del), u(unequal));
    if (fclose(f) != 0) { log_line("error", "write error on the error-profile output"); return false; }
    if (unequal) log_line("warning", "--error-profile: %llu columns of = words hold unequal letters (eq_columns_unequal): the records do not fit the reference or the reads", u(unequal));
    return true;
}

// the structural-variant table: every device's signatures appended to the first object's, sorted and clustered there, and the clusters
// written as text: positions 1-based; q is a length for DEL and INS and a 1-based position for BND; sides L / R for BND, . otherwise
bool write_sv(Options const& o, std::vector<flx_sv*> const& svs, std::vector<std::string> const& names) {
    for (size_t i = 1; i < svs.size(); ++i)
        if (flx_sv_absorb(svs[0], svs[i]) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
    flx_sv* const s = svs[0];
    if (flx_sv_finish(s) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
    std::vector<flx_sv_cluster> clusters(flx_sv_num_clusters(s));
    if (flx_sv_copy_clusters(s, clusters.data(), clusters.size()) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
    FILE* f = fopen(o.sv.c_str(), "w");
    if (!f) { log_line("error", "cannot open output file: %s", o.sv.c_str()); return false; }
    static const char* const types[3] = {"DEL", "INS", "BND"};
    for (auto const& c : clusters) {
        bool const bnd = c.type == 2;
        unsigned long long const one = bnd ? 1 : 0;
        fprintf(f, "%s\t%s\t%llu\t%llu\t%c\t%s\t%llu\t%llu\t%llu\t%c\t%u\n", types[c.type], names[(size_t)c.ref_a].c_str(), (unsigned long long)c.pos_a_min + 1,
                (unsigned long long)c.pos_a_max + 1, bnd ? "LR"[c.side_a] : '.', names[(size_t)c.ref_b].c_str(), c.q_min + one, c.q_median + one, c.q_max + one,
                bnd ? "LR"[c.side_b] : '.', c.support);
    }
    if (fclose(f) != 0) { log_line("error", "write error on the sv output"); return false; }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    Options o;
    try { o = parse_cli(argc, argv); }
    catch (CliError const& e) { fprintf(stderr, "[CLI PARSER ERROR]\n%s\n", e.msg.c_str()); return -1; }
    g_debug = o.console_debug_logs;
    if (!o.logfile.empty()) g_logfile = fopen(o.logfile.c_str(), "a");
    log_line("info", "successfully parsed CLI input ... starting");
    if (getenv("FLX_CLI_PARSE_ONLY")) {          // diagnostic: the FASTQ reader alone (no GPU): batches, records, seconds per stage
        FastqReader qin(o.queries.c_str(), io_threads(o.threads));
        if (!qin.is_open()) { log_line("error", "cannot open %s", o.queries.c_str()); return -1; }
        ReadBatch batch;
        std::string perr;
        uint64_t n = 0, batches = 0;
        double const t0 = FastqReader::now_s();
        while (qin.next(batch, 16384, perr)) { n += batch.ids.size(); ++batches; }
        double const secs = FastqReader::now_s() - t0;
        if (!perr.empty()) { log_line("error", "%s", perr.c_str()); return -1; }
        fprintf(stderr, "[flx cli parse only] %llu records in %llu batches, %.2f s (%.0f reads/s): reading %.2f s, line ends %.2f s, records %.2f s\n",
                (unsigned long long)n, (unsigned long long)batches, secs, n / secs, qin.s_read, qin.s_scan, qin.s_records);
        return 0;
    }

    Reference ref;
    std::string err;
    log_line("info", "reading reference sequences from %s", o.reference.c_str());
    if (!read_references(o.reference, ref, err)) { log_line("error", "An error occured while trying to read the reference from the file %s.\n%s", o.reference.c_str(), err.c_str()); return -1; }

    flx_index* index = nullptr;
    struct stat st;
    if (!o.index.empty() && stat(o.index.c_str(), &st) == 0) {
        log_line("info", "loading index from %s", o.index.c_str());
        if (flx_index_load(o.index.c_str(), &index) != FLX_OK) { log_line("error", "An error occured while trying to load the index from the file %s.\n%s", o.index.c_str(), flx_last_error()); return -1; }
        if (flx_index_matches_reference(index, ref.pool.data(), ref.lens.data(), (uint32_t)ref.ids.size()) != FLX_OK) {
            log_line("error", "The index in the file %s was not built from the reference in %s.\n%s", o.index.c_str(), o.reference.c_str(), flx_last_error());
            return -1;
        }
    } else {
        log_line("info", "building index with %llu thread%s", (unsigned long long)o.threads, o.threads == 1 ? "" : "s");
        auto const t0 = std::chrono::steady_clock::now();
        // suffix arrays on the GPU (FLX_INDEX_ON_HOST=1: the host's SA-IS; the index is the same either way)
        int const brc = getenv("FLX_INDEX_ON_HOST") ? flx_index_build(ref.pool.data(), ref.lens.data(), (uint32_t)ref.ids.size(), &index)
                                                    : flx_index_build_on_device(0, ref.pool.data(), ref.lens.data(), (uint32_t)ref.ids.size(), &index);
        if (brc != FLX_OK) { log_line("error", "index construction failed: %s", flx_last_error()); return -1; }
        log_line("info", "building index took %.3f seconds", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        if (!o.index.empty() && flx_index_save(index, o.index.c_str()) != FLX_OK)
            log_line("warning", "An error occured while trying to write the index to the file %s.\nContinuing without saving the index.\n%s", o.index.c_str(), flx_last_error());
    }

    // One context per device of the device list, all uploading the one index built / loaded above; batches of reads are dealt to
    // them in turn and written in input order (floxer.cpp:141-171: the reference's unit of parallelism is the read, too).
    int n_hip = flx_device_count();
    if (n_hip <= 0) { log_line("error", "no HIP device available; floxer_amd has no CPU fallback"); return -1; }
    std::vector<int> const devices = parse_devices(o.devices, n_hip, err);
    if (devices.empty()) { log_line("error", "%s", err.c_str()); return -1; }
    flx_stats* stats = nullptr;
    if (!o.stats.empty() && flx_stats_create(o.stats_input_hint.empty() ? nullptr : o.stats_input_hint.c_str(), &stats) != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }
    std::vector<flx_ctx*> ctxs;
    for (int d : devices) {
        flx_ctx* c = nullptr;
        if (flx_ctx_create(d, index, &c) != FLX_OK) { log_line("error", "cannot set up the GPU context on device %d: %s", d, flx_last_error()); return -1; }
        if (stats) flx_ctx_set_stats(c, stats);
        ctxs.push_back(c);
    }
    log_line("info", "running on %zu HIP device context%s", ctxs.size(), ctxs.size() == 1 ? "" : "s");
    {
        int requested = 0, found = -1;
        flx_hw_queue_request(&requested, &found);
        if (requested) log_line("debug", "hardware queues: asked the HIP runtime for %d (FLX_HW_QUEUES; GPU_MAX_HW_QUEUES on entry: %d, -1 = unset)", requested, found);
        else log_line("debug", "hardware queues: GPU_MAX_HW_QUEUES left as found (%d, -1 = unset; FLX_HW_QUEUES=0)", found);
    }
    // the depth track: one accumulator per device, fed by every batch that device aligns and summed into the first after the last batch
    flx_coverage_options cov_opt;
    memset(&cov_opt, 0, sizeof(cov_opt));
    cov_opt.count_deletions = o.coverage_deletions;
    cov_opt.count_secondary = o.coverage_secondary;
    cov_opt.min_mapq = (uint32_t)o.coverage_min_mapq;
    cov_opt.report_zero = o.coverage_zero;
    std::vector<flx_coverage*> covs;
    if (o.wants_coverage())
        for (flx_ctx* c : ctxs) {
            flx_coverage* cov = nullptr;
            if (flx_coverage_create(c, &cov_opt, &cov) != FLX_OK) { log_line("error", "cannot set up the coverage accumulator: %s", flx_last_error()); return -1; }
            covs.push_back(cov);
        }
    // the allele pileup: one accumulator per device too, fed with every batch's run and its own host reads
    flx_pileup_options pile_opt;
    memset(&pile_opt, 0, sizeof(pile_opt));
    pile_opt.count_secondary = o.pileup_secondary;
    pile_opt.min_mapq = (uint32_t)o.pileup_min_mapq;
    pile_opt.min_depth = (uint32_t)o.pileup_min_depth;
    pile_opt.min_count = (uint32_t)o.pileup_min_count;
    pile_opt.min_permille = (uint32_t)o.pileup_min_permille;
    std::vector<flx_pileup*> piles;
    if (!o.pileup.empty())
        for (flx_ctx* c : ctxs) {
            flx_pileup* pile = nullptr;
            if (flx_pileup_create(c, &pile_opt, &pile) != FLX_OK) { log_line("error", "cannot set up the pileup accumulator: %s", flx_last_error()); return -1; }
            piles.push_back(pile);
        }
    // the structural-variant signatures: one object per device too, fed with every batch's run and its reads' lengths
    flx_sv_options sv_opt;
    memset(&sv_opt, 0, sizeof(sv_opt));
    sv_opt.min_length = (uint32_t)o.sv_min_length;
    sv_opt.max_distance = (uint32_t)o.sv_max_distance;
    sv_opt.min_support = (uint32_t)o.sv_min_support;
    sv_opt.count_secondary = o.sv_secondary;
    sv_opt.min_mapq = (uint32_t)o.sv_min_mapq;
    std::vector<flx_sv*> svs;
    if (!o.sv.empty()) {
        if (!o.drop_duplicate_alignments)
            log_line("warning", "--sv-signatures counts records, not reads: without -D/--drop-duplicate-alignments a read's records at one locus all add to a cluster's support (use -D -N 1).");
        for (flx_ctx* c : ctxs) {
            flx_sv* s = nullptr;
            if (flx_sv_create(c, &sv_opt, &s) != FLX_OK) { log_line("error", "cannot set up the sv object: %s", flx_last_error()); return -1; }
            svs.push_back(s);
        }
    }
    // the error profile: one table per device context too, fed behind the pileup with every batch's run and its own host reads
    flx_errprof_options prof_opt;
    memset(&prof_opt, 0, sizeof(prof_opt));
    prof_opt.count_secondary = o.error_profile_secondary;
    prof_opt.min_mapq = (uint32_t)o.error_profile_min_mapq;
    std::vector<flx_errprof*> profs;
    if (!o.error_profile.empty()) {
        if (!o.drop_duplicate_alignments)
            log_line("warning", "--error-profile counts records, not reads: without -D/--drop-duplicate-alignments a read's records at one locus all add their columns (use -D -N 1).");
        for (flx_ctx* c : ctxs) {
            flx_errprof* e = nullptr;
            if (flx_errprof_create(c, &prof_opt, &e) != FLX_OK) { log_line("error", "cannot set up the error-profile object: %s", flx_last_error()); return -1; }
            profs.push_back(e);
        }
    }

    std::vector<const char*> ref_id_ptrs;
    for (auto const& s : ref.ids) ref_id_ptrs.push_back(s.c_str());
    // the PAF output: one summariser per device context, fed with every batch's copied records, and one writer
    std::vector<flx_paf*> pafs;
    flx_paf_writer* paf_out = nullptr;
    if (!o.paf.empty()) {
        for (int d : devices) {
            flx_paf* s = nullptr;
            if (flx_paf_create(d, &s) != FLX_OK) { log_line("error", "cannot set up the PAF summariser: %s", flx_last_error()); return -1; }
            pafs.push_back(s);
        }
        flx_paf_options paf_opt;
        memset(&paf_opt, 0, sizeof(paf_opt));
        paf_opt.write_cigar = o.paf_cigar;
        paf_opt.write_unmapped = o.paf_unmapped;
        paf_opt.mapq_from_records = o.mapping_quality;
        paf_opt.skip_secondary = o.paf_skip_secondary;
        if (flx_paf_open(o.paf.c_str(), ref_id_ptrs.data(), ref.lens.data(), (uint32_t)ref.ids.size(), &paf_opt, &paf_out) != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }
    }
    flx_sam_writer* out = nullptr;                                 // stays null when --paf is the only output
    if (o.output.empty()) out = nullptr;
    else if (o.sort_by_coordinate) {
        // the keys are sorted on the first device; the spill file is <dir>/<output's name>.sort.<pid>.tmp
        size_t const slash = o.output.find_last_of('/');
        std::string const dir = !o.sort_tmp.empty() ? o.sort_tmp : slash == std::string::npos ? std::string(".") : slash == 0 ? std::string("/") : o.output.substr(0, slash);
        std::string const spill = dir + "/" + (slash == std::string::npos ? o.output : o.output.substr(slash + 1)) + ".sort." + std::to_string((long long)getpid()) + ".tmp";
        if (flx_sam_open_sorted(o.output.c_str(), spill.c_str(), devices[0], o.bam_index ? 1 : 0, ref_id_ptrs.data(), ref.lens.data(), (uint32_t)ref.ids.size(), &out) != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }
    } else if (flx_sam_open(o.output.c_str(), ref_id_ptrs.data(), ref.lens.data(), (uint32_t)ref.ids.size(), &out) != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }

    flx_params p;
    flx_params_default(&p);
    p.query_error_probability = o.has_error_probability ? o.error_probability : -1.0;      // the probability wins (input.cpp:27-33)
    p.query_num_errors = o.query_errors;
    p.pex_seed_num_errors = o.seed_errors;
    p.search.max_num_anchors_hard = o.max_anchors_hard;
    p.search.max_num_anchors_soft = o.max_anchors_soft;
    p.search.anchor_group_order = o.anchor_group_order == "errors_first" ? FLX_ORDER_ERRORS_FIRST : o.anchor_group_order == "none" ? FLX_ORDER_NONE : FLX_ORDER_COUNT_FIRST;
    p.search.anchor_choice_strategy = o.anchor_choice_strategy == "full_groups" ? FLX_CHOICE_FULL_GROUPS : o.anchor_choice_strategy == "first_reported" ? FLX_CHOICE_FIRST_REPORTED : FLX_CHOICE_ROUND_ROBIN;
    p.search.erase_useless_anchors = !o.dont_erase_useless_anchors;
    p.seed_sampling_step_size = o.seed_sampling_step_size;
    p.bottom_up_pex_tree_building = o.bottom_up_pex_tree;
    p.use_interval_optimization = o.interval_optimization;
    p.extra_verification_ratio = o.extra_verification_ratio;
    p.direct_full_verification = o.direct_full_verification;
    p.without_cigar = o.without_cigar;
    p.num_anchors_per_verification_task = o.num_anchors_per_task;
    flx_output_options out_opt;
    memset(&out_opt, 0, sizeof(out_opt));
    out_opt.drop_duplicates = o.drop_duplicate_alignments;
    out_opt.max_alignments_per_read = o.max_alignments;
    out_opt.mapq = o.mapping_quality;            // (the options go with every batch, whichever device context aligns it)
    if (out) {
        flx_sam_set_mapq(out, o.mapping_quality);
        flx_sam_set_sa(out, o.sa_tag);
    }
    flx_tag_options tag_opt;
    memset(&tag_opt, 0, sizeof(tag_opt));
    tag_opt.md = o.md_tag;
    flx_partial_options partial_opt;
    memset(&partial_opt, 0, sizeof(partial_opt));
    partial_opt.enable = o.partial_alignments;
    partial_opt.min_query_span = (uint32_t)o.partial_min_span;
    partial_opt.max_records = (uint32_t)o.partial_max;
    flx_run_options run_opt;
    memset(&run_opt, 0, sizeof(run_opt));
    run_opt.output = &out_opt;
    run_opt.tags = &tag_opt;
    flx_extend_options extend_opt;
    memset(&extend_opt, 0, sizeof(extend_opt));
    extend_opt.enable = o.partial_extend;
    extend_opt.error_weight = (uint32_t)o.partial_extend_weight;
    extend_opt.x_drop = (uint32_t)o.partial_extend_xdrop;
    extend_opt.max_errors = (uint32_t)o.partial_extend_max_errors;
    run_opt.partial = &partial_opt;
    run_opt.extend = &extend_opt;
    flx_split_options split_opt;
    memset(&split_opt, 0, sizeof(split_opt));
    split_opt.enable = o.split_tails;
    split_opt.error_weight = (uint32_t)o.split_tails_weight;
    split_opt.x_drop = (uint32_t)o.split_tails_xdrop;
    split_opt.min_tail_rows = (uint32_t)o.split_tails_min_rows;
    flx_gap_options gap_opt;
    memset(&gap_opt, 0, sizeof(gap_opt));
    gap_opt.left_align = o.left_align_indels;
    flx_realign_options realign_opt;
    memset(&realign_opt, 0, sizeof(realign_opt));
    realign_opt.enable = o.realign_affine;
    realign_opt.match = (uint32_t)o.realign_match;
    realign_opt.mismatch = (uint32_t)o.realign_mismatch;
    realign_opt.gap_open = (uint32_t)o.realign_gap_open;
    realign_opt.gap_extend = (uint32_t)o.realign_gap_extend;
    realign_opt.band = (uint32_t)o.realign_band;
    flx_cs_options cs_opt;
    memset(&cs_opt, 0, sizeof(cs_opt));
    cs_opt.form = o.cs_tag_long ? 2u : o.cs_tag ? 1u : 0u;

    struct stat qst;
    stat(o.queries.c_str(), &qst);
    log_line("info", "aligning queries from a %lld bytes large file against %zu references on the GPU and writing output file to %s", (long long)qst.st_size, ref.ids.size(), out ? o.output.c_str() : o.paf.c_str());
    auto const t_align = std::chrono::steady_clock::now();
    unsigned const n_io = io_threads(o.threads);
    FastqReader qin(o.queries.c_str(), n_io);
    if (!qin.is_open()) { log_line("error", "cannot open %s", o.queries.c_str()); return -1; }
    if (out) flx_sam_set_threads(out, n_io);
    size_t batch_reads = 16384;      // 1024 reads per lane and chunk (see flx_align_reads_resident)
    if (const char* env = getenv("FLX_BATCH_READS")) { size_t const v = strtoull(env, nullptr, 10); if (v) batch_reads = v; }
    // Batches are independent: up to three are in a context at a time (their chunks share its lanes), the next one is parsed
    // while they run, and results are written in input order.
    struct Finished { std::unique_ptr<ReadBatch> batch; std::vector<flx_record> recs; std::vector<uint32_t> cig; std::vector<flx_md_ref> md_refs; std::vector<uint8_t> md; std::vector<int32_t> scores; std::vector<flx_md_ref> cs_refs; std::vector<uint8_t> cs; std::vector<flx_paf_summary> paf; std::vector<uint8_t> skipped; int rc = FLX_OK; std::string err; bool reader_error = false; };
    // FLX_CLI_PROFILE=1: seconds this run spent parsing (this thread), aligning (sum over the batches' tasks) and writing (the writer
    // thread) on stderr at the end: which of the three stages bounds the end-to-end rate
    std::atomic<uint64_t> us_parse{0}, us_align{0}, us_copy{0}, us_write{0}, us_records{0}, us_paf{0}, us_paf_write{0};
    auto const now_us = [] { return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    auto align_batch = [&](std::unique_ptr<ReadBatch> b, flx_ctx* ctx) {
        Finished f;
        flx_run* run = nullptr;
        {
            // the second stage of the reader, in this batch's own task
            uint64_t const tr = now_us();
            std::string perr;
            bool const ok = FastqReader::parse_records(*b, n_io, perr);
            us_records += now_us() - tr;
            if (!ok) { f.rc = FLX_ERR_INVALID; f.err = perr; f.reader_error = true; f.batch = std::move(b); return f; }
        }
        uint64_t const t0 = now_us();
        f.rc = flx_align_reads_cs(ctx, &p, b->pool.data(), b->offsets.data(), b->ids.size(), &run_opt, &split_opt, &gap_opt, &realign_opt, &cs_opt, &run);
        us_align += now_us() - t0;
        if (f.rc != FLX_OK) { f.err = flx_last_error(); f.batch = std::move(b); return f; }
        if (!covs.empty()) {
            size_t const at = std::find(ctxs.begin(), ctxs.end(), ctx) - ctxs.begin();
            f.rc = flx_coverage_add_run(covs[at], run);
            if (f.rc != FLX_OK) { f.err = flx_last_error(); flx_run_free(run); f.batch = std::move(b); return f; }
        }
        if (!piles.empty()) {
            size_t const at = std::find(ctxs.begin(), ctxs.end(), ctx) - ctxs.begin();
            f.rc = flx_pileup_add_run(piles[at], run, b->pool.data(), b->offsets.data(), b->ids.size());
            if (f.rc != FLX_OK) { f.err = flx_last_error(); flx_run_free(run); f.batch = std::move(b); return f; }
        }
        if (!profs.empty()) {
            size_t const at = std::find(ctxs.begin(), ctxs.end(), ctx) - ctxs.begin();
            f.rc = flx_errprof_add_run(profs[at], run, b->pool.data(), b->offsets.data(), b->ids.size());
            if (f.rc != FLX_OK) { f.err = flx_last_error(); flx_run_free(run); f.batch = std::move(b); return f; }
        }
        if (!svs.empty()) {
            size_t const at = std::find(ctxs.begin(), ctxs.end(), ctx) - ctxs.begin();
            f.rc = flx_sv_add_run(svs[at], run, b->offsets.data(), b->ids.size());
            if (f.rc != FLX_OK) { f.err = flx_last_error(); flx_run_free(run); f.batch = std::move(b); return f; }
        }
        f.recs.resize(flx_run_num_records(run));
        f.cig.resize(flx_run_num_cigar_words(run) + 1);
        f.skipped.resize(b->ids.size());
        uint64_t const t1 = now_us();
        flx_run_copy(run, f.recs.data(), f.cig.data(), f.skipped.data());
        if (o.md_tag) {
            f.md_refs.resize(f.recs.size());
            f.md.resize(flx_run_num_md_bytes(run) + 1);
            flx_run_copy_md(run, f.md_refs.data(), f.md.data());
        }
        if (o.realign_affine) {
            f.scores.resize(f.recs.size() + 1);
            flx_run_copy_scores(run, f.scores.data());
        }
        if (cs_opt.form) {
            f.cs_refs.resize(f.recs.size());
            f.cs.resize(flx_run_num_cs_bytes(run) + 1);
            flx_run_copy_cs(run, f.cs_refs.data(), f.cs.data());
        }
        flx_run_free(run);
        us_copy += now_us() - t1;
        if (!pafs.empty()) {
            uint64_t const t2 = now_us();
            size_t const at = std::find(ctxs.begin(), ctxs.end(), ctx) - ctxs.begin();
            f.paf.resize(f.recs.size() + 1);
            f.rc = flx_paf_summarize(pafs[at], f.recs.data(), f.recs.size(), f.cig.data(), f.cig.size() - 1, b->offsets.data(), b->ids.size(), ref.lens.data(),
                                     (uint32_t)ref.ids.size(), f.paf.data());
            us_paf += now_us() - t2;
            if (f.rc != FLX_OK) { f.err = flx_last_error(); f.batch = std::move(b); return f; }
        }
        f.batch = std::move(b);
        return f;
    };
    // Three stages run side by side: this thread parses the next batch, the batches in flight are aligned (one task each), a writer
    // thread takes them in input order and formats / compresses / writes them (itself on the writer's I/O threads).
    std::deque<std::future<Finished>> in_flight;           // guarded by q_mu
    std::vector<std::unique_ptr<ReadBatch>> spare_batches; // written batches, recycled by the reader (guarded by q_mu)
    std::mutex q_mu;
    std::condition_variable q_cv;
    bool no_more = false;
    uint64_t total_reads = 0, total_records = 0, n_batches = 0;
    std::atomic<bool> failed{false};
    bool eof = false, timed_out = false;
    auto write_one = [&](Finished& f) {
        if (failed.load()) return;
        if (f.rc != FLX_OK) {
            if (f.reader_error) log_line("error", "An error occured while trying to read the queries from the file %s.\n%s", o.queries.c_str(), f.err.c_str());
            else log_line("error", "An error occurred while aligning a batch of queries.\nShutting down. The output file is likely incomplete. Error message:\n%s", f.err.c_str());
            failed.store(true);
            return;
        }
        ReadBatch const& batch = *f.batch;
        for (size_t i = 0; i < f.skipped.size(); ++i)
            if (f.skipped[i]) log_line("warning", "skipping query: %s due to bad configuration regarding the number of errors.", batch.ids[i]);
        uint64_t const t0 = now_us();
        if (out && flx_sam_write_cs(out, batch.ids.data(), batch.pool.data(), batch.offsets.data(), batch.quals.data(), f.recs.data(), f.recs.size(), f.cig.data(),
                             o.md_tag ? f.md_refs.data() : nullptr, f.md.data(), o.realign_affine ? f.scores.data() : nullptr,
                             cs_opt.form ? f.cs_refs.data() : nullptr, f.cs.data()) != FLX_OK) { log_line("error", "%s", flx_last_error()); failed.store(true); }
        us_write += now_us() - t0;
        if (paf_out && !failed.load()) {
            uint64_t const t1 = now_us();
            if (flx_paf_write(paf_out, batch.ids.data(), batch.offsets.data(), f.recs.data(), f.recs.size(), f.cig.data(), f.paf.data(),
                              o.realign_affine ? f.scores.data() : nullptr, cs_opt.form ? f.cs_refs.data() : nullptr, f.cs.data()) != FLX_OK) { log_line("error", "%s", flx_last_error()); failed.store(true); }
            us_paf_write += now_us() - t1;
        }
        total_reads += batch.ids.size();
        total_records += f.recs.size();
        log_line("debug", "finished a batch: %llu queries, %llu records so far", (unsigned long long)total_reads, (unsigned long long)total_records);
    };
    std::thread writer([&] {
        while (true) {
            std::future<Finished> next;
            {
                std::unique_lock<std::mutex> g(q_mu);
                q_cv.wait(g, [&] { return !in_flight.empty() || no_more; });
                if (in_flight.empty()) return;
                next = std::move(in_flight.front());
                in_flight.pop_front();
            }
            q_cv.notify_all();
            Finished f = next.get();
            write_one(f);
            if (f.batch) { std::lock_guard<std::mutex> g(q_mu); spare_batches.push_back(std::move(f.batch)); }      // its buffers serve a later batch
        }
    });
    size_t const max_in_flight = 3 * ctxs.size() + 1;
    while (!eof && !failed.load()) {
        if (o.has_timeout && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_align).count() > (double)o.timeout) {
            log_line("warning", "Timeout happened. Shutting down now. The output file might be incomplete.");
            timed_out = true;
            break;
        }
        std::unique_ptr<ReadBatch> batch;
        {
            std::lock_guard<std::mutex> g(q_mu);
            if (!spare_batches.empty()) { batch = std::move(spare_batches.back()); spare_batches.pop_back(); }
        }
        if (!batch) batch = std::make_unique<ReadBatch>();
        uint64_t const t_parse = now_us();
        bool const got = qin.next_text(*batch, batch_reads, err);
        us_parse += now_us() - t_parse;
        if (!got) {
            eof = true;
            if (!err.empty()) { log_line("error", "An error occured while trying to read the queries from the file %s.\n%s", o.queries.c_str(), err.c_str()); failed.store(true); }
            break;
        }
        flx_ctx* const target = ctxs[n_batches++ % ctxs.size()];
        {
            std::unique_lock<std::mutex> g(q_mu);
            q_cv.wait(g, [&] { return in_flight.size() < max_in_flight; });
            in_flight.push_back(std::async(std::launch::async, align_batch, std::move(batch), target));
        }
        q_cv.notify_all();
    }
    { std::lock_guard<std::mutex> g(q_mu); no_more = true; }
    q_cv.notify_all();
    writer.join();
    auto const t_close = std::chrono::steady_clock::now();
    if (paf_out && flx_paf_close(paf_out) != FLX_OK) { log_line("error", "%s", flx_last_error()); failed.store(true); }
    for (flx_paf* s : pafs) flx_paf_free(s);
    if (out && flx_sam_close(out) != FLX_OK) { log_line("error", "%s", flx_last_error()); failed.store(true); }
    else if (o.sort_by_coordinate) log_line("info", "sorting the keys, merging the spilled batches%s took %.3f seconds", o.bam_index ? " and writing the index" : "", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_close).count());
    // (the alignment phase ends with the output file: floxer.cpp:154-179 stops its watch there; giving 40 GB of HBM back is not part of it)
    double const secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_align).count();
    if (!covs.empty() && !failed.load() && !timed_out && !write_coverage(o, covs, ref.ids)) failed.store(true);
    for (flx_coverage* c : covs) flx_coverage_free(c);
    if (!piles.empty() && !failed.load() && !timed_out && !write_pileup(o, piles, ref)) failed.store(true);
    for (flx_pileup* c : piles) flx_pileup_free(c);
    if (!svs.empty() && !failed.load() && !timed_out && !write_sv(o, svs, ref.ids)) failed.store(true);
    for (flx_sv* c : svs) flx_sv_free(c);
    if (!profs.empty() && !failed.load() && !timed_out && !write_error_profile(o, profs)) failed.store(true);
    for (flx_errprof* c : profs) flx_errprof_free(c);
    for (flx_ctx* c : ctxs) flx_ctx_destroy(c);
    flx_index_free(index);
    if (failed.load() || timed_out) return -1;
    log_line("info", "finished aligning successfully in %.3f seconds (%llu queries, %llu records)", secs, (unsigned long long)total_reads, (unsigned long long)total_records);
    if (getenv("FLX_CLI_PROFILE")) {
        fprintf(stderr, "[flx cli profile] reader thread: reading %.2f s, line ends %.2f s; records (ids, rank encoding: in the batches' own tasks) %.2f s\n", qin.s_read, qin.s_scan, us_records.load() / 1e6);
        fprintf(stderr, "[flx cli profile] wall %.2f s: parsing %.2f s (reader thread), aligning %.2f s summed over %llu batches (up to %zu in flight), copying results %.2f s, writing %.2f s (writer thread, %u I/O threads)\n",
                secs, us_parse.load() / 1e6, us_align.load() / 1e6, (unsigned long long)n_batches, max_in_flight, us_copy.load() / 1e6, us_write.load() / 1e6, n_io);
        if (!o.paf.empty()) fprintf(stderr, "[flx cli profile] PAF: summaries %.2f s summed over the batches' tasks, writing %.2f s (writer thread)\n", us_paf.load() / 1e6, us_paf_write.load() / 1e6);
    }
    if (stats) {                                                                       // floxer.cpp:182-192
        uint64_t len = 0;
        flx_stats_format(stats, o.stats != "terminal", nullptr, &len);
        std::string text(len, '\0');
        if (flx_stats_format(stats, o.stats != "terminal", &text[0], &len) == FLX_OK) {
            text.resize(strlen(text.c_str()));
            if (o.stats == "terminal") {
                for (size_t at = 0; at < text.size();) {
                    size_t const e = text.find("\n\n", at);
                    log_line("info", "%s", text.substr(at, e == std::string::npos ? std::string::npos : e - at).c_str());
                    if (e == std::string::npos) break;
                    at = e + 2;
                }
            } else if (FILE* f = fopen(o.stats.c_str(), "w")) { fwrite(text.data(), 1, text.size(), f); fclose(f); }
            else log_line("warning", "cannot write the statistics to %s", o.stats.c_str());
        }
        flx_stats_free(stats);
    }
    if (g_logfile) fclose(g_logfile);
    return 0;
}
