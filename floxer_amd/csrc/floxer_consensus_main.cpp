// floxer_consensus: the reference-guided consensus of a set of reads, over libfloxer_amd (flx_consensus, include/floxer_amd.h):
//   ./floxer_consensus --reference draft.fa --queries reads.fq --error-probability 0.08 --output consensus.fasta [--changes changes.tsv]
// It builds the index and one context on one device, aligns the reads batch after batch with duplicates dropped, at most one alignment
// per read and left-aligned indels (so that the reads' copies of one insertion share an anchor), feeds every run to one consensus
// object, finishes it and writes the FASTA and, if asked for, the table of changes. No SAM or BAM is written. Diagnostics go to stderr
// only; exit code 0 on success, 255 (-1) on any error, a refused command line under [CLI PARSER ERROR] as floxer has it. The readers
// are cli_input's, the log lines cli_log's; the options are the table below.
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/floxer_amd.h"
#include "cli_input.hpp"
#include "cli_log.hpp"

namespace {

struct CliError { std::string msg; };

struct Options {
    std::string reference, queries, output, changes;
    bool has_reference = false, has_queries = false, has_output = false, has_query_errors = false, has_error_probability = false, has_batch_reads = false;
    uint64_t query_errors = 0, device = 0, min_depth = 0, min_count = 0, min_mapq = 0, batch_reads = 16384;
    double error_probability = 0, min_fraction = 0;
    bool mask_low_depth = false, secondary = false, realign_affine = false;
};

// One row per option: its ids, the note --help prints, the member of Options it fills and the inclusive range of a count or a real
// (hi 0: none). `seen` is set whenever the option occurs.
struct OptDef {
    char short_id;                          // 0: long spelling only
    const char* long_id;
    const char* note;
    bool Options::* flag = nullptr;
    std::string Options::* text = nullptr;
    uint64_t Options::* count = nullptr;
    double Options::* real = nullptr;
    double lo = 0, hi = 0;
    bool Options::* seen = nullptr;
    OptDef range(double lo_, double hi_) const { OptDef d = *this; d.lo = lo_; d.hi = hi_; return d; }
    OptDef sets(bool Options::* m) const { OptDef d = *this; d.seen = m; return d; }
};
OptDef flag(char s, const char* l, bool Options::* m, const char* note) { OptDef d{s, l, note}; d.flag = m; return d; }
OptDef text(char s, const char* l, std::string Options::* m, const char* note) { OptDef d{s, l, note}; d.text = m; return d; }
OptDef count(char s, const char* l, uint64_t Options::* m, const char* note) { OptDef d{s, l, note}; d.count = m; return d; }
OptDef real(char s, const char* l, double Options::* m, const char* note) { OptDef d{s, l, note}; d.real = m; return d; }

using O = Options;
const OptDef OPTS[] = {
    text('r', "reference", &O::reference, "the draft or reference the reads are aligned to (FASTA, plain or .gz)").sets(&O::has_reference),
    text('q', "queries", &O::queries, "the reads (FASTQ, plain or .gz)").sets(&O::has_queries),
    text('o', "output", &O::output, "the consensus, one record per reference sequence in lines of 80 letters (<file.fa|.fasta>)").sets(&O::has_output),
    count('e', "query-errors", &O::query_errors, "the errors allowed per read, as floxer's -e").range(0, 4096).sets(&O::has_query_errors),
    real('p', "error-probability", &O::error_probability, "the errors allowed per read as a fraction of its length, as floxer's -p (wins over -e)").range(0.00001, 0.99999).sets(&O::has_error_probability),
    text(0, "changes", &O::changes, "one line per place the consensus departs from the reference (name, 1-based position, SUB|DEL|INS, reference letter, alternative, count, cov; <file.tsv>)"),
    count(0, "device", &O::device, "the HIP device to run on (default 0)").range(0, 1023),
    count(0, "min-depth", &O::min_depth, "positions covered by fewer records keep the reference letter (default 3)").range(1, 1000000),
    count(0, "min-count", &O::min_count, "the fewest records behind a change (default 2)").range(1, 1000000),
    real(0, "min-fraction", &O::min_fraction, "the smallest fraction of the covering records behind a change (default 0.5)").range(0.001, 1.0),
    flag(0, "mask-low-depth", &O::mask_low_depth, "write N instead of the reference letter at positions below --min-depth"),
    flag(0, "secondary", &O::secondary, "secondary records (flag 256) count as well"),
    count(0, "min-mapq", &O::min_mapq, "only records with at least this mapping quality count (computed from the read's distinct loci, 0..60)").range(1, 254),
    flag(0, "realign-affine", &O::realign_affine, "realign every CIGAR under affine gap costs before it is counted"),
    count(0, "batch-reads", &O::batch_reads, "the reads aligned per batch (default 16384)").range(1, 16777216).sets(&O::has_batch_reads),
};

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
    if (!(v >= lo && v <= hi)) throw CliError{"Validation failed for option --" + name + ": Value " + std::to_string(v) + " is not in range [" + std::to_string(lo) + "," + std::to_string(hi) + "]."};
}
void store(OptDef const& d, Options& o, std::string const& v) {
    if (d.flag) o.*d.flag = true;
    else if (d.text) o.*d.text = v;
    else if (d.count) { o.*d.count = parse_u64(d.long_id, v); if (d.hi) range_check(d.long_id, (double)(o.*d.count), d.lo, d.hi); }
    else { o.*d.real = parse_double(d.long_id, v); if (d.hi) range_check(d.long_id, o.*d.real, d.lo, d.hi); }
    if (d.seen) o.*d.seen = true;
}

void print_help() {
    fprintf(stderr, "floxer_consensus (MI355X-native path) - usage: ./floxer_consensus --reference draft.fasta --queries reads.fastq --error-probability 0.08 --output consensus.fasta\n");
    for (auto const& d : OPTS) {
        if (d.short_id) fprintf(stderr, "  -%c, ", d.short_id);
        else fprintf(stderr, "      ");
        fprintf(stderr, "--%s%s    %s\n", d.long_id, d.flag ? "" : " <value>", d.note);
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
bool file_readable(std::string const& p) { return access(p.c_str(), R_OK) == 0; }

// what the rows cannot check one by one
void cross_check(Options const& o) {
    if (!o.has_reference) throw CliError{"Option -r/--reference is required but not set."};
    if (!o.has_queries) throw CliError{"Option -q/--queries is required but not set."};
    if (!o.has_output) throw CliError{"Option -o/--output is required but not set."};
    if (!has_ext(o.reference, {"fa", "fasta", "fna", "ffn", "fas", "faa", "mpfa", "frn"}, true)) throw CliError{"Validation failed for option -r/--reference: Expected one of the following valid extensions: [fa,fasta,fna,ffn,fas,faa,mpfa,frn](.gz)."};
    if (!file_readable(o.reference)) throw CliError{"Validation failed for option -r/--reference: The file " + o.reference + " does not exist!"};
    if (!has_ext(o.queries, {"fq", "fastq"}, true)) throw CliError{"Validation failed for option -q/--queries: Expected one of the following valid extensions: [fq,fastq](.gz)."};
    if (!file_readable(o.queries)) throw CliError{"Validation failed for option -q/--queries: The file " + o.queries + " does not exist!"};
    if (!has_ext(o.output, {"fa", "fasta"}, false)) throw CliError{"Validation failed for option -o/--output: Expected one of the following valid extensions: [fa,fasta]."};
    if (!o.changes.empty() && !has_ext(o.changes, {"tsv"}, false)) throw CliError{"Validation failed for option --changes: Expected one of the following valid extensions: [tsv]."};
    if (!o.has_query_errors && !o.has_error_probability) throw CliError{"Either a fixed number of errors in the query or an error probability must be given."};
    flx_params p;
    flx_params_default(&p);
    if (!o.has_error_probability && o.query_errors < p.pex_seed_num_errors)
        throw CliError{"The number of errors per query (" + std::to_string(o.query_errors) + ") must be greater or equal than the number of errors in the PEX tree leaves (" + std::to_string(p.pex_seed_num_errors) + ")."};
}

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
        store(*def, o, value);
    }
    cross_check(o);
    return o;
}

uint32_t permille_of(Options const& o) { return o.min_fraction > 0 ? (uint32_t)std::lround(o.min_fraction * 1000.0) : 0u; }

// FLX_CONSENSUS_PARSE_ONLY: the parser's view, before any file is opened or any device touched
void dump_options(Options const& o) {
    fprintf(stderr, "reference=%s\nqueries=%s\noutput=%s\nchanges=%s\n", o.reference.c_str(), o.queries.c_str(), o.output.c_str(), o.changes.c_str());
    fprintf(stderr, "query-errors=%llu\nerror-probability=%g\ndevice=%llu\nmin-depth=%llu\nmin-count=%llu\nmin-permille=%u\nmask-low-depth=%d\nsecondary=%d\nmin-mapq=%llu\nrealign-affine=%d\nbatch-reads=%llu\n",
            (unsigned long long)o.query_errors, o.has_error_probability ? o.error_probability : -1.0, (unsigned long long)o.device, (unsigned long long)o.min_depth,
            (unsigned long long)o.min_count, permille_of(o), (int)o.mask_low_depth, (int)o.secondary, (unsigned long long)o.min_mapq, (int)o.realign_affine,
            (unsigned long long)o.batch_reads);
}

// everything the run holds, given back in the right order whichever way main() ends (the consensus object before its context)
struct Run {
    flx_index* index = nullptr;
    flx_ctx* ctx = nullptr;
    flx_consensus* cons = nullptr;
    ~Run() {
        if (cons) flx_consensus_free(cons);
        if (ctx) flx_ctx_destroy(ctx);
        if (index) flx_index_free(index);
    }
};

const char* const KINDS[3] = {"SUB", "DEL", "INS"};
char letter_of(uint32_t rank) { return rank >= 1 && rank <= 4 ? "ACGT"[rank - 1] : 'N'; }

bool write_fasta(std::string const& path, Reference const& ref, std::vector<std::string> const& letters) {
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { log_line("error", "cannot write %s", path.c_str()); return false; }
    for (size_t r = 0; r < ref.ids.size(); ++r) {
        fprintf(f, ">%s\n", ref.ids[r].c_str());
        for (size_t at = 0; at < letters[r].size(); at += 80) {
            fwrite(letters[r].data() + at, 1, std::min<size_t>(80, letters[r].size() - at), f);
            fputc('\n', f);
        }
    }
    bool const ok = !ferror(f);
    return fclose(f) == 0 && ok;
}

bool write_changes(std::string const& path, Reference const& ref, std::vector<flx_consensus_change> const& changes) {
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { log_line("error", "cannot write %s", path.c_str()); return false; }
    for (auto const& c : changes) {
        std::string alt;
        if (c.kind == 0) alt = std::string(1, letter_of(c.alt_rank));
        else if (c.kind == 1) alt = "-";
        else for (uint32_t k = 0; k < c.length; ++k) alt += "ACGT"[c.letters >> (62 - 2 * k) & 3];
        fprintf(f, "%s\t%llu\t%s\t%c\t%s\t%u\t%u\n", ref.ids[(size_t)c.reference_id].c_str(), (unsigned long long)c.position + 1, KINDS[c.kind], letter_of(c.ref_rank), alt.c_str(),
                c.count, c.cov);
    }
    bool const ok = !ferror(f);
    return fclose(f) == 0 && ok;
}

}  // namespace

int main(int argc, char** argv) {
    Options o;
    try { o = parse_cli(argc, argv); }
    catch (CliError const& e) { fprintf(stderr, "[CLI PARSER ERROR]\n%s\n", e.msg.c_str()); return -1; }
    if (getenv("FLX_CONSENSUS_PARSE_ONLY")) { dump_options(o); return 0; }
    if (!o.has_batch_reads)
        if (const char* env = getenv("FLX_BATCH_READS")) { uint64_t const v = strtoull(env, nullptr, 10); if (v) o.batch_reads = v; }
    log_line("info", "successfully parsed CLI input ... starting");

    Reference ref;
    std::string err;
    log_line("info", "reading reference sequences from %s", o.reference.c_str());
    if (!read_references(o.reference, ref, err)) { log_line("error", "An error occured while trying to read the reference from the file %s.\n%s", o.reference.c_str(), err.c_str()); return -1; }
    int const n_hip = flx_device_count();
    if (n_hip <= 0) { log_line("error", "no HIP device available; floxer_amd has no CPU fallback"); return -1; }
    if ((int)o.device >= n_hip) { log_line("error", "device %llu is not among the %d HIP devices", (unsigned long long)o.device, n_hip); return -1; }
    Run run;
    uint32_t const n_refs = (uint32_t)ref.ids.size();
    if (flx_index_build_on_device((int)o.device, ref.pool.data(), ref.lens.data(), n_refs, &run.index) != FLX_OK) { log_line("error", "index construction failed: %s", flx_last_error()); return -1; }
    if (flx_ctx_create((int)o.device, run.index, &run.ctx) != FLX_OK) { log_line("error", "cannot set up the GPU context on device %llu: %s", (unsigned long long)o.device, flx_last_error()); return -1; }
    flx_consensus_options copt{};
    copt.count_secondary = o.secondary;
    copt.min_mapq = (uint32_t)o.min_mapq;
    copt.min_depth = (uint32_t)o.min_depth;
    copt.min_count = (uint32_t)o.min_count;
    copt.min_permille = permille_of(o);
    copt.mask_low_depth = o.mask_low_depth;
    if (flx_consensus_create(run.ctx, &copt, &run.cons) != FLX_OK) { log_line("error", "cannot set up the consensus object: %s", flx_last_error()); return -1; }

    // the alignment options: duplicates dropped, one alignment per read, indels left-aligned; mapping qualities only when they are judged
    flx_params p;
    flx_params_default(&p);
    p.query_error_probability = o.has_error_probability ? o.error_probability : -1.0;
    p.query_num_errors = o.query_errors;
    flx_output_options output{};
    output.drop_duplicates = 1;
    output.max_alignments_per_read = 1;
    output.mapq = o.min_mapq > 0;
    flx_tag_options tags{};
    flx_partial_options partial{};
    flx_extend_options extend{};
    flx_split_options split{};
    flx_gap_options gap{};
    gap.left_align = 1;
    flx_realign_options realign{};
    realign.enable = o.realign_affine;
    flx_cs_options cs{};
    flx_run_options ropt{};
    ropt.output = &output;
    ropt.tags = &tags;
    ropt.partial = &partial;
    ropt.extend = &extend;

    FastqReader qin(o.queries.c_str(), io_threads(1));
    if (!qin.is_open()) { log_line("error", "cannot open %s", o.queries.c_str()); return -1; }
    ReadBatch batch;
    uint64_t n_reads = 0, n_records = 0;
    while (qin.next(batch, (size_t)o.batch_reads, err)) {
        flx_run* r = nullptr;
        if (flx_align_reads_cs(run.ctx, &p, batch.pool.data(), batch.offsets.data(), batch.ids.size(), &ropt, &split, &gap, &realign, &cs, &r) != FLX_OK) {
            log_line("error", "An error occurred while aligning a batch of queries.\n%s", flx_last_error());
            return -1;
        }
        int const rc = flx_consensus_add_run(run.cons, r, batch.pool.data(), batch.offsets.data(), batch.ids.size());
        n_reads += batch.ids.size();
        n_records += flx_run_num_records(r);
        flx_run_free(r);
        if (rc != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }
        log_line("debug", "finished a batch: %llu queries, %llu records so far", (unsigned long long)n_reads, (unsigned long long)n_records);
    }
    if (!err.empty()) { log_line("error", "An error occured while trying to read the queries from the file %s.\n%s", o.queries.c_str(), err.c_str()); return -1; }
    if (flx_consensus_finish(run.cons) != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }

    std::vector<std::string> letters(n_refs);
    for (uint32_t r = 0; r < n_refs; ++r) {
        letters[r].resize(flx_consensus_num_letters(run.cons, r));
        if (flx_consensus_copy_letters(run.cons, r, &letters[r][0], letters[r].size()) != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }
    }
    std::vector<flx_consensus_change> changes(flx_consensus_num_changes(run.cons));
    if (flx_consensus_copy_changes(run.cons, changes.data(), changes.size()) != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }
    if (!write_fasta(o.output, ref, letters)) return -1;
    if (!o.changes.empty() && !write_changes(o.changes, ref, changes)) return -1;
    log_line("info", "finished successfully: %llu queries, %llu records, %zu changes", (unsigned long long)n_reads, (unsigned long long)n_records, changes.size());
    return 0;
}
