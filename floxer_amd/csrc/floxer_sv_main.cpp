// floxer_sv: structural-variant calls of a set of reads as VCF 4.2, over libfloxer_amd (flx_sv and flx_svcaller, include/floxer_amd.h):
//   ./floxer_sv --reference ref.fa --queries reads.fq --error-probability 0.08 --output sv.vcf
// It builds the index and one context on one device, aligns the reads batch after batch with duplicates dropped, at most one alignment
// per read and every CIGAR realigned under affine gap costs (without that an edit-distance CIGAR scatters a long deletion over many short
// D words and no signature reaches --min-length; --no-realign-affine turns it off), feeds every run to one sv object and one svcaller
// object, finishes the sv object, hands its clusters to the svcaller's finish and writes one VCF line per called DEL / INS cluster: one
// sample column, GT:GQ:DP:AD:PL. There are no partial alignments, so no junctions; BND clusters get no line anyway. No SAM or BAM is
// written. The five costs of the genotype model come from --read-error e (default: --error-probability, else 0.08) and
// --heterozygosity t exactly as floxer_variants derives them: m = -1000 log10(1 - e), x = -1000 log10(e / 3),
// h = -1000 log10((1 - e) / 2 + e / 6), prior_het = -1000 log10(t), prior_hom = -1000 log10(t / 2), each rounded to the nearest integer
// and at least 1. Diagnostics go to stderr only; exit code 0 on success, 255 (-1) on any error, a refused command line under
// [CLI PARSER ERROR] as floxer has it. The readers are cli_input's, the log lines cli_log's; the options are the table below.
//
// A line, from a row of flx_svcaller_copy_rows (positions 0-based there, 1-based here):
//   DEL   pos_a is the first deleted column: POS = max(pos_a_min, 1), the base in front of it; END = pos_a_max + q_median; SVLEN = -q_median
//   INS   pos_a is the column the inserted letters follow: POS = pos_a_min + 1; END = POS; SVLEN = q_median
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/floxer_amd.h"
#include "cli_input.hpp"
#include "cli_log.hpp"

namespace {

struct CliError { std::string msg; };

struct Options {
    std::string reference, queries, output, sample = "SAMPLE";
    bool has_reference = false, has_queries = false, has_output = false, has_query_errors = false, has_error_probability = false, has_batch_reads = false, has_read_error = false;
    uint64_t query_errors = 0, device = 0, min_length = 50, max_distance = 100, min_support = 2, flank = 50, min_depth = 4, min_mapq = 0, batch_reads = 16384;
    double error_probability = 0, min_qual = 20, heterozygosity = 0.001, read_error = 0;
    bool secondary = false, no_realign_affine = false, all_rows = false;
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
    text('r', "reference", &O::reference, "the reference the reads are aligned to (FASTA, plain or .gz)").sets(&O::has_reference),
    text('q', "queries", &O::queries, "the reads (FASTQ, plain or .gz)").sets(&O::has_queries),
    text('o', "output", &O::output, "the calls as VCF 4.2, one sample column with GT:GQ:DP:AD:PL (<file.vcf>)").sets(&O::has_output),
    count('e', "query-errors", &O::query_errors, "the errors allowed per read, as floxer's -e").range(0, 4096).sets(&O::has_query_errors),
    real('p', "error-probability", &O::error_probability, "the errors allowed per read as a fraction of its length, as floxer's -p (wins over -e)").range(0.00001, 0.99999).sets(&O::has_error_probability),
    count(0, "device", &O::device, "the HIP device to run on (default 0)").range(0, 1023),
    count(0, "min-length", &O::min_length, "the fewest symbols of a D or I word that is a signature (default 50)").range(1, 268435455),
    count(0, "max-distance", &O::max_distance, "the largest gap, in position and in length, between neighbours of one cluster (default 100)").range(1, 268435455),
    count(0, "min-support", &O::min_support, "the fewest signatures of a cluster that is called (default 2)").range(1, 1000000),
    count(0, "flank", &O::flank, "the columns a record must reach on both sides of a cluster to count as spanning it (default 50)").range(1, 1048576),
    count(0, "min-depth", &O::min_depth, "clusters with fewer counted records (carriers and spanning others) fail the filter (default 4)").range(1, 1000000),
    real(0, "min-qual", &O::min_qual, "the smallest QUAL of a call that passes the filter, phred (default 20)").range(0.01, 10000.0),
    real(0, "heterozygosity", &O::heterozygosity, "the prior probability of a heterozygous site; a homozygous one has half of it (default 0.001)").range(0.000000001, 0.5),
    real(0, "read-error", &O::read_error, "the per-read error the genotype costs are derived from (default: --error-probability, else 0.08)").range(0.00001, 0.5).sets(&O::has_read_error),
    flag(0, "secondary", &O::secondary, "secondary records (flag 256) count as well"),
    count(0, "min-mapq", &O::min_mapq, "only records with at least this mapping quality count (computed from the read's distinct loci, 0..60)").range(1, 254),
    flag(0, "no-realign-affine", &O::no_realign_affine, "do not realign the CIGARs under affine gap costs (long deletions then scatter over short words and are not seen)"),
    flag(0, "all-rows", &O::all_rows, "write the clusters genotyped 0/0 as well"),
    count(0, "batch-reads", &O::batch_reads, "the reads aligned per batch (default 16384)").range(1, 16777216).sets(&O::has_batch_reads),
    text(0, "sample", &O::sample, "the name of the VCF's sample column (default SAMPLE)"),
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
    fprintf(stderr, "floxer_sv (MI355X-native path) - usage: ./floxer_sv --reference ref.fasta --queries reads.fastq --error-probability 0.08 --output sv.vcf\n");
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
    if (!has_ext(o.output, {"vcf"}, false)) throw CliError{"Validation failed for option -o/--output: Expected one of the following valid extensions: [vcf]."};
    if (o.sample.empty() || o.sample.find_first_of(" \t\n") != std::string::npos) throw CliError{"Validation failed for option --sample: a sample name is not empty and holds no white space."};
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

// the five costs of the genotype model in centi-phred, from the per-read error and the heterozygosity (floxer_variants' derivation)
struct Costs { uint32_t m, x, h, prior_het, prior_hom; };
// (at least 1: the library takes its default for a cost of 0, and a read error below 0.00115 rounds cost_match to that)
uint32_t centiphred(double probability) { return (uint32_t)std::max<long long>(1, std::llround(-1000.0 * std::log10(probability))); }
double read_error_of(Options const& o) { return o.has_read_error ? o.read_error : o.has_error_probability ? o.error_probability : 0.08; }
Costs costs_of(Options const& o) {
    double const e = read_error_of(o), t = o.heterozygosity;
    return Costs{centiphred(1.0 - e), centiphred(e / 3.0), centiphred((1.0 - e) / 2.0 + e / 6.0), centiphred(t), centiphred(t / 2.0)};
}
uint32_t min_qual_of(Options const& o) { return (uint32_t)std::llround(o.min_qual * 100.0); }

// FLX_SV_PARSE_ONLY: the parser's view and the derived costs, before any file is opened or any device touched
void dump_options(Options const& o) {
    Costs const c = costs_of(o);
    fprintf(stderr, "reference=%s\nqueries=%s\noutput=%s\nsample=%s\n", o.reference.c_str(), o.queries.c_str(), o.output.c_str(), o.sample.c_str());
    fprintf(stderr, "query-errors=%llu\nerror-probability=%g\ndevice=%llu\nmin-length=%llu\nmax-distance=%llu\nmin-support=%llu\nflank=%llu\nmin-depth=%llu\nmin-qual=%u\n",
            (unsigned long long)o.query_errors, o.has_error_probability ? o.error_probability : -1.0, (unsigned long long)o.device, (unsigned long long)o.min_length,
            (unsigned long long)o.max_distance, (unsigned long long)o.min_support, (unsigned long long)o.flank, (unsigned long long)o.min_depth, min_qual_of(o));
    fprintf(stderr, "heterozygosity=%g\nread-error=%g\nsecondary=%d\nmin-mapq=%llu\nrealign-affine=%d\nall-rows=%d\nbatch-reads=%llu\n", o.heterozygosity, read_error_of(o), (int)o.secondary,
            (unsigned long long)o.min_mapq, (int)!o.no_realign_affine, (int)o.all_rows, (unsigned long long)o.batch_reads);
    fprintf(stderr, "cost-match=%u\ncost-mismatch=%u\ncost-het=%u\nprior-het=%u\nprior-hom=%u\n", c.m, c.x, c.h, c.prior_het, c.prior_hom);
}

// everything the run holds, given back in the right order whichever way main() ends (the objects before their context)
struct Run {
    flx_index* index = nullptr;
    flx_ctx* ctx = nullptr;
    flx_sv* sv = nullptr;
    flx_svcaller* caller = nullptr;
    ~Run() {
        if (caller) flx_svcaller_free(caller);
        if (sv) flx_sv_free(sv);
        if (ctx) flx_ctx_destroy(ctx);
        if (index) flx_index_free(index);
    }
};

char letter_of(uint32_t rank) { return rank >= 1 && rank <= 4 ? "ACGT"[rank - 1] : 'N'; }

uint64_t pos_of(flx_svcall_row const& r) { return r.type == 0 ? std::max<uint64_t>(r.pos_a_min, 1) : (uint64_t)r.pos_a_min + 1; }

// VCF 4.2 with symbolic alleles; the rows in (sequence, POS, type, q_median) order; letters of the text outside A C G T print as N
bool write_vcf(std::string const& path, Options const& o, Reference const& ref, std::vector<flx_svcall_row> rows) {
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { log_line("error", "cannot write %s", path.c_str()); return false; }
    fprintf(f, "##fileformat=VCFv4.2\n##source=floxer_sv\n");
    for (size_t r = 0; r < ref.ids.size(); ++r) fprintf(f, "##contig=<ID=%s,length=%llu>\n", ref.ids[r].c_str(), (unsigned long long)ref.lens[r]);
    fprintf(f, "##ALT=<ID=DEL,Description=\"Deletion\">\n##ALT=<ID=INS,Description=\"Insertion\">\n");
    fprintf(f, "##FILTER=<ID=PASS,Description=\"All filters passed\">\n");
    fprintf(f, "##FILTER=<ID=LowQual,Description=\"Genotyped 0/0, fewer than --min-depth counted records, or QUAL below --min-qual\">\n");
    fprintf(f, "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">\n");
    fprintf(f, "##INFO=<ID=END,Number=1,Type=Integer,Description=\"End position of the variant: the last deleted base of the rightmost member at the median length, POS for an insertion\">\n");
    fprintf(f, "##INFO=<ID=SVLEN,Number=1,Type=Integer,Description=\"The cluster's median length, negative for a deletion\">\n");
    fprintf(f, "##INFO=<ID=CIPOS,Number=2,Type=Integer,Description=\"The spread of the members' positions behind POS\">\n");
    fprintf(f, "##INFO=<ID=SUPPORT,Number=1,Type=Integer,Description=\"Signatures in the cluster\">\n");
    fprintf(f, "##INFO=<ID=IMPRECISE,Number=0,Type=Flag,Description=\"The members differ in position or in length\">\n");
    fprintf(f, "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality\">\n");
    fprintf(f, "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Counted records: carriers and the others that span the locus\">\n");
    fprintf(f, "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Records that span the locus without the event, and signatures of the event\">\n");
    fprintf(f, "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype likelihoods, the smallest 0\">\n");
    fprintf(f, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n", o.sample.c_str());
    std::vector<uint64_t> starts(ref.ids.size() + 1, 0);
    for (size_t r = 0; r < ref.ids.size(); ++r) starts[r + 1] = starts[r] + ref.lens[r];
    std::stable_sort(rows.begin(), rows.end(), [](flx_svcall_row const& a, flx_svcall_row const& b) {
        return std::make_tuple(a.ref, pos_of(a), a.type, a.q_median) < std::make_tuple(b.ref, pos_of(b), b.type, b.q_median);
    });
    static const char* const gts[3] = {"0/0", "0/1", "1/1"};
    for (auto const& r : rows) {
        if (r.gt == 0 && !o.all_rows) continue;
        bool const del = r.type == 0;
        uint64_t const pos = pos_of(r), end = del ? (uint64_t)r.pos_a_max + r.q_median : pos;
        bool const imprecise = r.pos_a_min != r.pos_a_max || r.q_min != r.q_max;
        fprintf(f, "%s\t%llu\t.\t%c\t<%s>\t%u.%02u\t%s\tSVTYPE=%s;END=%llu;SVLEN=%s%u;CIPOS=0,%u;SUPPORT=%u%s\tGT:GQ:DP:AD:PL\t%s:%u:%llu:%u,%u:%u,%u,%u\n",
                ref.ids[(size_t)r.ref].c_str(), (unsigned long long)pos, letter_of(ref.pool[starts[(size_t)r.ref] + pos - 1]), del ? "DEL" : "INS", r.qual / 100u, r.qual % 100u,
                r.pass ? "PASS" : "LowQual", del ? "DEL" : "INS", (unsigned long long)end, del ? "-" : "", r.q_median, r.pos_a_max - r.pos_a_min, r.alt_n, imprecise ? ";IMPRECISE" : "",
                gts[r.gt < 3 ? r.gt : 0], r.gq, (unsigned long long)r.ref_n + r.alt_n, r.ref_n, r.alt_n, r.pl[0], r.pl[1], r.pl[2]);
    }
    bool const ok = !ferror(f);
    return fclose(f) == 0 && ok;
}

}  // namespace

int main(int argc, char** argv) {
    Options o;
    try { o = parse_cli(argc, argv); }
    catch (CliError const& e) { fprintf(stderr, "[CLI PARSER ERROR]\n%s\n", e.msg.c_str()); return -1; }
    if (getenv("FLX_SV_PARSE_ONLY")) { dump_options(o); return 0; }
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
    Costs const costs = costs_of(o);
    log_line("info", "genotype costs in centi-phred: match %u, mismatch %u, het %u, prior het %u, prior hom %u", costs.m, costs.x, costs.h, costs.prior_het, costs.prior_hom);
    flx_sv_options sopt{};
    sopt.min_length = (uint32_t)o.min_length;
    sopt.max_distance = (uint32_t)o.max_distance;
    sopt.min_support = (uint32_t)o.min_support;
    sopt.count_secondary = o.secondary;
    sopt.min_mapq = (uint32_t)o.min_mapq;
    if (flx_sv_create(run.ctx, &sopt, &run.sv) != FLX_OK) { log_line("error", "cannot set up the sv object: %s", flx_last_error()); return -1; }
    flx_svcall_options copt{};
    copt.count_secondary = o.secondary;
    copt.min_mapq = (uint32_t)o.min_mapq;
    copt.flank = (uint32_t)o.flank;
    copt.min_depth = (uint32_t)o.min_depth;
    copt.min_qual = min_qual_of(o);
    copt.cost_match = costs.m; copt.cost_mismatch = costs.x; copt.cost_het = costs.h; copt.prior_het = costs.prior_het; copt.prior_hom = costs.prior_hom;
    if (flx_svcaller_create(run.ctx, &copt, &run.caller) != FLX_OK) { log_line("error", "cannot set up the svcaller object: %s", flx_last_error()); return -1; }

    // the alignment options: duplicates dropped, one alignment per read, the CIGARs realigned; mapping qualities only when they are judged
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
    flx_realign_options realign{};
    realign.enable = !o.no_realign_affine;
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
        int rc = flx_sv_add_run(run.sv, r, batch.offsets.data(), batch.ids.size());
        if (rc == FLX_OK) rc = flx_svcaller_add_run(run.caller, r);
        n_reads += batch.ids.size();
        n_records += flx_run_num_records(r);
        flx_run_free(r);
        if (rc != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }
        log_line("debug", "finished a batch: %llu queries, %llu records so far", (unsigned long long)n_reads, (unsigned long long)n_records);
    }
    if (!err.empty()) { log_line("error", "An error occured while trying to read the queries from the file %s.\n%s", o.queries.c_str(), err.c_str()); return -1; }
    if (flx_sv_finish(run.sv) != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }
    std::vector<flx_sv_cluster> clusters(flx_sv_num_clusters(run.sv));
    if (flx_sv_copy_clusters(run.sv, clusters.data(), clusters.size()) != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }
    if (flx_svcaller_finish(run.caller, clusters.data(), clusters.size()) != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }

    std::vector<flx_svcall_row> rows(flx_svcaller_num_rows(run.caller));
    if (flx_svcaller_copy_rows(run.caller, rows.data(), rows.size()) != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }
    if (!write_vcf(o.output, o, ref, rows)) return -1;
    log_line("info", "finished successfully: %llu queries, %llu records, %zu clusters, %zu rows", (unsigned long long)n_reads, (unsigned long long)n_records, clusters.size(), rows.size());
    return 0;
}
