// floxer_phase: read-backed phasing of the heterozygous calls of a VCF, over libfloxer_amd (flx_phase, include/floxer_amd.h):
//   ./floxer_phase --reference ref.fa --queries reads.fq --error-probability 0.08 --variants calls.vcf --output phased.vcf [--haplotags tags.tsv]
// It reads the calls, takes as sites the biallelic records with a GT of 0/1 or 1/0 in the first sample that have a form floxer_variants
// writes (an SNV, or an anchored indel with letters A C G T, an insertion of at most 32 letters), builds the index and one context on
// one device, aligns the reads batch after batch exactly as floxer_variants does (duplicates dropped, at most one alignment per read,
// left-aligned indels), feeds every run to one phase object, finishes it and writes the VCF again: a phased site's line changes only in
// FORMAT (:PS appended) and in the sample columns (GT 1|0 or 0|1 and the phase set, the 1-based POS of the set's first site, in the
// first; . in the others), an unphased site keeps its GT and gets . for PS, every other line passes through byte for byte, and one
// ##FORMAT line for PS goes in front of #CHROM unless the input has one. --haplotags writes one line per read in input order: name, hap
// (1, 2 or .), PS (or .), h1, h2, sites. No SAM or BAM is written. Diagnostics go to stderr only; exit code 0 on success, 255 (-1) on
// any error, a refused command line under [CLI PARSER ERROR] as floxer has it; nothing is written before the phasing is done. The
// readers are cli_input's, the log lines cli_log's; the options are the table below.
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
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
    std::string reference, queries, variants, output, haplotags;
    bool has_reference = false, has_queries = false, has_variants = false, has_output = false, has_haplotags = false, has_query_errors = false, has_error_probability = false,
         has_batch_reads = false;
    uint64_t query_errors = 0, device = 0, min_link = 0, min_tag_margin = 0, refine_rounds = 0, min_mapq = 0, batch_reads = 16384;
    double error_probability = 0;
    bool no_refine = false, secondary = false, realign_affine = false;
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
    text('v', "variants", &O::variants, "the calls whose heterozygous records are phased (<file.vcf>, as floxer_variants writes it)").sets(&O::has_variants),
    text('o', "output", &O::output, "the calls again, the phased ones with GT 1|0 or 0|1 and PS (<file.vcf>)").sets(&O::has_output),
    text(0, "haplotags", &O::haplotags, "one line per read: name, hap (1, 2 or .), PS, h1, h2, sites (<file.tsv>)").sets(&O::has_haplotags),
    count('e', "query-errors", &O::query_errors, "the errors allowed per read, as floxer's -e").range(0, 4096).sets(&O::has_query_errors),
    real('p', "error-probability", &O::error_probability, "the errors allowed per read as a fraction of its length, as floxer's -p (wins over -e)").range(0.00001, 0.99999).sets(&O::has_error_probability),
    count(0, "device", &O::device, "the HIP device to run on (default 0)").range(0, 1023),
    count(0, "min-link", &O::min_link, "neighbouring sites are joined when the records for and against differ by at least this (default 2)").range(1, 1000000),
    count(0, "min-tag-margin", &O::min_tag_margin, "a read is tagged when its observations for one haplotype lead by at least this (default 1)").range(1, 1000000),
    count(0, "refine-rounds", &O::refine_rounds, "rounds in which the tagged reads vote on every site's phase (default 1)").range(1, 8),
    flag(0, "no-refine", &O::no_refine, "no such round: the phase is the chain's"),
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
    fprintf(stderr, "floxer_phase (MI355X-native path) - usage: ./floxer_phase --reference ref.fasta --queries reads.fastq --error-probability 0.08 --variants calls.vcf --output phased.vcf\n");
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
// the same path, or two names of one existing file
bool same_file(std::string const& a, std::string const& b) {
    if (a == b) return true;
    struct stat sa, sb;
    return stat(a.c_str(), &sa) == 0 && stat(b.c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
}

// what the rows cannot check one by one
void cross_check(Options const& o) {
    if (!o.has_reference) throw CliError{"Option -r/--reference is required but not set."};
    if (!o.has_queries) throw CliError{"Option -q/--queries is required but not set."};
    if (!o.has_variants) throw CliError{"Option -v/--variants is required but not set."};
    if (!o.has_output) throw CliError{"Option -o/--output is required but not set."};
    if (!has_ext(o.reference, {"fa", "fasta", "fna", "ffn", "fas", "faa", "mpfa", "frn"}, true)) throw CliError{"Validation failed for option -r/--reference: Expected one of the following valid extensions: [fa,fasta,fna,ffn,fas,faa,mpfa,frn](.gz)."};
    if (!file_readable(o.reference)) throw CliError{"Validation failed for option -r/--reference: The file " + o.reference + " does not exist!"};
    if (!has_ext(o.queries, {"fq", "fastq"}, true)) throw CliError{"Validation failed for option -q/--queries: Expected one of the following valid extensions: [fq,fastq](.gz)."};
    if (!file_readable(o.queries)) throw CliError{"Validation failed for option -q/--queries: The file " + o.queries + " does not exist!"};
    if (!has_ext(o.variants, {"vcf"}, false)) throw CliError{"Validation failed for option -v/--variants: Expected one of the following valid extensions: [vcf]."};
    if (!file_readable(o.variants)) throw CliError{"Validation failed for option -v/--variants: The file " + o.variants + " does not exist!"};
    if (!has_ext(o.output, {"vcf"}, false)) throw CliError{"Validation failed for option -o/--output: Expected one of the following valid extensions: [vcf]."};
    if (same_file(o.output, o.variants)) throw CliError{"Validation failed for option -o/--output: the output is the input given with -v/--variants."};
    if (o.has_haplotags) {
        if (!has_ext(o.haplotags, {"tsv"}, false)) throw CliError{"Validation failed for option --haplotags: Expected one of the following valid extensions: [tsv]."};
        if (same_file(o.haplotags, o.output) || same_file(o.haplotags, o.variants)) throw CliError{"Validation failed for option --haplotags: the file is another file of this command line."};
    }
    if (o.no_refine && o.refine_rounds) throw CliError{"--no-refine and --refine-rounds exclude each other."};
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

// FLX_PHASE_PARSE_ONLY: the parser's view, before any file is opened or any device touched
void dump_options(Options const& o) {
    fprintf(stderr, "reference=%s\nqueries=%s\nvariants=%s\noutput=%s\nhaplotags=%s\n", o.reference.c_str(), o.queries.c_str(), o.variants.c_str(), o.output.c_str(), o.haplotags.c_str());
    fprintf(stderr, "query-errors=%llu\nerror-probability=%g\ndevice=%llu\nmin-link=%llu\nmin-tag-margin=%llu\nrefine-rounds=%llu\nno-refine=%d\nsecondary=%d\nmin-mapq=%llu\nrealign-affine=%d\nbatch-reads=%llu\n",
            (unsigned long long)o.query_errors, o.has_error_probability ? o.error_probability : -1.0, (unsigned long long)o.device, (unsigned long long)o.min_link,
            (unsigned long long)o.min_tag_margin, (unsigned long long)o.refine_rounds, (int)o.no_refine, (int)o.secondary, (unsigned long long)o.min_mapq, (int)o.realign_affine,
            (unsigned long long)o.batch_reads);
}

// everything the run holds, given back in the right order whichever way main() ends (the phase object before its context)
struct Run {
    flx_index* index = nullptr;
    flx_ctx* ctx = nullptr;
    flx_phase* phase = nullptr;
    ~Run() {
        if (phase) flx_phase_free(phase);
        if (ctx) flx_ctx_destroy(ctx);
        if (index) flx_index_free(index);
    }
};

char letter_of(uint32_t rank) { return rank >= 1 && rank <= 4 ? "ACGT"[rank - 1] : 'N'; }

// ---- the calls: every line of the input as it stands (its end of line included), and for the lines that are sites their site
struct Vcf {
    std::vector<std::string> lines;
    std::vector<int64_t> site_of;           // per line: the index of its site, or -1
    std::vector<flx_phase_site> sites;
    size_t chrom_line = 0;                  // the #CHROM line
    bool has_ps_header = false;
};

std::vector<std::string> split(std::string const& s, char sep) {
    std::vector<std::string> out;
    size_t at = 0;
    for (;;) {
        size_t const e = s.find(sep, at);
        out.push_back(s.substr(at, e == std::string::npos ? std::string::npos : e - at));
        if (e == std::string::npos) return out;
        at = e + 1;
    }
}
std::string join(std::vector<std::string> const& v, char sep) {
    std::string out;
    for (size_t i = 0; i < v.size(); ++i) { if (i) out += sep; out += v[i]; }
    return out;
}
bool plain_letters(std::string const& s) { return !s.empty() && s.find_first_not_of("ACGT") == std::string::npos; }
// a line without its end of line, and that end
std::string body_of(std::string const& line, std::string& eol) {
    size_t n = line.size();
    while (n > 0 && (line[n - 1] == '\n' || line[n - 1] == '\r')) --n;
    eol = line.substr(n);
    return line.substr(0, n);
}

// false: refused as an input error (err set); nothing has been written by then
bool read_vcf(std::string const& path, Reference const& ref, Vcf& vcf, std::string& err) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { err = "cannot open the file"; return false; }
    std::string all;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) all.append(buf, got);
    bool const bad = ferror(f) != 0;
    fclose(f);
    if (bad) { err = "cannot read the file"; return false; }
    for (size_t at = 0; at < all.size();) {
        size_t const e = all.find('\n', at);
        size_t const end = e == std::string::npos ? all.size() : e + 1;
        vcf.lines.push_back(all.substr(at, end - at));
        at = end;
    }
    std::vector<uint64_t> starts(ref.ids.size() + 1, 0);
    for (size_t r = 0; r < ref.ids.size(); ++r) starts[r + 1] = starts[r] + ref.lens[r];
    vcf.site_of.assign(vcf.lines.size(), -1);
    bool seen_chrom = false;
    int64_t last_ref = -1;
    uint64_t last_pos = 0;
    for (size_t i = 0; i < vcf.lines.size(); ++i) {
        std::string eol;
        std::string const line = body_of(vcf.lines[i], eol);
        std::string const where = "line " + std::to_string(i + 1);
        if (line.empty()) continue;
        if (line[0] == '#') {
            if (line.compare(0, 16, "##FORMAT=<ID=PS,") == 0) vcf.has_ps_header = true;
            if (line.compare(0, 6, "#CHROM") == 0) {
                if (seen_chrom) { err = where + ": a second #CHROM line"; return false; }
                seen_chrom = true;
                vcf.chrom_line = i;
            }
            continue;
        }
        if (!seen_chrom) { err = where + ": a record in front of the #CHROM line"; return false; }
        std::vector<std::string> const col = split(line, '\t');
        if (col.size() < 8) { err = where + ": fewer than eight columns"; return false; }
        size_t r = 0;
        while (r < ref.ids.size() && ref.ids[r] != col[0]) ++r;
        if (r == ref.ids.size()) { err = where + ": the contig " + col[0] + " is not in the reference"; return false; }
        char* end = nullptr;
        unsigned long long const pos1 = strtoull(col[1].c_str(), &end, 10);
        if (col[1].empty() || *end || pos1 < 1 || col[3].empty() || pos1 - 1 + col[3].size() > ref.lens[r]) { err = where + ": POS and REF do not lie inside the contig"; return false; }
        uint64_t const pos = pos1 - 1;
        if ((int64_t)r < last_ref || ((int64_t)r == last_ref && pos < last_pos)) { err = where + ": the records are out of order"; return false; }
        for (size_t k = 0; k < col[3].size(); ++k)
            if (col[3][k] != letter_of(ref.pool[starts[r] + pos + k])) { err = where + ": REF is not the reference's letters"; return false; }
        last_ref = (int64_t)r; last_pos = pos;
        // a site: biallelic, plain letters, a form floxer_variants writes, GT 0/1 or 1/0 in the first sample
        if (col.size() < 10) continue;
        std::string const &R = col[3], &A = col[4];
        if (!plain_letters(R) || !plain_letters(A)) continue;
        flx_phase_site s{};
        s.reference_id = (int32_t)r; s.position = (uint32_t)pos;
        if (R.size() == 1 && A.size() == 1 && R != A) { s.kind = 0; s.alt_rank = (uint32_t)(std::string("ACGT").find(A[0]) + 1); s.length = 1; }
        else if (R.size() == 1 && A.size() > 1 && A.size() - 1 <= 32 && A[0] == R[0]) {
            s.kind = 2; s.length = (uint32_t)(A.size() - 1);
            for (size_t k = 1; k < A.size(); ++k) s.letters |= (uint64_t)std::string("ACGT").find(A[k]) << (62 - 2 * (k - 1));
        } else if (A.size() == 1 && R.size() > 1 && A[0] == R[0]) { s.kind = 1; s.length = (uint32_t)(R.size() - 1); }
        else continue;
        std::vector<std::string> const fmt = split(col[8], ':');
        size_t gt = 0;
        while (gt < fmt.size() && fmt[gt] != "GT") ++gt;
        std::vector<std::string> const sample = split(col[9], ':');
        if (gt >= fmt.size() || gt >= sample.size() || (sample[gt] != "0/1" && sample[gt] != "1/0")) continue;
        if (!vcf.sites.empty()) {
            flx_phase_site const& b = vcf.sites.back();
            if (b.reference_id == s.reference_id && b.position == s.position && b.kind >= s.kind) { err = where + ": the records are out of order (at one position: an SNV, then a deletion, then an insertion)"; return false; }
        }
        vcf.site_of[i] = (int64_t)vcf.sites.size();
        vcf.sites.push_back(s);
    }
    if (!seen_chrom) { err = "no #CHROM line"; return false; }
    return true;
}

// the line of a site: FORMAT with PS, the first sample with its GT and phase set, the others with .
std::string site_line(std::string const& stored, bool phased, uint32_t p, uint64_t ps) {
    std::string eol;
    std::vector<std::string> col = split(body_of(stored, eol), '\t');
    std::vector<std::string> fmt = split(col[8], ':');
    size_t gt = 0, at = 0;
    while (fmt[gt] != "GT") ++gt;                                        // (read_vcf found it)
    while (at < fmt.size() && fmt[at] != "PS") ++at;
    if (at == fmt.size()) fmt.push_back("PS");
    col[8] = join(fmt, ':');
    for (size_t c = 9; c < col.size(); ++c) {
        std::vector<std::string> v = split(col[c], ':');
        if (v.size() <= at) v.resize(at + 1, ".");
        v[at] = c == 9 && phased ? std::to_string(ps) : ".";
        if (c == 9 && phased) v[gt] = p ? "0|1" : "1|0";
        col[c] = join(v, ':');
    }
    return join(col, '\t') + eol;
}

bool write_all(std::string const& path, std::string const& content) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { log_line("error", "cannot write %s", path.c_str()); return false; }
    bool ok = fwrite(content.data(), 1, content.size(), f) == content.size();
    ok = fclose(f) == 0 && ok;
    if (!ok) { log_line("error", "cannot write %s", path.c_str()); unlink(path.c_str()); }
    return ok;
}

}  // namespace

int main(int argc, char** argv) {
    Options o;
    try { o = parse_cli(argc, argv); }
    catch (CliError const& e) { fprintf(stderr, "[CLI PARSER ERROR]\n%s\n", e.msg.c_str()); return -1; }
    if (getenv("FLX_PHASE_PARSE_ONLY")) { dump_options(o); return 0; }
    if (!o.has_batch_reads)
        if (const char* env = getenv("FLX_BATCH_READS")) { uint64_t const v = strtoull(env, nullptr, 10); if (v) o.batch_reads = v; }
    log_line("info", "successfully parsed CLI input ... starting");

    Reference ref;
    std::string err;
    log_line("info", "reading reference sequences from %s", o.reference.c_str());
    if (!read_references(o.reference, ref, err)) { log_line("error", "An error occured while trying to read the reference from the file %s.\n%s", o.reference.c_str(), err.c_str()); return -1; }
    Vcf vcf;
    if (!read_vcf(o.variants, ref, vcf, err)) { log_line("error", "An error occured while trying to read the calls from the file %s.\n%s", o.variants.c_str(), err.c_str()); return -1; }
    log_line("info", "%zu lines of calls, %zu heterozygous sites", vcf.lines.size(), vcf.sites.size());
    if (getenv("FLX_PHASE_SITES_ONLY")) {                                // the reader's view of the calls: no device is touched, nothing is written
        for (size_t i = 0; i < vcf.lines.size(); ++i) {
            if (vcf.site_of[i] < 0) continue;
            flx_phase_site const& s = vcf.sites[(size_t)vcf.site_of[i]];
            fprintf(stderr, "site line=%zu ref=%d pos=%u kind=%u alt=%u length=%u letters=%016llx\n", i + 1, s.reference_id, s.position, s.kind, s.alt_rank, s.length,
                    (unsigned long long)s.letters);
        }
        fprintf(stderr, "ps-header=%d\n", (int)vcf.has_ps_header);
        return 0;
    }
    int const n_hip = flx_device_count();
    if (n_hip <= 0) { log_line("error", "no HIP device available; floxer_amd has no CPU fallback"); return -1; }
    if ((int)o.device >= n_hip) { log_line("error", "device %llu is not among the %d HIP devices", (unsigned long long)o.device, n_hip); return -1; }
    Run run;
    uint32_t const n_refs = (uint32_t)ref.ids.size();
    if (flx_index_build_on_device((int)o.device, ref.pool.data(), ref.lens.data(), n_refs, &run.index) != FLX_OK) { log_line("error", "index construction failed: %s", flx_last_error()); return -1; }
    if (flx_ctx_create((int)o.device, run.index, &run.ctx) != FLX_OK) { log_line("error", "cannot set up the GPU context on device %llu: %s", (unsigned long long)o.device, flx_last_error()); return -1; }
    flx_phase_options popt{};
    popt.count_secondary = o.secondary;
    popt.min_mapq = (uint32_t)o.min_mapq;
    popt.min_link = (uint32_t)o.min_link;
    popt.min_margin = (uint32_t)o.min_tag_margin;
    popt.refine_rounds = (uint32_t)o.refine_rounds;
    popt.skip_refine = o.no_refine;
    if (flx_phase_create(run.ctx, &popt, vcf.sites.data(), vcf.sites.size(), &run.phase) != FLX_OK) { log_line("error", "cannot set up the phase object: %s", flx_last_error()); return -1; }

    // the alignment options, floxer_variants' own: duplicates dropped, one alignment per read, indels left-aligned; mapping qualities only when they are judged
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
    flx_split_options split_opt{};
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
    std::vector<uint64_t> batch_start;                                   // the first read of every add (one add per batch, in order)
    std::vector<std::string> names;
    while (qin.next(batch, (size_t)o.batch_reads, err)) {
        flx_run* r = nullptr;
        if (flx_align_reads_cs(run.ctx, &p, batch.pool.data(), batch.offsets.data(), batch.ids.size(), &ropt, &split_opt, &gap, &realign, &cs, &r) != FLX_OK) {
            log_line("error", "An error occurred while aligning a batch of queries.\n%s", flx_last_error());
            return -1;
        }
        int const rc = flx_phase_add_run(run.phase, r, batch.pool.data(), batch.offsets.data(), batch.ids.size());
        batch_start.push_back(n_reads);
        if (o.has_haplotags) for (const char* id : batch.ids) names.emplace_back(id);
        n_reads += batch.ids.size();
        n_records += flx_run_num_records(r);
        flx_run_free(r);
        if (rc != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }
        log_line("debug", "finished a batch: %llu queries, %llu records so far", (unsigned long long)n_reads, (unsigned long long)n_records);
    }
    if (!err.empty()) { log_line("error", "An error occured while trying to read the queries from the file %s.\n%s", o.queries.c_str(), err.c_str()); return -1; }
    if (flx_phase_finish(run.phase) != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }

    std::vector<flx_phase_result> results(flx_phase_num_sites(run.phase));
    if (flx_phase_copy_results(run.phase, results.data(), results.size()) != FLX_OK) { log_line("error", "%s", flx_last_error()); return -1; }
    std::string out;
    size_t n_phased = 0;
    for (size_t i = 0; i < vcf.lines.size(); ++i) {
        if (i == vcf.chrom_line && !vcf.has_ps_header) out += "##FORMAT=<ID=PS,Number=1,Type=Integer,Description=\"Phase set\">\n";
        if (vcf.site_of[i] < 0) { out += vcf.lines[i]; continue; }
        flx_phase_result const& res = results[(size_t)vcf.site_of[i]];
        n_phased += res.phased;
        out += site_line(vcf.lines[i], res.phased != 0, res.phase, (uint64_t)vcf.sites[res.phase_set].position + 1);
    }
    if (!write_all(o.output, out)) return -1;
    if (o.has_haplotags) {
        std::vector<flx_phase_tag> tag(flx_phase_num_tags(run.phase));
        if (flx_phase_copy_tags(run.phase, tag.data(), tag.size()) != FLX_OK) { log_line("error", "%s", flx_last_error()); unlink(o.output.c_str()); return -1; }
        std::vector<int64_t> of_read(n_reads, -1);                       // the read's first tag (one alignment per read: its only one)
        for (size_t t = 0; t < tag.size(); ++t) {
            uint64_t const read = batch_start[tag[t].add] + tag[t].read;
            if (of_read[read] < 0) of_read[read] = (int64_t)t;
        }
        std::string tsv;
        for (uint64_t r = 0; r < n_reads; ++r) {
            tsv += names[r];
            if (of_read[r] < 0) { tsv += "\t.\t.\t0\t0\t0\n"; continue; }
            flx_phase_tag const& t = tag[(size_t)of_read[r]];
            tsv += "\t" + (t.hap ? std::to_string(t.hap) : std::string(".")) + "\t" + (t.phase_set != 0xFFFFFFFFu ? std::to_string((uint64_t)vcf.sites[t.phase_set].position + 1) : std::string(".")) +
                   "\t" + std::to_string(t.h1) + "\t" + std::to_string(t.h2) + "\t" + std::to_string(t.n_slots) + "\n";
        }
        if (!write_all(o.haplotags, tsv)) { unlink(o.output.c_str()); return -1; }
    }
    log_line("info", "finished successfully: %llu queries, %llu records, %zu sites, %zu phased", (unsigned long long)n_reads, (unsigned long long)n_records, results.size(), n_phased);
    return 0;
}
