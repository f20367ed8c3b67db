// floxer-compatible command line over libfloxer_amd (drop-in for the process boundary):
//   ./floxer --reference ref.fa --queries reads.fq --error-probability 0.08 --output out.bam   (README.md:35)
// main() follows src/main/floxer.cpp:35-195. Diagnostics go to stderr only, stdout stays empty
// (floxer_whole_program_via_cli_test.cpp:125-126); exit code 0 on success, 255 (-1) on any error.
// The options are cli_options, the readers cli_input, the side outputs cli_outputs; this file holds the stages of main() and the
// batch pipeline.
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <future>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/floxer_amd.h"
#include "cli_input.hpp"
#include "cli_log.hpp"
#include "cli_options.hpp"
#include "cli_outputs.hpp"

namespace {

using Clock = std::chrono::steady_clock;
double seconds_since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }
uint64_t now_us() { return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(Clock::now().time_since_epoch()).count(); }

// FLX_CLI_PARSE_ONLY (any value but "options"): the FASTQ reader alone (no GPU): batches, records, seconds per stage
int reader_diagnostic(Options const& o) {
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

// The index: loaded from --index when that file exists (and checked against the reference), built and saved there otherwise. Null
// behind the error line.
flx_index* load_or_build_index(Options const& o, Reference const& ref) {
    flx_index* index = nullptr;
    struct stat st;
    if (!o.index.empty() && stat(o.index.c_str(), &st) == 0) {
        log_line("info", "loading index from %s", o.index.c_str());
        if (flx_index_load(o.index.c_str(), &index) != FLX_OK) { log_line("error", "An error occured while trying to load the index from the file %s.\n%s", o.index.c_str(), flx_last_error()); return nullptr; }
        if (flx_index_matches_reference(index, ref.pool.data(), ref.lens.data(), (uint32_t)ref.ids.size()) != FLX_OK) {
            log_line("error", "The index in the file %s was not built from the reference in %s.\n%s", o.index.c_str(), o.reference.c_str(), flx_last_error());
            return nullptr;
        }
        return index;
    }
    log_line("info", "building index with %llu thread%s", (unsigned long long)o.threads, o.threads == 1 ? "" : "s");
    auto const t0 = Clock::now();
    // suffix arrays on the GPU (FLX_INDEX_ON_HOST=1: the host's SA-IS; the index is the same either way)
    int const brc = getenv("FLX_INDEX_ON_HOST") ? flx_index_build(ref.pool.data(), ref.lens.data(), (uint32_t)ref.ids.size(), &index)
                                                : flx_index_build_on_device(0, ref.pool.data(), ref.lens.data(), (uint32_t)ref.ids.size(), &index);
    if (brc != FLX_OK) { log_line("error", "index construction failed: %s", flx_last_error()); return nullptr; }
    log_line("info", "building index took %.3f seconds", seconds_since(t0));
    if (!o.index.empty() && flx_index_save(index, o.index.c_str()) != FLX_OK)
        log_line("warning", "An error occured while trying to write the index to the file %s.\nContinuing without saving the index.\n%s", o.index.c_str(), flx_last_error());
    return index;
}

// One context per device of the device list, all uploading the one index; batches of reads are dealt to them in turn and written in
// input order (floxer.cpp:141-171: the reference's unit of parallelism is the read, too). The statistics object, if asked for, is
// shared by all of them.
struct Devices {
    std::vector<int> ids;
    std::vector<flx_ctx*> ctxs;
    flx_stats* stats = nullptr;
};
bool make_contexts(Options const& o, flx_index* index, Devices& dev) {
    int n_hip = flx_device_count();
    if (n_hip <= 0) { log_line("error", "no HIP device available; floxer_amd has no CPU fallback"); return false; }
    std::string err;
    dev.ids = parse_devices(o.devices, n_hip, err);
    if (dev.ids.empty()) { log_line("error", "%s", err.c_str()); return false; }
    if (!o.stats.empty() && flx_stats_create(o.stats_input_hint.empty() ? nullptr : o.stats_input_hint.c_str(), &dev.stats) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
    for (int d : dev.ids) {
        flx_ctx* c = nullptr;
        if (flx_ctx_create(d, index, &c) != FLX_OK) { log_line("error", "cannot set up the GPU context on device %d: %s", d, flx_last_error()); return false; }
        if (dev.stats) flx_ctx_set_stats(c, dev.stats);
        dev.ctxs.push_back(c);
    }
    log_line("info", "running on %zu HIP device context%s", dev.ctxs.size(), dev.ctxs.size() == 1 ? "" : "s");
    int requested = 0, found = -1;
    flx_hw_queue_request(&requested, &found);
    if (requested) log_line("debug", "hardware queues: asked the HIP runtime for %d (FLX_HW_QUEUES; GPU_MAX_HW_QUEUES on entry: %d, -1 = unset)", requested, found);
    else log_line("debug", "hardware queues: GPU_MAX_HW_QUEUES left as found (%d, -1 = unset; FLX_HW_QUEUES=0)", found);
    return true;
}

// The ordered outputs: they take every batch's copied records in input order on the writer thread. SAM / BAM (null when --paf is the
// only output) and PAF: one summariser per device context, fed in the batch's own task, and one writer.
struct Writers {
    flx_sam_writer* out = nullptr;
    std::vector<flx_paf*> pafs;
    flx_paf_writer* paf_out = nullptr;
};
bool open_writers(Options const& o, std::vector<int> const& devices, Reference const& ref, Writers& w) {
    std::vector<const char*> names;
    for (auto const& s : ref.ids) names.push_back(s.c_str());
    uint32_t const n_refs = (uint32_t)ref.ids.size();
    if (!o.paf.empty()) {
        for (int d : devices) {
            flx_paf* s = nullptr;
            if (flx_paf_create(d, &s) != FLX_OK) { log_line("error", "cannot set up the PAF summariser: %s", flx_last_error()); return false; }
            w.pafs.push_back(s);
        }
        flx_paf_options paf_opt{};
        paf_opt.write_cigar = o.paf_cigar;
        paf_opt.write_unmapped = o.paf_unmapped;
        paf_opt.mapq_from_records = o.mapping_quality;
        paf_opt.skip_secondary = o.paf_skip_secondary;
        if (flx_paf_open(o.paf.c_str(), names.data(), ref.lens.data(), n_refs, &paf_opt, &w.paf_out) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
    }
    if (o.output.empty()) return true;
    if (o.sort_by_coordinate) {
        // the keys are sorted on the first device; the spill file is <dir>/<output's name>.sort.<pid>.tmp
        size_t const slash = o.output.find_last_of('/');
        std::string const dir = !o.sort_tmp.empty() ? o.sort_tmp : slash == std::string::npos ? std::string(".") : slash == 0 ? std::string("/") : o.output.substr(0, slash);
        std::string const spill = dir + "/" + (slash == std::string::npos ? o.output : o.output.substr(slash + 1)) + ".sort." + std::to_string((long long)getpid()) + ".tmp";
        if (flx_sam_open_sorted(o.output.c_str(), spill.c_str(), devices[0], o.bam_index ? 1 : 0, names.data(), ref.lens.data(), n_refs, &w.out) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
    } else if (flx_sam_open(o.output.c_str(), names.data(), ref.lens.data(), n_refs, &w.out) != FLX_OK) { log_line("error", "%s", flx_last_error()); return false; }
    flx_sam_set_mapq(w.out, o.mapping_quality);
    flx_sam_set_sa(w.out, o.sa_tag);
    return true;
}

// Every option struct of the library for a run, filled from the command line's options once; `run` points at its neighbours, so the
// value is not copied. (The options go with every batch, whichever device context aligns it.)
struct RunOptions {
    flx_params p;
    flx_output_options output{};
    flx_tag_options tags{};
    flx_partial_options partial{};
    flx_extend_options extend{};
    flx_split_options split{};
    flx_gap_options gap{};
    flx_realign_options realign{};
    flx_cs_options cs{};
    flx_run_options run{};
    RunOptions(RunOptions const&) = delete;
    explicit RunOptions(Options const& o) {
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
        output.drop_duplicates = o.drop_duplicate_alignments;
        output.max_alignments_per_read = o.max_alignments;
        output.mapq = o.mapping_quality;
        tags.md = o.md_tag;
        partial.enable = o.partial_alignments;
        partial.min_query_span = (uint32_t)o.partial_min_span;
        partial.max_records = (uint32_t)o.partial_max;
        extend.enable = o.partial_extend;
        extend.error_weight = (uint32_t)o.partial_extend_weight;
        extend.x_drop = (uint32_t)o.partial_extend_xdrop;
        extend.max_errors = (uint32_t)o.partial_extend_max_errors;
        split.enable = o.split_tails;
        split.error_weight = (uint32_t)o.split_tails_weight;
        split.x_drop = (uint32_t)o.split_tails_xdrop;
        split.min_tail_rows = (uint32_t)o.split_tails_min_rows;
        gap.left_align = o.left_align_indels;
        realign.enable = o.realign_affine;
        realign.match = (uint32_t)o.realign_match;
        realign.mismatch = (uint32_t)o.realign_mismatch;
        realign.gap_open = (uint32_t)o.realign_gap_open;
        realign.gap_extend = (uint32_t)o.realign_gap_extend;
        realign.band = (uint32_t)o.realign_band;
        cs.form = o.cs_tag_long ? 2u : o.cs_tag ? 1u : 0u;
        run.output = &output;
        run.tags = &tags;
        run.partial = &partial;
        run.extend = &extend;
    }
};

// What a batch's task hands to the writer thread: the batch and the copies of its run
struct Finished {
    std::unique_ptr<ReadBatch> batch;
    std::vector<flx_record> recs;
    std::vector<uint32_t> cig;
    std::vector<flx_md_ref> md_refs;            // with --md-tag
    std::vector<uint8_t> md;
    std::vector<int32_t> scores;                // with --realign-affine
    std::vector<flx_md_ref> cs_refs;            // with --cs-tag / --cs-tag-long
    std::vector<uint8_t> cs;
    std::vector<flx_paf_summary> paf;           // with --paf
    std::vector<uint8_t> skipped;
    int rc = FLX_OK;
    std::string err;
    bool reader_error = false;
};

// Three stages run side by side: the calling thread reads the next batch's text, the batches in flight are parsed and aligned (one
// task each, dealt to the contexts in turn; up to three are in a context at a time, their chunks share its lanes), a writer thread
// takes them in input order and formats / compresses / writes them (itself on the writer's I/O threads).
struct Pipeline {
    Options const& o;
    Reference const& ref;
    std::vector<flx_ctx*> const& ctxs;
    RunOptions const& opts;
    std::vector<std::unique_ptr<SideOutput>> const& sides;
    Writers const& w;
    unsigned const n_io;
    size_t const max_in_flight = 3 * ctxs.size() + 1;
    Pipeline(Options const& o_, Reference const& ref_, std::vector<flx_ctx*> const& ctxs_, RunOptions const& opts_, std::vector<std::unique_ptr<SideOutput>> const& sides_,
             Writers const& w_, unsigned n_io_) : o(o_), ref(ref_), ctxs(ctxs_), opts(opts_), sides(sides_), w(w_), n_io(n_io_) {}

    std::deque<std::future<Finished>> in_flight;           // guarded by q_mu
    std::vector<std::unique_ptr<ReadBatch>> spare_batches; // written batches, recycled by the reader (guarded by q_mu)
    std::mutex q_mu;
    std::condition_variable q_cv;
    bool no_more = false;
    uint64_t total_reads = 0, total_records = 0, n_batches = 0;
    std::atomic<bool> failed{false};
    bool timed_out = false;
    // FLX_CLI_PROFILE=1: seconds this run spent parsing (the reader thread), aligning (sum over the batches' tasks) and writing (the
    // writer thread) on stderr at the end: which of the three stages bounds the end-to-end rate
    std::atomic<uint64_t> us_parse{0}, us_align{0}, us_copy{0}, us_write{0}, us_records{0}, us_paf{0}, us_paf_write{0};

    // the optional arrays of a batch, as the writers take them: null where the option is off
    const flx_md_ref* md_refs_of(Finished const& f) const { return o.md_tag ? f.md_refs.data() : nullptr; }
    const int32_t* scores_of(Finished const& f) const { return o.realign_affine ? f.scores.data() : nullptr; }
    const flx_md_ref* cs_refs_of(Finished const& f) const { return opts.cs.form ? f.cs_refs.data() : nullptr; }

    // a batch's own task: the second stage of the reader, the alignment on context number `slot`, the side outputs, the copies
    Finished align_batch(std::unique_ptr<ReadBatch> batch, size_t slot) {
        Finished f;
        f.batch = std::move(batch);
        ReadBatch& b = *f.batch;
        uint64_t const tr = now_us();
        bool const ok = FastqReader::parse_records(b, n_io, f.err);
        us_records += now_us() - tr;
        if (!ok) { f.rc = FLX_ERR_INVALID; f.reader_error = true; return f; }
        flx_run* run = nullptr;
        uint64_t const t0 = now_us();
        f.rc = flx_align_reads_cs(ctxs[slot], &opts.p, b.pool.data(), b.offsets.data(), b.ids.size(), &opts.run, &opts.split, &opts.gap, &opts.realign, &opts.cs, &run);
        us_align += now_us() - t0;
        if (f.rc != FLX_OK) { f.err = flx_last_error(); return f; }
        for (auto const& s : sides)
            if ((f.rc = s->add(slot, run, b)) != FLX_OK) { f.err = flx_last_error(); flx_run_free(run); return f; }
        f.recs.resize(flx_run_num_records(run));
        f.cig.resize(flx_run_num_cigar_words(run) + 1);
        f.skipped.resize(b.ids.size());
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
        if (opts.cs.form) {
            f.cs_refs.resize(f.recs.size());
            f.cs.resize(flx_run_num_cs_bytes(run) + 1);
            flx_run_copy_cs(run, f.cs_refs.data(), f.cs.data());
        }
        flx_run_free(run);
        us_copy += now_us() - t1;
        if (!w.pafs.empty()) {
            uint64_t const t2 = now_us();
            f.paf.resize(f.recs.size() + 1);
            f.rc = flx_paf_summarize(w.pafs[slot], f.recs.data(), f.recs.size(), f.cig.data(), f.cig.size() - 1, b.offsets.data(), b.ids.size(), ref.lens.data(),
                                     (uint32_t)ref.ids.size(), f.paf.data());
            us_paf += now_us() - t2;
            if (f.rc != FLX_OK) f.err = flx_last_error();
        }
        return f;
    }

    // the writer thread's step: one finished batch into the ordered outputs
    void write_one(Finished& f) {
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
        if (w.out && flx_sam_write_cs(w.out, batch.ids.data(), batch.pool.data(), batch.offsets.data(), batch.quals.data(), f.recs.data(), f.recs.size(), f.cig.data(),
                                      md_refs_of(f), f.md.data(), scores_of(f), cs_refs_of(f), f.cs.data()) != FLX_OK) { log_line("error", "%s", flx_last_error()); failed.store(true); }
        us_write += now_us() - t0;
        if (w.paf_out && !failed.load()) {
            uint64_t const t1 = now_us();
            if (flx_paf_write(w.paf_out, batch.ids.data(), batch.offsets.data(), f.recs.data(), f.recs.size(), f.cig.data(), f.paf.data(), scores_of(f), cs_refs_of(f),
                              f.cs.data()) != FLX_OK) { log_line("error", "%s", flx_last_error()); failed.store(true); }
            us_paf_write += now_us() - t1;
        }
        total_reads += batch.ids.size();
        total_records += f.recs.size();
        log_line("debug", "finished a batch: %llu queries, %llu records so far", (unsigned long long)total_reads, (unsigned long long)total_records);
    }

    void writer_loop() {
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
    }

    // the reader loop, on the calling thread, until the file ends, a batch fails or the timeout passes; returns with the writer joined
    void run(FastqReader& qin, size_t batch_reads, Clock::time_point t_align) {
        std::thread writer([this] { writer_loop(); });
        std::string err;
        while (!failed.load()) {
            if (o.has_timeout && seconds_since(t_align) > (double)o.timeout) {
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
                if (!err.empty()) { log_line("error", "An error occured while trying to read the queries from the file %s.\n%s", o.queries.c_str(), err.c_str()); failed.store(true); }
                break;
            }
            size_t const slot = n_batches++ % ctxs.size();
            {
                std::unique_lock<std::mutex> g(q_mu);
                q_cv.wait(g, [&] { return in_flight.size() < max_in_flight; });
                in_flight.push_back(std::async(std::launch::async, [this, slot](std::unique_ptr<ReadBatch> b) { return align_batch(std::move(b), slot); }, std::move(batch)));
            }
            q_cv.notify_all();
        }
        { std::lock_guard<std::mutex> g(q_mu); no_more = true; }
        q_cv.notify_all();
        writer.join();
    }

    void print_profile(FastqReader const& qin, double secs) const {
        fprintf(stderr, "[flx cli profile] reader thread: reading %.2f s, line ends %.2f s; records (ids, rank encoding: in the batches' own tasks) %.2f s\n", qin.s_read, qin.s_scan, us_records.load() / 1e6);
        fprintf(stderr, "[flx cli profile] wall %.2f s: parsing %.2f s (reader thread), aligning %.2f s summed over %llu batches (up to %zu in flight), copying results %.2f s, writing %.2f s (writer thread, %u I/O threads)\n",
                secs, us_parse.load() / 1e6, us_align.load() / 1e6, (unsigned long long)n_batches, max_in_flight, us_copy.load() / 1e6, us_write.load() / 1e6, n_io);
        if (!o.paf.empty()) fprintf(stderr, "[flx cli profile] PAF: summaries %.2f s summed over the batches' tasks, writing %.2f s (writer thread)\n", us_paf.load() / 1e6, us_paf_write.load() / 1e6);
    }
};

// the statistics at the end, on the terminal or as a TOML file (floxer.cpp:182-192)
void write_statistics(Options const& o, flx_stats* stats) {
    uint64_t len = 0;
    flx_stats_format(stats, o.stats != "terminal", nullptr, &len);
    std::string text(len, '\0');
    if (flx_stats_format(stats, o.stats != "terminal", &text[0], &len) != FLX_OK) return;
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

}  // namespace

int main(int argc, char** argv) {
    Options o;
    try { o = parse_cli(argc, argv); }
    catch (CliError const& e) { fprintf(stderr, "[CLI PARSER ERROR]\n%s\n", e.msg.c_str()); return -1; }
    const char* const parse_only = getenv("FLX_CLI_PARSE_ONLY");
    if (parse_only && strcmp(parse_only, "options") == 0) { dump_options(o, stderr); return 0; }      // the parser's view, before any file is opened
    g_debug = o.console_debug_logs;
    if (!o.logfile.empty()) g_logfile = fopen(o.logfile.c_str(), "a");
    log_line("info", "successfully parsed CLI input ... starting");
    if (parse_only) return reader_diagnostic(o);

    Reference ref;
    std::string err;
    log_line("info", "reading reference sequences from %s", o.reference.c_str());
    if (!read_references(o.reference, ref, err)) { log_line("error", "An error occured while trying to read the reference from the file %s.\n%s", o.reference.c_str(), err.c_str()); return -1; }
    flx_index* const index = load_or_build_index(o, ref);
    if (!index) return -1;
    Devices dev;
    if (!make_contexts(o, index, dev)) return -1;
    std::vector<std::unique_ptr<SideOutput>> sides;      // (emptied before the contexts are destroyed: flx_ctx_destroy refuses while an error-profile object lives)
    if (!make_side_outputs(o, dev.ctxs, ref, sides)) return -1;
    Writers w;
    if (!open_writers(o, dev.ids, ref, w)) return -1;
    RunOptions const opts(o);

    struct stat qst;
    stat(o.queries.c_str(), &qst);
    log_line("info", "aligning queries from a %lld bytes large file against %zu references on the GPU and writing output file to %s", (long long)qst.st_size, ref.ids.size(), w.out ? o.output.c_str() : o.paf.c_str());
    auto const t_align = Clock::now();
    unsigned const n_io = io_threads(o.threads);
    FastqReader qin(o.queries.c_str(), n_io);
    if (!qin.is_open()) { log_line("error", "cannot open %s", o.queries.c_str()); return -1; }
    if (w.out) flx_sam_set_threads(w.out, n_io);
    size_t batch_reads = 16384;      // 1024 reads per lane and chunk (see flx_align_reads_resident)
    if (const char* env = getenv("FLX_BATCH_READS")) { size_t const v = strtoull(env, nullptr, 10); if (v) batch_reads = v; }
    Pipeline pipe(o, ref, dev.ctxs, opts, sides, w, n_io);
    pipe.run(qin, batch_reads, t_align);

    auto const t_close = Clock::now();
    if (w.paf_out && flx_paf_close(w.paf_out) != FLX_OK) { log_line("error", "%s", flx_last_error()); pipe.failed.store(true); }
    for (flx_paf* s : w.pafs) flx_paf_free(s);
    if (w.out && flx_sam_close(w.out) != FLX_OK) { log_line("error", "%s", flx_last_error()); pipe.failed.store(true); }
    else if (o.sort_by_coordinate) log_line("info", "sorting the keys, merging the spilled batches%s took %.3f seconds", o.bam_index ? " and writing the index" : "", seconds_since(t_close));
    // (the alignment phase ends with the output file: floxer.cpp:154-179 stops its watch there; giving 40 GB of HBM back is not part of it)
    double const secs = seconds_since(t_align);
    for (auto const& s : sides)
        if (!pipe.failed.load() && !pipe.timed_out && !s->write()) pipe.failed.store(true);
    sides.clear();
    for (flx_ctx* c : dev.ctxs) flx_ctx_destroy(c);
    flx_index_free(index);
    if (pipe.failed.load() || pipe.timed_out) return -1;
    log_line("info", "finished aligning successfully in %.3f seconds (%llu queries, %llu records)", secs, (unsigned long long)pipe.total_reads, (unsigned long long)pipe.total_records);
    if (getenv("FLX_CLI_PROFILE")) pipe.print_profile(qin, secs);
    if (dev.stats) { write_statistics(o, dev.stats); flx_stats_free(dev.stats); }
    if (g_logfile) fclose(g_logfile);
    return 0;
}
