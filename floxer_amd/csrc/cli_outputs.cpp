#include "cli_outputs.hpp"

#include <algorithm>
#include <cstdio>

#include "cli_log.hpp"

namespace {

// What the four share: the object per context, the sum into the first one, the text file's opening and closing, the freeing.
template <class T>
struct PerContext : SideOutput {
    Options const& o;
    Reference const& ref;
    std::vector<T*> objs;                       // one per context, in the contexts' order
    bool ready = false;                         // every object was set up
    int (*const absorb)(T*, T*);
    int (*const finish)(T*);                    // null: the object needs no finishing
    void (*const release)(T*);
    PerContext(Options const& o_, Reference const& ref_, int (*absorb_)(T*, T*), int (*finish_)(T*), void (*release_)(T*))
        : o(o_), ref(ref_), absorb(absorb_), finish(finish_), release(release_) {}
    ~PerContext() override { for (T* x : objs) release(x); }

    template <class Opt>
    void create(std::vector<flx_ctx*> const& ctxs, int (*make)(flx_ctx*, const Opt*, T**), Opt const& opt, const char* what) {
        for (flx_ctx* c : ctxs) {
            T* x = nullptr;
            if (make(c, &opt, &x) != FLX_OK) { log_line("error", "cannot set up the %s: %s", what, flx_last_error()); return; }
            objs.push_back(x);
        }
        ready = true;
    }
    // every context's object summed into the first and finished there; null behind the error line
    T* total() {
        for (size_t i = 1; i < objs.size(); ++i)
            if (absorb(objs[0], objs[i]) != FLX_OK) { log_line("error", "%s", flx_last_error()); return nullptr; }
        if (finish && finish(objs[0]) != FLX_OK) { log_line("error", "%s", flx_last_error()); return nullptr; }
        return objs[0];
    }
};

// a text file that `body` prints; false behind the error line ("write error on <what>" when closing it fails)
template <class F>
bool write_text(std::string const& path, const char* what, F&& body) {
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { log_line("error", "cannot open output file: %s", path.c_str()); return false; }
    body(f);
    if (fclose(f) != 0) { log_line("error", "write error on %s", what); return false; }
    return true;
}
bool failed_call() { log_line("error", "%s", flx_last_error()); return false; }
unsigned long long u(uint64_t v) { return (unsigned long long)v; }

// the depth track: its runs as a bedGraph file, its per-sequence and per-window sums as tables
struct Coverage : PerContext<flx_coverage> {
    Coverage(Options const& o_, std::vector<flx_ctx*> const& ctxs, Reference const& ref_) : PerContext(o_, ref_, flx_coverage_absorb, flx_coverage_finish, flx_coverage_free) {
        flx_coverage_options opt{};
        opt.count_deletions = o.coverage_deletions;
        opt.count_secondary = o.coverage_secondary;
        opt.min_mapq = (uint32_t)o.coverage_min_mapq;
        opt.report_zero = o.coverage_zero;
        create(ctxs, flx_coverage_create, opt, "coverage accumulator");
    }
    int add(size_t slot, const flx_run* run, ReadBatch const&) override { return flx_coverage_add_run(objs[slot], run); }
    bool write() override {
        flx_coverage* const cov = total();
        if (!cov) return false;
        auto const& names = ref.ids;
        auto windows_of = [&](uint64_t w, std::vector<flx_depth_window>& out) {
            out.resize(flx_coverage_num_windows(cov, w));
            return flx_coverage_copy_windows(cov, w, out.data(), out.size()) == FLX_OK || failed_call();
        };
        if (!o.coverage.empty()) {
            std::vector<flx_depth_run> runs(flx_coverage_num_runs(cov));
            if (flx_coverage_copy_runs(cov, runs.data(), runs.size()) != FLX_OK) return failed_call();
            if (!write_text(o.coverage, "a coverage output", [&](FILE* f) {
                    for (auto const& r : runs) fprintf(f, "%s\t%llu\t%llu\t%u\n", names[(size_t)r.reference_id].c_str(), u(r.start), u(r.end), r.depth);
                })) return false;
        }
        if (!o.coverage_summary.empty()) {
            std::vector<flx_depth_window> win;
            if (!windows_of(0, win)) return false;
            if (!write_text(o.coverage_summary, "a coverage output", [&](FILE* f) {
                    for (auto const& w : win) fprintf(f, "%s\t%llu\t%llu\t%llu\t%u\n", names[(size_t)w.reference_id].c_str(), u(w.end), u(w.covered), u(w.depth_sum), w.max_depth);
                })) return false;
        }
        if (!o.coverage_windows.empty()) {
            std::vector<flx_depth_window> win;
            if (!windows_of(o.coverage_window, win)) return false;
            if (!write_text(o.coverage_windows, "a coverage output", [&](FILE* f) {
                    for (auto const& w : win)
                        fprintf(f, "%s\t%llu\t%llu\t%llu\t%llu\t%u\n", names[(size_t)w.reference_id].c_str(), u(w.start), u(w.end), u(w.depth_sum), u(w.covered), w.max_depth);
                })) return false;
        }
        return true;
    }
};

// the variant-site table: the sites as text with the reference letter from the sequences read here (ranks 1..4 are ACGT, anything
// else N) and the position 1-based
struct Pileup : PerContext<flx_pileup> {
    Pileup(Options const& o_, std::vector<flx_ctx*> const& ctxs, Reference const& ref_) : PerContext(o_, ref_, flx_pileup_absorb, flx_pileup_finish, flx_pileup_free) {
        flx_pileup_options opt{};
        opt.count_secondary = o.pileup_secondary;
        opt.min_mapq = (uint32_t)o.pileup_min_mapq;
        opt.min_depth = (uint32_t)o.pileup_min_depth;
        opt.min_count = (uint32_t)o.pileup_min_count;
        if (o.pileup_min_fraction > 0) opt.min_permille = (uint32_t)std::max<uint64_t>(1, flx_floating_point_error_aware_ceil(o.pileup_min_fraction * 1000.0));
        create(ctxs, flx_pileup_create, opt, "pileup accumulator");
    }
    int add(size_t slot, const flx_run* run, ReadBatch const& b) override { return flx_pileup_add_run(objs[slot], run, b.pool.data(), b.offsets.data(), b.ids.size()); }
    bool write() override {
        flx_pileup* const pile = total();
        if (!pile) return false;
        std::vector<flx_pileup_site> sites(flx_pileup_num_sites(pile));
        if (flx_pileup_copy_sites(pile, sites.data(), sites.size()) != FLX_OK) return failed_call();
        std::vector<uint64_t> starts(ref.lens.size() + 1, 0);
        for (size_t r = 0; r < ref.lens.size(); ++r) starts[r + 1] = starts[r] + ref.lens[r];
        return write_text(o.pileup, "the pileup output", [&](FILE* f) {
            for (auto const& s : sites) {
                uint8_t const rank = ref.pool[starts[(size_t)s.reference_id] + s.position];
                fprintf(f, "%s\t%llu\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", ref.ids[(size_t)s.reference_id].c_str(), u(s.position) + 1,
                        rank >= 1 && rank <= 4 ? "ACGT"[rank - 1] : 'N', s.depth, s.alt[0], s.alt[1], s.alt[2], s.alt[3], s.del, s.ins);
            }
        });
    }
};

// the structural-variant table: the signatures sorted and clustered in the first object, and the clusters written as text: positions
// 1-based; q is a length for DEL and INS and a 1-based position for BND; sides L / R for BND, . otherwise
struct Sv : PerContext<flx_sv> {
    Sv(Options const& o_, std::vector<flx_ctx*> const& ctxs, Reference const& ref_) : PerContext(o_, ref_, flx_sv_absorb, flx_sv_finish, flx_sv_free) {
        flx_sv_options opt{};
        opt.min_length = (uint32_t)o.sv_min_length;
        opt.max_distance = (uint32_t)o.sv_max_distance;
        opt.min_support = (uint32_t)o.sv_min_support;
        opt.count_secondary = o.sv_secondary;
        opt.min_mapq = (uint32_t)o.sv_min_mapq;
        if (!o.drop_duplicate_alignments)
            log_line("warning", "--sv-signatures counts records, not reads: without -D/--drop-duplicate-alignments a read's records at one locus all add to a cluster's support (use -D -N 1).");
        create(ctxs, flx_sv_create, opt, "sv object");
    }
    int add(size_t slot, const flx_run* run, ReadBatch const& b) override { return flx_sv_add_run(objs[slot], run, b.offsets.data(), b.ids.size()); }
    bool write() override {
        flx_sv* const s = total();
        if (!s) return false;
        std::vector<flx_sv_cluster> clusters(flx_sv_num_clusters(s));
        if (flx_sv_copy_clusters(s, clusters.data(), clusters.size()) != FLX_OK) return failed_call();
        auto const& names = ref.ids;
        return write_text(o.sv, "the sv output", [&](FILE* f) {
            static const char* const types[3] = {"DEL", "INS", "BND"};
            for (auto const& c : clusters) {
                bool const bnd = c.type == 2;
                unsigned long long const one = bnd ? 1 : 0;
                fprintf(f, "%s\t%s\t%llu\t%llu\t%c\t%s\t%llu\t%llu\t%llu\t%c\t%u\n", types[c.type], names[(size_t)c.ref_a].c_str(), u(c.pos_a_min) + 1, u(c.pos_a_max) + 1,
                        bnd ? "LR"[c.side_a] : '.', names[(size_t)c.ref_b].c_str(), c.q_min + one, c.q_median + one, c.q_max + one, bnd ? "LR"[c.side_b] : '.', c.support);
            }
        });
    }
};

// the error profile: one line per counter in the table's fixed order (section, keys, count; zero counters too, so the file's shape
// never changes), then the summary lines. Letters: . for rank 0, then A C G T N.
struct ErrorProfile : PerContext<flx_errprof> {
    ErrorProfile(Options const& o_, std::vector<flx_ctx*> const& ctxs, Reference const& ref_) : PerContext(o_, ref_, flx_errprof_absorb, nullptr, flx_errprof_free) {
        flx_errprof_options opt{};
        opt.count_secondary = o.error_profile_secondary;
        opt.min_mapq = (uint32_t)o.error_profile_min_mapq;
        if (!o.drop_duplicate_alignments)
            log_line("warning", "--error-profile counts records, not reads: without -D/--drop-duplicate-alignments a read's records at one locus all add their columns (use -D -N 1).");
        create(ctxs, flx_errprof_create, opt, "error-profile object");
    }
    int add(size_t slot, const flx_run* run, ReadBatch const& b) override { return flx_errprof_add_run(objs[slot], run, b.pool.data(), b.offsets.data(), b.ids.size()); }
    bool write() override {
        flx_errprof* const prof = total();
        if (!prof) return false;
        flx_errprof_table t;
        if (flx_errprof_copy(prof, &t) != FLX_OK) return failed_call();
        uint64_t unequal = 0;
        for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) if (a != b) unequal += t.pair_eq[a * 6 + b];
        if (!write_text(o.error_profile, "the error-profile output", [&](FILE* f) { print(f, t, unequal); })) return false;
        if (unequal) log_line("warning", "--error-profile: %llu columns of = words hold unequal letters (eq_columns_unequal): the records do not fit the reference or the reads", u(unequal));
        return true;
    }
    static void print(FILE* f, flx_errprof_table const& t, uint64_t unequal) {
        static const char letter[6] = {'.', 'A', 'C', 'G', 'T', 'N'};
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
        fprintf(f, "summary\tcolumns\t%llu\nsummary\terror_rate_ppm\t%llu\nsummary\tmismatch_ppm\t%llu\nsummary\tinsertion_ppm\t%llu\nsummary\tdeletion_ppm\t%llu\nsummary\teq_columns_unequal\t%llu\n",
                u(columns), ppm(mismatches + ins + del), ppm(mismatches), ppm(ins), ppm(del), u(unequal));
    }
};

template <class S>
bool put(std::vector<std::unique_ptr<SideOutput>>& list, Options const& o, std::vector<flx_ctx*> const& ctxs, Reference const& ref) {
    auto s = std::make_unique<S>(o, ctxs, ref);
    bool const ready = s->ready;
    list.push_back(std::move(s));
    return ready;
}

}  // namespace

bool make_side_outputs(Options const& o, std::vector<flx_ctx*> const& ctxs, Reference const& ref, std::vector<std::unique_ptr<SideOutput>>& list) {
    return (!o.wants_coverage() || put<Coverage>(list, o, ctxs, ref)) && (o.pileup.empty() || put<Pileup>(list, o, ctxs, ref)) &&
           (o.sv.empty() || put<Sv>(list, o, ctxs, ref)) && (o.error_profile.empty() || put<ErrorProfile>(list, o, ctxs, ref));
}
