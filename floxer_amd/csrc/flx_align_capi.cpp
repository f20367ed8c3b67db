// The C ABI of alignment job batches (seam 2): flx_align_shapes, the flx_align_batch chain, and the entry points of a kernel alone
// (extension, tails, left-align, realign, cs) over jobs made by the caller.
#include <algorithm>
#include <cstring>
#include <string>

#include "flx_partial.hpp"
#include "flx_tails.hpp"
#include "flx_leftalign.hpp"
#include "flx_cs.hpp"
#include "flx_traceback.hpp"
#include "flx_realign.hpp"
#include "flx_paf.hpp"
#include "flx_coverage.hpp"
#include "flx_pileup.hpp"
#include "flx_sort.hpp"
#include "flx_sv.hpp"
#include "flx_errprof.hpp"

using namespace flx;

// ================================================================================================ C ABI: seam 2
// The jobs of one flx_align_batch call as the three request lists it runs, by mode (ids: the job of every request). WITHOUT_CIGAR jobs
// run on the reversed pools: their offsets are mirrored in text_len / query_pool_len.
struct BatchRequests { hvec<AlignRequest> reqs[3]; hvec<u32> ids[3]; };
static void split_batch_jobs(const flx_align_job* jobs, uint64_t n_jobs, u64 text_len, u64 query_pool_len, BatchRequests& B) {
    for (uint64_t i = 0; i < n_jobs; ++i) {
        flx_align_job const& j = jobs[i];
        if (j.mode == FLX_MODE_WITHOUT_CIGAR) B.reqs[j.mode].push_back({text_len - j.ref_offset - j.ref_length, query_pool_len - j.query_offset - j.query_length, j.ref_length, j.query_length, j.num_allowed_errors});
        else B.reqs[j.mode].push_back({j.ref_offset, j.query_offset, j.ref_length, j.query_length, j.num_allowed_errors});
        B.ids[j.mode].push_back((u32)i);
    }
}

// The launch shape flx_align_batch gives every job: the same three lists, their distinct requests (run_deduplicated) and choose_shapes on
// each. queue: the hand-over slots the job's own ring occupies in that shape (0: it never waits; more than RING_QUEUE_MAX would mean a
// shape that does not hold the job). Host arithmetic only: no context, no device.
extern "C" int flx_align_shapes(const flx_align_job* jobs, uint64_t n_jobs, flx_align_shape* out) {
    if (n_jobs && (!jobs || !out)) { set_error("flx_align_shapes: null argument"); return FLX_ERR_INVALID; }
    if (n_jobs >= (1ull << 31)) { set_error("too many jobs in one call"); return FLX_ERR_INVALID; }
    u64 text_len = 0, query_pool_len = 0;                 // (any pool that holds every job mirrors the offsets one to one)
    for (uint64_t i = 0; i < n_jobs; ++i) {
        flx_align_job const& j = jobs[i];
        if (j.query_length == 0 || j.mode > 2) { set_error("flx_align_shapes: job without query rows, or of an unknown mode"); return FLX_ERR_INVALID; }
        if (j.query_length > align_supported_max_query()) { set_error("query longer than the supported maximum"); return FLX_ERR_UNSUPPORTED; }
        text_len = std::max<u64>(text_len, j.ref_offset + j.ref_length);
        query_pool_len = std::max<u64>(query_pool_len, j.query_offset + j.query_length);
    }
    BatchRequests B;
    split_batch_jobs(jobs, n_jobs, text_len, query_pool_len, B);
    for (int mode = 0; mode < 3; ++mode) {
        hvec<AlignRequest> uniq;
        hvec<u32> uniq_of;
        hvec<AlignShape> shapes;
        dedup_requests(B.reqs[mode], uniq, uniq_of);
        if (int const rc = choose_shapes(uniq, shapes)) return rc;
        for (size_t i = 0; i < B.reqs[mode].size(); ++i) {
            AlignRequest const& r = B.reqs[mode][i];
            AlignShape const sh = shapes[uniq_of[i]];
            out[B.ids[mode][i]] = flx_align_shape{sh.words_per_lane, sh.lanes_per_job, ring_queue_for(ring_delay(r.n, r.m, r.k, sh.words_per_lane, sh.lanes_per_job))};
        }
    }
    return FLX_OK;
}

extern "C" int flx_align_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool,
                               uint64_t query_pool_len, const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out,
                               uint32_t* cigar_pool, uint64_t* cigar_pool_words) {
    return flx_align_batch_gaps(ctx, ref_pool, ref_pool_len, query_pool, query_pool_len, jobs, n_jobs, out, cigar_pool, cigar_pool_words, nullptr, nullptr, nullptr, nullptr);
}
extern "C" int flx_align_batch_md(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool,
                                  uint64_t query_pool_len, const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out,
                                  uint32_t* cigar_pool, uint64_t* cigar_pool_words, flx_md_ref* out_md, uint8_t* md_pool, uint64_t* md_pool_bytes) {
    return flx_align_batch_gaps(ctx, ref_pool, ref_pool_len, query_pool, query_pool_len, jobs, n_jobs, out, cigar_pool, cigar_pool_words, out_md, md_pool, md_pool_bytes, nullptr);
}
extern "C" int flx_align_batch_gaps(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool,
                                    uint64_t query_pool_len, const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out,
                                    uint32_t* cigar_pool, uint64_t* cigar_pool_words, flx_md_ref* out_md, uint8_t* md_pool, uint64_t* md_pool_bytes,
                                    const flx_gap_options* gaps) {
    return flx_align_batch_realign(ctx, ref_pool, ref_pool_len, query_pool, query_pool_len, jobs, n_jobs, out, cigar_pool, cigar_pool_words, out_md, md_pool,
                                   md_pool_bytes, gaps, nullptr, nullptr);
}
// out_md == NULL: no MD strings (flx_align_batch); gaps NULL or zeroed: the gaps stay where K5 put them (flx_align_batch_md); realign
// NULL or zeroed: the paths stay edit-distance paths (flx_align_batch_gaps)
extern "C" int flx_align_batch_realign(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool,
                                       uint64_t query_pool_len, const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out,
                                       uint32_t* cigar_pool, uint64_t* cigar_pool_words, flx_md_ref* out_md, uint8_t* md_pool, uint64_t* md_pool_bytes,
                                       const flx_gap_options* gaps, const flx_realign_options* realign, int32_t* out_scores) {
    return flx_align_batch_cs(ctx, ref_pool, ref_pool_len, query_pool, query_pool_len, jobs, n_jobs, out, cigar_pool, cigar_pool_words, out_md, md_pool, md_pool_bytes,
                              gaps, realign, out_scores, nullptr, nullptr, nullptr, nullptr);
}
// cs NULL or zeroed: no cs strings (flx_align_batch_realign)
extern "C" int flx_align_batch_cs(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool,
                                  uint64_t query_pool_len, const flx_align_job* jobs, uint64_t n_jobs, flx_align_result* out,
                                  uint32_t* cigar_pool, uint64_t* cigar_pool_words, flx_md_ref* out_md, uint8_t* md_pool, uint64_t* md_pool_bytes,
                                  const flx_gap_options* gaps, const flx_realign_options* realign, int32_t* out_scores, const flx_cs_options* cs,
                                  flx_md_ref* out_cs, uint8_t* cs_pool, uint64_t* cs_pool_bytes) {
    if (!cs_options_valid(cs)) return FLX_ERR_INVALID;                                 // (before the context is looked at)
    uint32_t const cs_form = cs_options_form(cs);
    std::string const fn = cs_form ? "flx_align_batch_cs" : realign_options_active(realign) ? "flx_align_batch_realign" : gap_options_active(gaps) ? "flx_align_batch_gaps" : out_md ? "flx_align_batch_md" : "flx_align_batch";        // (all forward here)
    if (!gap_options_valid(gaps) || !realign_options_valid(realign)) return FLX_ERR_INVALID;
    RealignScores const ra_scores = realign_scores(realign);
    if (cs_form && (!out_cs || !cs_pool_bytes)) { set_error(fn + ": null argument"); return FLX_ERR_INVALID; }
    uint64_t const cs_pool_cap = cs_pool_bytes ? *cs_pool_bytes : 0;
    if (cs_pool_bytes) *cs_pool_bytes = 0;                                            // (out: bytes used, also on an early return)
    if (out_md && !md_pool_bytes) { set_error(fn + ": null argument"); return FLX_ERR_INVALID; }
    uint64_t const md_pool_cap = md_pool_bytes ? *md_pool_bytes : 0;
    if (md_pool_bytes) *md_pool_bytes = 0;                                            // (out: bytes used, also on an early return)
    if (!ctx || (n_jobs && (!jobs || !out || !query_pool))) { set_error(fn + ": null argument"); return FLX_ERR_INVALID; }
    FLX_HIP(hipSetDevice(ctx->device));
    if (n_jobs >= (1ull << 31)) { set_error("too many jobs in one call"); return FLX_ERR_INVALID; }
    u64 const text_len = ref_pool ? ref_pool_len : ctx->hidx->n;
    bool any_rev = false, any_trace = false;
    for (uint64_t i = 0; i < n_jobs; ++i) {
        flx_align_job const& j = jobs[i];
        if (j.query_length == 0 || j.query_offset + j.query_length > query_pool_len || j.ref_offset + j.ref_length > text_len || j.mode > 2) {
            set_error(fn + ": job outside its pools"); return FLX_ERR_INVALID;
        }
        if (j.query_length > align_supported_max_query()) { set_error("query longer than the supported maximum"); return FLX_ERR_UNSUPPORTED; }
        any_rev |= j.mode == FLX_MODE_WITHOUT_CIGAR;
        any_trace |= j.mode == FLX_MODE_WITH_CIGAR;
    }
    int rc;
    LaneLease lease(ctx, ctx->external_stream ? 0 : -1);
    Lane* L = lease.lane;
    const u8* d_text = ctx->didx.text;
    const u8* d_text_rev = nullptr;
    hvec<u8> tmp;
    if (ref_pool) {
        if ((rc = upload_padded(L, L->user_text, ref_pool, ref_pool_len, &d_text))) return rc;
        if (any_rev) {
            tmp.assign(ref_pool, ref_pool + ref_pool_len);
            std::reverse(tmp.begin(), tmp.end());
            if ((rc = upload_padded(L, L->user_text_rev, tmp.data(), tmp.size(), &d_text_rev))) return rc;
            if ((rc = L->sync())) return rc;
        }
    } else if (any_rev) {
        if ((rc = ensure_reversed_text(L))) return rc;
        d_text_rev = ctx->text_rev.as<u8>() + TEXT_PAD;
    }
    if ((rc = h2d(L, L->seq, query_pool, query_pool_len, 192))) return rc;
    if ((rc = build_peq(L, L->seq.as<u8>(), query_pool_len, L->peq))) return rc;
    hvec<u8> qrev;
    if (any_rev) {
        qrev.assign(query_pool, query_pool + query_pool_len);
        std::reverse(qrev.begin(), qrev.end());
        if ((rc = h2d(L, L->seq_rev, qrev.data(), qrev.size(), 64))) return rc;
        if ((rc = build_peq(L, L->seq_rev.as<u8>(), query_pool_len, L->peq_rev))) return rc;
    }
    BatchRequests B;
    split_batch_jobs(jobs, n_jobs, text_len, query_pool_len, B);
    hvec<AlignRequest> const &score_reqs = B.reqs[FLX_MODE_EXISTS], &rev_reqs = B.reqs[FLX_MODE_WITHOUT_CIGAR], &trace_reqs = B.reqs[FLX_MODE_WITH_CIGAR];
    hvec<u32> const &score_ids = B.ids[FLX_MODE_EXISTS], &rev_ids = B.ids[FLX_MODE_WITHOUT_CIGAR], &trace_ids = B.ids[FLX_MODE_WITH_CIGAR];
    for (uint64_t i = 0; i < n_jobs; ++i) out[i] = flx_align_result{0, 0, 0, 0, 0, 0};
    if (out_md) for (uint64_t i = 0; i < n_jobs; ++i) out_md[i] = flx_md_ref{0, 0, 0};
    if (out_scores) for (uint64_t i = 0; i < n_jobs; ++i) out_scores[i] = 0;
    if (cs_form) for (uint64_t i = 0; i < n_jobs; ++i) out_cs[i] = flx_md_ref{0, 0, 0};
    hvec<DevAlignOut> outs;
    if ((rc = run_score_jobs(L, d_text, L->peq.as<u64>(), score_reqs, outs, "ed_align_exists"))) return rc;
    for (size_t i = 0; i < outs.size(); ++i)
        if (outs[i].score != 0xFFFFFFFFu) { out[score_ids[i]].exists = 1; out[score_ids[i]].num_errors = outs[i].score; }
    if ((rc = run_score_jobs(L, d_text_rev, L->peq_rev.as<u64>(), rev_reqs, outs, "ed_align_exists"))) return rc;
    for (size_t i = 0; i < outs.size(); ++i)
        if (outs[i].score != 0xFFFFFFFFu) {
            flx_align_result& r = out[rev_ids[i]];
            r.exists = 1; r.num_errors = outs[i].score; r.begin = rev_reqs[i].n - outs[i].end_col;      // alignment.cpp:135
        }
    hvec<TraceResult> tres;
    hvec<u32> cig;
    hvec<u8> mdp, csp;
    TraceWants wants;
    wants.md_pool = out_md ? &mdp : nullptr;
    wants.left_align = gap_options_active(gaps);
    wants.realign = realign_options_active(realign) ? &ra_scores : nullptr;      // (the scores have their defaults also when the option is off)
    wants.cs_form = cs_form;
    wants.cs_pool = &csp;
    wants.d_query = L->seq.as<u8>();
    if ((rc = run_trace_jobs(L, d_text, L->peq.as<u64>(), trace_reqs, tres, cig, wants))) return rc;
    uint64_t const cap = cigar_pool_words ? *cigar_pool_words : 0;
    if (cigar_pool_words) *cigar_pool_words = cig.size();
    if (any_trace && (!cigar_pool || cig.size() > cap)) { set_error("cigar pool too small"); return FLX_ERR_CAPACITY; }
    if (!cig.empty()) memcpy(cigar_pool, cig.data(), cig.size() * 4);
    if (out_md) {
        *md_pool_bytes = mdp.size();
        if (!mdp.empty() && (!md_pool || mdp.size() > md_pool_cap)) { set_error("md pool too small"); return FLX_ERR_CAPACITY; }
        if (!mdp.empty()) memcpy(md_pool, mdp.data(), mdp.size());
    }
    if (cs_form) {
        *cs_pool_bytes = csp.size();
        if (!csp.empty() && (!cs_pool || csp.size() > cs_pool_cap)) { set_error("cs pool too small"); return FLX_ERR_CAPACITY; }
        if (!csp.empty()) memcpy(cs_pool, csp.data(), csp.size());
    }
    for (size_t i = 0; i < tres.size(); ++i)
        if (tres[i].exists) {
            flx_align_result& r = out[trace_ids[i]];
            r.exists = 1; r.num_errors = tres[i].nm; r.begin = tres[i].begin; r.cigar_offset = tres[i].cigar_off; r.cigar_length = tres[i].cigar_len;
            if (out_md) out_md[trace_ids[i]] = flx_md_ref{tres[i].md_off, tres[i].md_len, 0};
            if (out_scores) out_scores[trace_ids[i]] = tres[i].score;
            if (cs_form) out_cs[trace_ids[i]] = flx_md_ref{tres[i].cs_off, tres[i].cs_len, 0};
        }
    return FLX_OK;
}

// ================================================================================================ C ABI: the extension kernel alone
extern "C" int flx_extend_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                                const flx_extend_job* jobs, uint64_t n_jobs, flx_extend_result* out) {
    if (!ctx || (n_jobs && (!jobs || !out || !query_pool))) { set_error("flx_extend_batch: null argument"); return FLX_ERR_INVALID; }
    if (n_jobs >= (1ull << 31)) { set_error("too many jobs in one call"); return FLX_ERR_INVALID; }
    u64 const text_len = ref_pool ? ref_pool_len : ctx->hidx->n;
    hvec<DevExtendJob> dj(n_jobs);
    for (uint64_t i = 0; i < n_jobs; ++i) {
        flx_extend_job const& j = jobs[i];
        flx_extend_options const as_options{0, j.error_weight, j.x_drop, j.max_errors, {}};
        if (!extend_options_valid(&as_options)) return FLX_ERR_INVALID;
        if (j.direction != 1 && j.direction != -1) { set_error("flx_extend_batch: direction must be +1 or -1"); return FLX_ERR_INVALID; }
        if (j.row_limit > EXTEND_MAX_ROWS || j.ref_limit >= (1u << 31)) { set_error("flx_extend_batch: row_limit must be below 2^19 and ref_limit below 2^31"); return FLX_ERR_INVALID; }
        bool const inside = j.direction > 0 ? (j.text_pos <= text_len && j.ref_limit <= text_len - j.text_pos && j.q_pos <= query_pool_len && j.row_limit <= query_pool_len - j.q_pos)
                                            : ((j.ref_limit == 0 || (j.text_pos < text_len && j.ref_limit <= j.text_pos + 1)) &&
                                               (j.row_limit == 0 || (j.q_pos < query_pool_len && j.row_limit <= j.q_pos + 1)));
        if (!inside) { set_error("flx_extend_batch: job outside its pools"); return FLX_ERR_INVALID; }
        dj[i] = DevExtendJob{j.text_pos, j.q_pos, j.ref_limit, j.row_limit, j.direction, extend_weight(j.error_weight), extend_x_drop(j.x_drop),
                             extend_max_errors(j.max_errors), (u32)i, 0};
        if (j.ref_limit == 0 || j.row_limit == 0) { dj[i].text_pos = 0; dj[i].q_pos = 0; dj[i].ref_limit = 0; }      // nothing is read: R(0) = 0 (row_limit 0), or only D[i][0] = i (ref_limit 0)
    }
    FLX_HIP(hipSetDevice(ctx->device));
    int rc;
    LaneLease lease(ctx, ctx->external_stream ? 0 : -1);
    Lane* L = lease.lane;
    const u8* d_text = ctx->didx.text;
    if (ref_pool && (rc = upload_padded(L, L->user_text, ref_pool, ref_pool_len, &d_text))) return rc;
    if ((rc = h2d(L, L->seq, query_pool, query_pool_len, 192))) return rc;
    hvec<DevExtendOut> outs;
    if ((rc = run_extend_jobs(L, d_text, L->seq.as<u8>(), dj, outs))) return rc;
    for (uint64_t i = 0; i < n_jobs; ++i) out[i] = flx_extend_result{outs[i].rows, outs[i].cols, outs[i].errors, outs[i].reason};
    return FLX_OK;
}

// ================================================================================================ C ABI: the tail kernel alone
extern "C" int flx_cigar_tails_batch(flx_ctx* ctx, const uint32_t* cigar_words, uint64_t n_words, const flx_tail_job* jobs, uint64_t n_jobs, flx_tail_result* out) {
    if (!ctx || (n_jobs && (!jobs || !out)) || (n_words && !cigar_words)) { set_error("flx_cigar_tails_batch: null argument"); return FLX_ERR_INVALID; }
    if (n_jobs >= (1ull << 31)) { set_error("too many jobs in one call"); return FLX_ERR_INVALID; }
    if (!tail_jobs_valid(cigar_words, n_words, jobs, n_jobs, "flx_cigar_tails_batch")) return FLX_ERR_INVALID;      // (before any launch)
    hvec<DevTraceOut> touts(n_jobs);
    TailPass pass;
    for (uint64_t i = 0; i < n_jobs; ++i) {
        flx_tail_job const& j = jobs[i];
        touts[i] = DevTraceOut{0, 0, j.cigar_length, 0};
        pass.add(TailParams{split_weight(j.error_weight), split_x_drop(j.x_drop), split_min_tail_rows(j.min_tail_rows)}, j.cigar_offset, (u32)i);
    }
    FLX_HIP(hipSetDevice(ctx->device));
    LaneLease lease(ctx, ctx->external_stream ? 0 : -1);
    if (int const rc = run_tail_jobs(lease.lane, cigar_words, n_words, touts, pass)) return rc;
    for (uint64_t i = 0; i < n_jobs; ++i) memcpy(&out[i], &pass.outs[i], sizeof(flx_tail_result));
    return FLX_OK;
}

// ================================================================================================ C ABI: left-align, realign, cs alone
// What flx_left_align_batch, flx_realign_batch and flx_cs_batch share (their jobs are one type). The prologue: the argument checks, the
// output capacity in and out, the jobs judged under the caller's name and the DevTraceOuts they describe; then build_jobs (the caller's
// device jobs: host arithmetic, it may refuse); then a lane with the text and the query on it.
namespace {
struct AloneCall {
    uint64_t out_cap = 0;
    hvec<DevTraceOut> touts;
    std::unique_ptr<LaneLease> lease;
    const u8* d_text = nullptr;
    template <class BuildJobs>
    int begin(const char* fn, flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
              const uint32_t* cigar_words, uint64_t n_words, const flx_left_align_job* jobs, uint64_t n_jobs, uint64_t* out_n, const void* out, BuildJobs&& build_jobs) {
        if (!ctx || !out_n || (n_jobs && (!jobs || !out)) || (n_words && !cigar_words) || (query_pool_len && !query_pool)) {
            set_error(std::string(fn) + ": null argument"); return FLX_ERR_INVALID;
        }
        out_cap = *out_n;
        *out_n = 0;
        if (n_jobs >= (1ull << 31)) { set_error("too many jobs in one call"); return FLX_ERR_INVALID; }
        u64 const text_len = ref_pool ? ref_pool_len : ctx->hidx->n;
        if (!left_align_jobs_valid(text_len, query_pool_len, cigar_words, n_words, jobs, n_jobs, fn)) return FLX_ERR_INVALID;      // (before any launch)
        touts.resize(n_jobs);
        for (uint64_t i = 0; i < n_jobs; ++i) touts[i] = DevTraceOut{jobs[i].begin, 0, jobs[i].cigar_length, 0};
        int rc;
        if ((rc = build_jobs())) return rc;
        FLX_HIP(hipSetDevice(ctx->device));
        lease.reset(new LaneLease(ctx, ctx->external_stream ? 0 : -1));
        Lane* const L = lease->lane;
        if (n_jobs) {
            d_text = ctx->didx.text;
            if (ref_pool && (rc = upload_padded(L, L->user_text, ref_pool, ref_pool_len, &d_text))) return rc;
            if ((rc = h2d(L, L->seq, query_pool, query_pool_len, 192))) return rc;
        }
        return FLX_OK;
    }
};
// The epilogue: job i's result, len(i) elements at off(i) of `slabs`, packed into the caller's pool in job order; ref(i, at) tells the
// caller where it went. *out_n: the elements used, also when they do not fit.
template <class T, class Len, class Off, class Ref>
int pack_in_job_order(const char* too_small, uint64_t n_jobs, uint64_t out_cap, uint64_t* out_n, T* out_pool, const T* slabs, Len&& len, Off&& off, Ref&& ref) {
    u64 used = 0;
    for (uint64_t i = 0; i < n_jobs; ++i) used += len(i);
    *out_n = used;
    if (used > out_cap || (used && !out_pool)) { set_error(too_small); return FLX_ERR_CAPACITY; }
    used = 0;
    for (uint64_t i = 0; i < n_jobs; ++i) {
        if (len(i)) memcpy(out_pool + used, slabs + off(i), sizeof(T) * len(i));
        ref(i, used);
        used += len(i);
    }
    return FLX_OK;
}
}  // namespace

extern "C" int flx_left_align_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                                    const uint32_t* cigar_words, uint64_t n_words, const flx_left_align_job* jobs, uint64_t n_jobs, uint32_t* out_words,
                                    uint64_t* out_n_words, flx_cigar_ref* out) {
    AloneCall call;
    LeftAlignPass pass;
    u64 slab_words = 0;
    int rc = call.begin("flx_left_align_batch", ctx, ref_pool, ref_pool_len, query_pool, query_pool_len, cigar_words, n_words, jobs, n_jobs, out_n_words, out, [&] {
        for (uint64_t i = 0; i < n_jobs; ++i) {
            flx_left_align_job const& j = jobs[i];
            u64 const cap = left_align_cap(cigar_words + j.cigar_offset, j.cigar_length);
            pass.jobs.push_back(DevLeftAlignJob{j.ref_offset, j.query_offset, j.cigar_offset, slab_words, j.ref_length, j.query_length, (u32)cap, (u32)i});
            slab_words += cap;
        }
        return FLX_OK;
    });
    if (rc) return rc;
    Lane* const L = call.lease->lane;
    hvec<DevTraceOut>& touts = call.touts;
    hvec<u32> slabs;
    if (n_jobs && (rc = run_left_align_jobs(L, call.d_text, L->seq.as<u8>(), cigar_words, n_words, touts, pass, slab_words, slabs))) return rc;
    return pack_in_job_order("flx_left_align_batch: the output word pool is too small", n_jobs, call.out_cap, out_n_words, out_words, slabs.data(),
                             [&](uint64_t i) { return touts[i].cigar_len; }, [&](uint64_t i) { return pass.jobs[i].out_off + touts[i].cigar_start; },
                             [&](uint64_t i, u64 at) { out[i] = flx_cigar_ref{at, touts[i].cigar_len, 0}; });
}

extern "C" int flx_realign_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                                 const uint32_t* cigar_words, uint64_t n_words, const flx_realign_job* jobs, uint64_t n_jobs,
                                 const flx_realign_options* options, uint32_t* out_words, uint64_t* out_n_words, flx_realign_result* out) {
    if (!realign_options_valid(options)) return FLX_ERR_INVALID;
    RealignScores const scores = realign_scores(options);
    AloneCall call;
    RealignPass pass;
    u64 slab_words = 0;
    int rc = call.begin("flx_realign_batch", ctx, ref_pool, ref_pool_len, query_pool, query_pool_len, cigar_words, n_words, jobs, n_jobs, out_n_words, out, [&] {
        for (uint64_t i = 0; i < n_jobs; ++i) {
            flx_realign_job const& j = jobs[i];
            RealignShape const p = realign_shape(cigar_words + j.cigar_offset, j.cigar_length, scores);
            u64 const cap = realign_cap(p.nm, j.cigar_length, scores);
            u64 const need = realign_trace_words(p.m, (u64)((int64_t)p.d_max - p.d_min + 2 * (int64_t)scores.w + 1));
            if (cap >= (1ull << 32)) { set_error("flx_realign_batch: a job's result could exceed 2^32 words"); return FLX_ERR_INVALID; }
            // (a need beyond 32 bits is beyond every arena: 0 words, the path is kept)
            pass.jobs.push_back(DevRealignJob{j.ref_offset, j.query_offset, j.cigar_offset, slab_words, 0, j.ref_length, j.query_length, (u32)cap, (u32)i,
                                              need > 0xFFFFFFFFull ? 0u : (u32)need, 0});
            slab_words += cap;
        }
        return FLX_OK;
    });
    if (rc) return rc;
    Lane* const L = call.lease->lane;
    hvec<DevTraceOut>& touts = call.touts;
    hvec<u32> slabs;
    if (n_jobs && (rc = run_realign_jobs(L, call.d_text, L->seq.as<u8>(), cigar_words, n_words, touts, pass, scores, slab_words, slabs))) return rc;
    return pack_in_job_order("flx_realign_batch: the output word pool is too small", n_jobs, call.out_cap, out_n_words, out_words, slabs.data(),
                             [&](uint64_t i) { return touts[i].cigar_len; }, [&](uint64_t i) { return pass.jobs[i].out_off + touts[i].cigar_start; },
                             [&](uint64_t i, u64 at) {
                                 DevRealignStat const& s = pass.stats[i];
                                 out[i] = flx_realign_result{at, touts[i].cigar_len, s.num_errors, s.score, s.diag_lo, s.diag_hi, s.kept};
                             });
}

extern "C" int flx_cs_batch(flx_ctx* ctx, const uint8_t* ref_pool, uint64_t ref_pool_len, const uint8_t* query_pool, uint64_t query_pool_len,
                            const uint32_t* cigar_words, uint64_t n_words, const flx_cs_job* jobs, uint64_t n_jobs, const flx_cs_options* options,
                            uint8_t* out_bytes, uint64_t* out_n_bytes, flx_md_ref* out) {
    if (!cs_options_valid(options)) return FLX_ERR_INVALID;
    u32 const form = cs_options_form(options);
    if (form == 0) { set_error("flx_cs_batch: form must be 1 (short) or 2 (long)"); return FLX_ERR_INVALID; }
    AloneCall call;
    CsPass pass;
    int rc = call.begin("flx_cs_batch", ctx, ref_pool, ref_pool_len, query_pool, query_pool_len, cigar_words, n_words, jobs, n_jobs, out_n_bytes, out, [&] {
        for (uint64_t i = 0; i < n_jobs; ++i) {
            flx_cs_job const& j = jobs[i];
            u64 const need = cs_path_bytes(cigar_words + j.cigar_offset, j.cigar_length, form);      // (below 2^30: rows and columns are below 2^28)
            pass.jobs.push_back(DevCsJob{j.ref_offset, j.query_offset, j.cigar_offset, pass.slab_bytes, j.ref_length, j.query_length, (u32)need, (u32)i});
            pass.slab_bytes += need;
        }
        return FLX_OK;
    });
    if (rc) return rc;
    Lane* const L = call.lease->lane;
    hvec<u8> slabs;
    if (n_jobs && (rc = run_cs_jobs(L, call.d_text, L->seq.as<u8>(), cigar_words, n_words, call.touts, pass, form, slabs))) return rc;
    return pack_in_job_order("flx_cs_batch: the output byte pool is too small", n_jobs, call.out_cap, out_n_bytes, out_bytes, slabs.data(),
                             [&](uint64_t i) { return pass.outs[i].len; }, [&](uint64_t i) { return pass.jobs[i].cs_off; },
                             [&](uint64_t i, u64 at) { out[i] = flx_md_ref{at, pass.outs[i].len, 0}; });
}

// ------------------------------------------------------------------------------------------------ grid caps
extern "C" int flx_grid_caps(uint32_t out[16]) {
    if (!out) { set_error("flx_grid_caps: null argument"); return FLX_ERR_INVALID; }
    u32 const caps[16] = {MD_GRID_CAP, CS_GRID_CAP, LEFT_ALIGN_GRID_CAP, TAILS_GRID_CAP, EXTEND_GRID_CAP, REALIGN_GRID_CAP, PAF_GRID_CAP,
                          CoverageDevice::ADD_GRID_CAP, PileupDevice::ADD_GRID_CAP, SvDevice::EXTRACT_GRID_CAP, SortDevice::KEYS_GRID_CAP,
                          ErrprofDevice::ADD_GRID_CAP, SortDevice::CENSUS_GRID_CAP, SortDevice::STRIDED_GRID_CAP, SvDevice::STRIDED_GRID_CAP, 0};
    std::copy(caps, caps + 16, out);
    return FLX_OK;
}
