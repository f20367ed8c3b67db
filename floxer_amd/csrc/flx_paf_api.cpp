// flx_paf and flx_paf_writer: the objects behind the PAF calls of the C ABI (include/floxer_amd.h). The rule and its checks: flx_paf.hpp;
// the kernel: flx_paf.hip. A flx_paf owns one stream and three grow-only device buffers (jobs, words, summaries). A call judges its
// records without the object's lock (that is the host rule itself, into a buffer of the call's own) and takes the lock for upload, launch
// and download, so calls from several host threads are serialised there. A large call is judged on up to eight threads of its own. With
// device -1 nothing of the device exists and the judged summaries are the result. The writer is host code: it formats a call in full,
// then writes it. What flx_paf shares with the other side objects: flx_object.hpp.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>

#include "flx_object.hpp"
#include "flx_paf.hpp"

using namespace flx;

struct flx_paf : SideObject {            // mu: the buffers and the launches; FLX_PAF_PROFILE
    DeviceBuffer jobs, words, out;       // a call's staging: one PafJob per record, the stretch of the pool in use, the summaries
};

struct flx_paf_writer {
    FILE* f = nullptr;
    flx_paf_options opt{};
    std::vector<std::string> ref_ids;
    std::vector<u64> ref_lens;
    bool failed = false;
};

namespace {

// the buffer holds at least `bytes` afterwards; a failure leaves it as it was (contents are not preserved by a growth)
int grow(DeviceBuffer& b, size_t bytes) {
    if (b.ptr && bytes <= b.cap) return FLX_OK;
    DeviceBuffer fresh;
    int const rc = fresh.ensure(bytes);
    if (rc) return rc;
    b.take(fresh);
    return FLX_OK;
}

bool arguments_given(const flx_record* records, uint64_t n, const uint64_t* ref_lens, uint32_t n_refs, flx_paf_summary* out, const char* who) {
    if ((n && (!records || !out)) || (n_refs && !ref_lens)) { set_error(std::string(who) + ": null argument"); return false; }
    return true;
}

// Every record judged into `judged` (the host rule itself), on up to eight threads when the call has at least half a million words per
// thread; the first refusal in record order is the one reported.
bool judge_all(const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words, const uint64_t* read_offsets, uint64_t n_reads,
               const uint64_t* ref_lens, uint32_t n_refs, const char* who, flx_paf_summary* judged) {
    u64 words = 0;
    for (uint64_t i = 0; i < n; ++i) words += records[i].cigar_length;
    size_t const n_threads = (size_t)std::max<u64>(1, std::min<u64>({8, words >> 19, n}));
    return judge_in_parallel(n_threads, [&](size_t t) {
        return paf_plan(records, n * t / n_threads, n * (t + 1) / n_threads, cigar_words, n_words, read_offsets, n_reads, ref_lens, n_refs, who, judged);
    });
}

void append_number(std::string& s, u64 v) {
    char num[24];
    char* const e = num + sizeof(num);
    char* p = e;
    do { *--p = (char)('0' + v % 10); v /= 10; } while (v);
    s.append(p, (size_t)(e - p));
}

}  // namespace

extern "C" int flx_paf_create(int hip_device, flx_paf** out) {
    if (!out) { set_error("flx_paf_create: null argument"); return FLX_ERR_INVALID; }
    if (hip_device < -1) { set_error("flx_paf_create: the device is -1 (the host) or a HIP device"); return FLX_ERR_INVALID; }
    auto p = std::make_unique<flx_paf>();            // (an error below drops it: nothing stays allocated)
    int const rc = p->open(hip_device, "FLX_PAF_PROFILE");
    if (rc) return rc;
    *out = p.release();
    return FLX_OK;
}
extern "C" void flx_paf_free(flx_paf* p) { free_object(p); }

extern "C" int flx_paf_summarize_host(const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words, const uint64_t* read_offsets,
                                      uint64_t n_reads, const uint64_t* ref_lens, uint32_t n_refs, flx_paf_summary* out) {
    if (!arguments_given(records, n, ref_lens, n_refs, out, "flx_paf_summarize_host")) return FLX_ERR_INVALID;
    if (!paf_lengths_valid(ref_lens, n_refs, "flx_paf_summarize_host")) return FLX_ERR_INVALID;
    std::vector<flx_paf_summary> judged(n);
    if (!judge_all(records, n, cigar_words, n_words, read_offsets, n_reads, ref_lens, n_refs, "flx_paf_summarize_host", judged.data())) return FLX_ERR_INVALID;
    if (n) memcpy(out, judged.data(), n * sizeof(flx_paf_summary));
    return FLX_OK;
}

extern "C" int flx_paf_summarize(flx_paf* p, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words, const uint64_t* read_offsets,
                                 uint64_t n_reads, const uint64_t* ref_lens, uint32_t n_refs, flx_paf_summary* out) {
    if (!p) { set_error("flx_paf_summarize: null argument"); return FLX_ERR_INVALID; }
    if (!arguments_given(records, n, ref_lens, n_refs, out, "flx_paf_summarize")) return FLX_ERR_INVALID;
    if (!paf_lengths_valid(ref_lens, n_refs, "flx_paf_summarize")) return FLX_ERR_INVALID;
    if (n >= (1ull << 32)) { set_error("flx_paf_summarize: too many records in one call"); return FLX_ERR_INVALID; }
    auto const t0 = std::chrono::steady_clock::now();
    std::vector<flx_paf_summary> judged(n);
    if (!judge_all(records, n, cigar_words, n_words, read_offsets, n_reads, ref_lens, n_refs, "flx_paf_summarize", judged.data())) return FLX_ERR_INVALID;
    if (n == 0) return FLX_OK;
    if (p->device < 0) { memcpy(out, judged.data(), n * sizeof(flx_paf_summary)); return FLX_OK; }
    // one job per record and the stretch of the pool the mapped records use: [lo, hi)
    u64 lo = n_words, hi = 0;
    for (uint64_t i = 0; i < n; ++i)
        if (paf_record_mapped(records[i])) { lo = std::min<u64>(lo, records[i].cigar_offset); hi = std::max<u64>(hi, records[i].cigar_offset + records[i].cigar_length); }
    if (hi < lo) lo = hi = 0;                          // (no mapped record)
    std::vector<PafJob> jobs(n);
    for (uint64_t i = 0; i < n; ++i) {
        flx_record const& r = records[i];
        if (!paf_record_mapped(r)) { jobs[i] = PafJob{0, 0, 0, 0, 0}; continue; }
        jobs[i] = PafJob{r.cigar_offset - lo, r.cigar_length, (u32)(read_offsets[r.read_index + 1] - read_offsets[r.read_index]), (u32)r.position, (r.flag & 16u) ? 1u : 0u};
    }
    std::lock_guard<std::mutex> g(p->mu);
    FLX_HIP(hipSetDevice(p->device));
    int rc;
    if ((rc = grow(p->jobs, n * sizeof(PafJob))) || (rc = grow(p->words, (hi - lo) * 4 + 4)) || (rc = grow(p->out, n * sizeof(flx_paf_summary)))) return rc;
    FLX_HIP(hipMemcpyAsync(p->jobs.ptr, jobs.data(), n * sizeof(PafJob), hipMemcpyHostToDevice, p->stream));
    if (hi > lo) FLX_HIP(hipMemcpyAsync(p->words.ptr, cigar_words + lo, (hi - lo) * 4, hipMemcpyHostToDevice, p->stream));
    if ((rc = p->span_begin())) return rc;
    FLX_LAUNCH("paf_summarise", PafDevice::summarise(p->stream, p->jobs.as<PafJob>(), (u32)n, p->words.as<u32>(), p->out.as<flx_paf_summary>()));
    if ((rc = p->span_end())) return rc;
    FLX_HIP(hipMemcpyAsync(out, p->out.ptr, n * sizeof(flx_paf_summary), hipMemcpyDeviceToHost, p->stream));
    FLX_HIP(hipStreamSynchronize(p->stream));          // (the staging buffers are free for the next call)
    if (p->profile) {
        float ms;
        if ((rc = p->span_ms(ms))) return rc;
        double const wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[flx paf] summarize: records %llu words %llu upload_bytes %llu paf_summarise_ms %.3f wall_ms %.3f\n", (unsigned long long)n,
                (unsigned long long)(hi - lo), (unsigned long long)(n * sizeof(PafJob) + (hi - lo) * 4), (double)ms, wall);
    }
    for (uint64_t i = 0; i < n; ++i)
        if (paf_summary_is_violation(out[i])) { set_error("flx_paf_summarize: the kernel met a record that breaks the rule the host judged it by (record " + std::to_string(i) + ")"); return FLX_ERR_INTERNAL; }
    return FLX_OK;
}

extern "C" int flx_paf_open(const char* path, const char* const* ref_ids, const uint64_t* ref_lens, uint32_t n_refs, const flx_paf_options* o, flx_paf_writer** out) {
    if (!path || !out || (n_refs && (!ref_ids || !ref_lens))) { set_error("flx_paf_open: null argument"); return FLX_ERR_INVALID; }
    if (!paf_options_valid(o)) return FLX_ERR_INVALID;
    auto w = std::make_unique<flx_paf_writer>();
    if (o) w->opt = *o;
    for (uint32_t r = 0; r < n_refs; ++r) {
        if (!ref_ids[r]) { set_error("flx_paf_open: null argument"); return FLX_ERR_INVALID; }
        w->ref_ids.emplace_back(ref_ids[r]);
        w->ref_lens.push_back(ref_lens[r]);
    }
    w->f = fopen(path, "wb");
    if (!w->f) { set_error(std::string("cannot open output file: ") + path); return FLX_ERR_IO; }
    *out = w.release();
    return FLX_OK;
}

extern "C" int flx_paf_write(flx_paf_writer* w, const char* const* read_ids, const uint64_t* read_offsets, const flx_record* records, uint64_t n,
                             const uint32_t* cigar_words, const flx_paf_summary* summaries, const int32_t* scores, const flx_md_ref* cs_refs,
                             const uint8_t* cs_bytes) {
    if (!w || (n && (!read_ids || !read_offsets || !records || !summaries))) { set_error("flx_paf_write: null argument"); return FLX_ERR_INVALID; }
    if (w->failed) { set_error("write error on the PAF output"); return FLX_ERR_IO; }
    static const char ops[] = "MIDNSHP=X";
    static const struct Table { bool ok[256]; Table() { for (int c = 0; c < 256; ++c) ok[c] = (c >= '0' && c <= '9') || (c != 0 && strchr(":*+=-acgtnACGTN", c) != nullptr); } } table;
    std::string text;
    for (uint64_t i = 0; i < n; ++i) {
        flx_record const& r = records[i];
        const char* const id = read_ids[r.read_index];
        u64 const qlen = read_offsets[r.read_index + 1] - read_offsets[r.read_index];
        if (!paf_record_mapped(r)) {
            if (!w->opt.write_unmapped) continue;
            text += id; text += '\t'; append_number(text, qlen);
            text += "\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0\n";
            continue;
        }
        if ((r.flag & 256u) && w->opt.skip_secondary) continue;
        flx_paf_summary const& s = summaries[i];
        auto refuse = [&](const char* what) { set_error(std::string("flx_paf_write: ") + what + " in record " + std::to_string(i) + " (read " + id + ")"); return FLX_ERR_INVALID; };
        if (paf_summary_is_violation(s)) return refuse("a summary the kernel could not make");
        if ((size_t)r.reference_id >= w->ref_ids.size() || r.position < 0) return refuse("a reference or position outside the references");
        if (w->opt.mapq_from_records && r.reserved > 254u) return refuse("mapping quality above 254");
        u64 const num = (u64)s.mismatches + s.gap_opens, den = (u64)s.matches + num;
        if (den == 0) return refuse("a summary without columns");
        if (w->opt.write_cigar && r.cigar_length && !cigar_words) return refuse("CIGAR words missing");
        text += id; text += '\t'; append_number(text, qlen);
        text += '\t'; append_number(text, s.query_start);
        text += '\t'; append_number(text, s.query_end);
        text += (r.flag & 16u) ? "\t-\t" : "\t+\t";
        text += w->ref_ids[(size_t)r.reference_id];
        text += '\t'; append_number(text, w->ref_lens[(size_t)r.reference_id]);
        text += '\t'; append_number(text, (u64)r.position);
        text += '\t'; append_number(text, s.ref_end);
        text += '\t'; append_number(text, s.matches);
        text += '\t'; append_number(text, (u64)s.matches + s.mismatches + s.ins_bases + s.del_bases);
        text += '\t'; append_number(text, w->opt.mapq_from_records ? r.reserved : 255u);
        text += (r.flag & 256u) ? "\ttp:A:S" : "\ttp:A:P";
        text += "\tNM:i:"; append_number(text, r.num_errors);
        if (scores) {
            text += "\tAS:i:";
            if (scores[i] < 0) text += '-';
            append_number(text, scores[i] < 0 ? 0ull - (u64)(int64_t)scores[i] : (u64)scores[i]);
        }
        u64 const t = paf_divergence_e4(num, den);
        char frac[8];
        snprintf(frac, sizeof(frac), "%04u", (unsigned)(t % 10000));
        text += "\tde:f:"; append_number(text, t / 10000); text += '.'; text += frac;
        if (w->opt.write_cigar) {
            text += "\tcg:Z:";
            for (uint32_t c = 0; c < r.cigar_length; ++c) {
                uint32_t const word = cigar_words[r.cigar_offset + c];
                if ((word & 15u) > 8u) return refuse("a CIGAR op outside MIDNSHP=X");
                append_number(text, word >> 4);
                text += ops[word & 15u];
            }
        }
        if (cs_refs && cs_refs[i].length) {
            if (!cs_bytes) return refuse("cs references without cs bytes");
            const uint8_t* const cs = cs_bytes + cs_refs[i].offset;
            for (uint32_t b = 0; b < cs_refs[i].length; ++b)
                if (!table.ok[cs[b]]) return refuse("a cs string with a byte outside [0-9:*+=acgtnACGTN-]");
            text += "\tcs:Z:";
            text.append((const char*)cs, cs_refs[i].length);
        }
        text += '\n';
    }
    if (!text.empty() && fwrite(text.data(), 1, text.size(), w->f) != text.size()) { w->failed = true; set_error("write error on the PAF output"); return FLX_ERR_IO; }
    return FLX_OK;
}

extern "C" int flx_paf_close(flx_paf_writer* w) {
    if (!w) return FLX_OK;
    bool const ok = fclose(w->f) == 0 && !w->failed;
    delete w;
    if (!ok) { set_error("write error while closing the PAF output"); return FLX_ERR_IO; }
    return FLX_OK;
}
