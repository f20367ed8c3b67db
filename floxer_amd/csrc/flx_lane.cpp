// Device buffers, the lanes of a context (a stream with its own grow-only workspaces) and their synchronisation, host <-> device copies.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "flx_pipeline.hpp"

namespace flx {

int DeviceBuffer::ensure(size_t bytes, bool exact) {
    if (bytes <= cap && ptr) return FLX_OK;
    static int const debug = getenv("FLX_ALLOC_DEBUG") ? 1 : 0;
    if (debug) fprintf(stderr, "[flx alloc] %.3f device buffer grows %zu -> %zu bytes\n", std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count(), cap, bytes);
    release();
    size_t const want = exact ? std::max<size_t>(bytes, 4096) : std::max<size_t>(bytes + bytes / 2, 4096);       // 50 % slack: batches of a run differ by a few per cent
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, want);
    size_t got = want;
    if (e != hipSuccess) { (void)hipGetLastError(); got = bytes; e = hipMalloc(&p, bytes); }   // retry without slack
    if (e != hipSuccess) { set_error(std::string("hipMalloc of ") + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e)); return FLX_ERR_NO_DEVICE; }
    ptr = p;
    cap = got;
    if (debug) fprintf(stderr, "[flx alloc] buffer %p .. %p (%zu bytes, asked %zu)\n", p, (void*)((char*)p + got), got, bytes);
    return FLX_OK;
}
void DeviceBuffer::release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
}

int PinnedBuffer::ensure(size_t bytes) {
    if (bytes <= cap && ptr) return FLX_OK;
    release();
    size_t const want = std::max<size_t>(bytes + bytes / 2, 4096);
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocMapped);
    size_t got = want;
    if (e != hipSuccess) { (void)hipGetLastError(); got = bytes; e = hipHostMalloc(&p, bytes, hipHostMallocMapped); }   // retry without slack
    if (e != hipSuccess) { set_error(std::string("hipHostMalloc of ") + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e)); return FLX_ERR_NO_DEVICE; }
    ptr = p;
    cap = got;
    return FLX_OK;
}
void PinnedBuffer::release() {
    if (ptr) (void)hipHostFree(ptr);
    ptr = nullptr;
    cap = 0;
}

void* Lane::stage_begin(size_t bytes) {
    if (bytes > staging.cap || !staging.ptr) {
        if (wait_idle()) return nullptr;                 // (nothing of this lane reads the old block any more)
        if (staging.ensure(bytes)) return nullptr;
    }
    return staging.ptr;
}
void* Lane::result_slot(size_t bytes) {
    if (!results_limit_read) {
        const char* const env = getenv("FLX_RESULT_BLOCK_BYTES");
        if (env) results_limit = std::min<size_t>(strtoull(env, nullptr, 10), RESULT_BLOCK_BYTES);
        results_limit_read = true;
    }
    if (results_limit == 0) return nullptr;
    if (!results.ptr && results.ensure(results_limit)) { (void)hipGetLastError(); return nullptr; }
    size_t const at = (results_used + 63) & ~(size_t)63;
    if (bytes == 0 || at + bytes > results_limit) return nullptr;      // (the limit, not results.cap: ensure may have allocated slack)
    results_used = at + bytes;
    return (char*)results.ptr + at;
}

hipEvent_t Lane::get_event() {
    if (!event_pool.empty()) { hipEvent_t e = event_pool.back(); event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
// the workspaces of a lane, in the order workspaces() lists them
namespace {
struct Workspace { const char* name; DeviceBuffer Lane::*member; };
#define FLX_WS(m) Workspace{#m, &Lane::m}
constexpr Workspace WORKSPACES[] = {
    FLX_WS(seq), FLX_WS(seq_rev), FLX_WS(peq), FLX_WS(peq_rev), FLX_WS(scheme), FLX_WS(seeds), FLX_WS(stack), FLX_WS(hits), FLX_WS(counters), FLX_WS(rows),
    FLX_WS(rows_out), FLX_WS(jobs), FLX_WS(job_out), FLX_WS(trace), FLX_WS(tjobs), FLX_WS(tjob_out), FLX_WS(cigar), FLX_WS(md), FLX_WS(md_out), FLX_WS(user_text), FLX_WS(user_text_rev),
    FLX_WS(lastrow), FLX_WS(row_windows), FLX_WS(row_out), FLX_WS(seed_cnt), FLX_WS(hit_off), FLX_WS(grouped), FLX_WS(sel_stat), FLX_WS(sel_n), FLX_WS(sel_off),
    FLX_WS(sel_out), FLX_WS(sel_tmp), FLX_WS(sel_rows), FLX_WS(sel_row_off), FLX_WS(sel_sparse), FLX_WS(sel_lists), FLX_WS(vr), FLX_WS(qpack), FLX_WS(items),
    FLX_WS(seed_gen), FLX_WS(mailboxes), FLX_WS(ext_jobs), FLX_WS(ext_out), FLX_WS(tail_jobs), FLX_WS(tail_out), FLX_WS(cigar_la), FLX_WS(la_jobs), FLX_WS(la_stat), FLX_WS(cigar_ra), FLX_WS(ra_jobs), FLX_WS(ra_stat), FLX_WS(cs), FLX_WS(cs_jobs), FLX_WS(cs_out)};
#undef FLX_WS
}  // namespace
std::vector<DeviceBuffer*> Lane::workspaces() {
    std::vector<DeviceBuffer*> v;
    for (Workspace const& w : WORKSPACES) v.push_back(&(this->*w.member));
    return v;
}
void dump_lane_buffers(Lane& l, const char* when) {
    for (Workspace const& w : WORKSPACES) {
        DeviceBuffer const& b = l.*w.member;
        if (b.ptr) fprintf(stderr, "[flx alloc] lane %d %s %s %p .. %p\n", l.id, when, w.name, b.ptr, (void*)((char*)b.ptr + b.cap));
    }
}
int Lane::size_like(Lane& other) {
    auto mine = workspaces(), theirs = other.workspaces();
    for (size_t i = 0; i < mine.size(); ++i)
        if (theirs[i]->cap > mine[i]->cap) {
            // the other lane's capacity already holds the growth slack: take exactly that
            void* p = nullptr;
            if (hipMalloc(&p, theirs[i]->cap) != hipSuccess) { (void)hipGetLastError(); return FLX_OK; }     // best effort
            mine[i]->release();
            mine[i]->ptr = p;
            mine[i]->cap = theirs[i]->cap;
        }
    return FLX_OK;
}
void Lane::release_all() {
    for (DeviceBuffer* b : workspaces()) b->release();
    for (auto& p : pending) { (void)hipEventDestroy(p.start); (void)hipEventDestroy(p.stop); }
    for (auto e : event_pool) (void)hipEventDestroy(e);
    pending.clear();
    event_pool.clear();
    if (own_stream) (void)hipStreamDestroy(own_stream);
    own_stream = stream = nullptr;
    if (vr_host_scalars) { (void)hipHostFree(vr_host_scalars); vr_host_scalars = nullptr; }
    staging.release();
    results.release();
    results_used = 0;
}
int Lane::wait_idle() {
    // hipStreamSynchronize and hipEventSynchronize keep the calling core busy for as long as the GPU works (also with
    // hipEventBlockingSync on this runtime); polling an event with short sleeps leaves the core to the other lanes' host work.
    static int const spin = getenv("FLX_SPIN_SYNC") ? 1 : 0;
    if (spin) { FLX_HIP(hipStreamSynchronize(stream)); return FLX_OK; }
    if (!sync_event) FLX_HIP(hipEventCreateWithFlags(&sync_event, hipEventDisableTiming));
    FLX_HIP(hipEventRecord(sync_event, stream));
    // (the sleeps grow with the time already waited: a long kernel is not polled thousands of times, a short one is not overslept
    // by more than a fifth of its duration)
    static unsigned const max_sleep = getenv("FLX_POLL_MAX_US") ? (unsigned)atoi(getenv("FLX_POLL_MAX_US")) : 1000u;
    for (unsigned sleep_us = 20;;) {
        hipError_t const e = hipEventQuery(sync_event);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) { set_error(std::string("hipEventQuery: ") + hipGetErrorString(e)); return FLX_ERR_NO_DEVICE; }
        std::this_thread::sleep_for(std::chrono::microseconds(sleep_us));
        sleep_us = std::min(max_sleep, sleep_us + sleep_us / 4 + 1);
    }
    return FLX_OK;
}
int Lane::sync() {
    if (int const rc = wait_idle()) return rc;
    if (!pending.empty()) {
        std::lock_guard<std::mutex> g(ctx->mu);
        for (auto& p : pending) {
            ctx->account(p.name.c_str(), p.bytes, p.units, p.start, p.stop);
            event_pool.push_back(p.start);
            event_pool.push_back(p.stop);
        }
        pending.clear();
    }
    return FLX_OK;
}

}  // namespace flx

using namespace flx;

void flx_ctx::account_more(const char* name, u64 bytes, u64 units) {
    if (!timing) return;
    std::lock_guard<std::mutex> g(mu);
    auto it = stats.find(name);
    if (it == stats.end()) return;
    it->second.algorithmic_bytes += bytes;
    it->second.work_units += units;
}
void flx_ctx::account(const char* name, u64 bytes, u64 units, hipEvent_t start, hipEvent_t stop) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, start, stop);
    auto it = stats.find(name);
    if (it == stats.end()) {
        flx_kernel_stat st{};
        strncpy(st.name, name, sizeof(st.name) - 1);
        it = stats.emplace(name, st).first;
        stat_order.push_back(name);
    }
    it->second.launches += 1;
    it->second.device_ms += ms;
    it->second.algorithmic_bytes += bytes;
    it->second.work_units += units;
}
flx::Lane* flx_ctx::acquire_lane(int wanted) {
    std::unique_lock<std::mutex> g(lane_mu);
    while (true) {
        for (size_t i = free_lanes.size(); i-- > 0;)            // the lane released last first: its workspaces are warm
            if (wanted < 0 || free_lanes[i] == wanted) {
                int const id = free_lanes[i];
                free_lanes.erase(free_lanes.begin() + (long)i);
                return lanes[(size_t)id].get();
            }
        lane_cv.wait(g);
    }
}
void flx_ctx::warm_one_cold_lane(flx::Lane* like) {
    // A lane allocates its workspaces (the trace arena alone is GBs) the first time a chunk runs on it. The thread that has
    // just finished a chunk pays that for one lane that has not run yet, so that lanes first used later in a run, when more
    // batches are in flight, start warm.
    flx::Lane* cold = nullptr;
    {
        std::lock_guard<std::mutex> g(lane_mu);
        for (size_t i = 0; i < free_lanes.size(); ++i)
            if (!lanes[(size_t)free_lanes[i]]->has_run) {
                cold = lanes[(size_t)free_lanes[i]].get();
                free_lanes.erase(free_lanes.begin() + (long)i);
                break;
            }
    }
    if (!cold) return;
    (void)cold->size_like(*like);
    cold->has_run = true;
    release_lane(cold);
}
void flx_ctx::release_lane(flx::Lane* lane) {
    { std::lock_guard<std::mutex> g(lane_mu); free_lanes.push_back(lane->id); }
    lane_cv.notify_all();
}
void flx_ctx::k1_acquire() {
    if (k1_tokens <= 0) return;
    std::unique_lock<std::mutex> g(lane_mu);
    lane_cv.wait(g, [&] { return k1_running < k1_tokens; });
    ++k1_running;
}
void flx_ctx::k1_release() {
    if (k1_tokens <= 0) return;
    { std::lock_guard<std::mutex> g(lane_mu); --k1_running; }
    lane_cv.notify_all();
}
int flx_ctx::sync_all() {
    for (auto& l : lanes) { int rc = l->sync(); if (rc) return rc; }
    return FLX_OK;
}

namespace flx {

int h2d(Lane* ctx, DeviceBuffer& buf, const void* src, size_t bytes, size_t extra_zero_tail) {
    int rc = buf.ensure(bytes + extra_zero_tail + 16);
    if (rc) return rc;
    if (bytes) FLX_HIP(hipMemcpyAsync(buf.ptr, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (extra_zero_tail) FLX_HIP(hipMemsetAsync((char*)buf.ptr + bytes, 0, extra_zero_tail, ctx->stream));
    return FLX_OK;
}
int d2h(Lane* ctx, void* dst, const void* src, size_t bytes) {
    // A copy into pageable memory makes the calling thread wait, spinning, for everything queued before it. Waiting for the
    // stream on a blocking event first lets the thread sleep while the kernels run, so its core serves another lane.
    if (bytes) {
        int const rc = ctx->wait_idle();
        if (rc) return rc;
        FLX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    return FLX_OK;
}
// upload a byte sequence with TEXT_PAD zero bytes in front and behind; returns pointer to element 0
int upload_padded(Lane* ctx, DeviceBuffer& buf, const u8* src, u64 len, const u8** d_first) {
    int rc = buf.ensure(len + 2 * TEXT_PAD + 16);
    if (rc) return rc;
    FLX_HIP(hipMemsetAsync(buf.ptr, 0, TEXT_PAD, ctx->stream));
    if (len) FLX_HIP(hipMemcpyAsync((char*)buf.ptr + TEXT_PAD, src, len, hipMemcpyHostToDevice, ctx->stream));
    FLX_HIP(hipMemsetAsync((char*)buf.ptr + TEXT_PAD + len, 0, TEXT_PAD + 16, ctx->stream));
    *d_first = (const u8*)buf.ptr + TEXT_PAD;
    return FLX_OK;
}

}  // namespace flx
