// What the side objects behind the C ABI share (flx_coverage, flx_pileup, flx_sort, flx_paf, flx_sv, flx_errprof, flx_consensus; each in its own
// *_api.cpp): the base with the device, the stream, the lock and the profile's events; the pieces of a run; judging on several threads;
// the staging of the reads' letters; and, for coverage, pileup and the consensus, the base of an accumulator of u32 planes over the
// concatenation of the sequences with its scan and its absorb.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "flx_pipeline.hpp"
#include "flx_scan.hpp"

namespace flx {

struct SideObject {
    int device = 0;                      // -1: the host form (no stream, nothing of the device)
    hipStream_t stream = nullptr;
    std::mutex mu;                       // buffers, launches and the object's state
    bool profile = false;                // the object's FLX_*_PROFILE is set (and not 0): its calls print their times to stderr
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    ~SideObject() {
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
        if (stream) (void)hipStreamDestroy(stream);
    }
    // the device made current and the stream made; dev -1: neither
    int open(int dev, const char* profile_env) {
        device = dev;
        if (const char* env = getenv(profile_env)) profile = strtol(env, nullptr, 10) != 0 || env[0] == '\0';
        if (dev < 0) return FLX_OK;
        FLX_HIP(hipSetDevice(dev));
        FLX_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return FLX_OK;
    }
    // A span of device time on the stream, measured only with `profile`: span_begin and span_end round the launches, span_ms behind the
    // wait for the stream (0 without `profile`). The events are made on first use.
    int span_begin() {
        if (!profile) return FLX_OK;
        if (!ev_a) { FLX_HIP(hipEventCreate(&ev_a)); FLX_HIP(hipEventCreate(&ev_b)); }
        FLX_HIP(hipEventRecord(ev_a, stream));
        return FLX_OK;
    }
    int span_end() {
        if (profile) FLX_HIP(hipEventRecord(ev_b, stream));
        return FLX_OK;
    }
    int span_ms(float& ms) {
        ms = 0;
        if (profile) FLX_HIP(hipEventElapsedTime(&ms, ev_a, ev_b));
        return FLX_OK;
    }
};

template <class T>
void free_object(T* o) {
    if (!o) return;
    if (o->device >= 0) (void)hipSetDevice(o->device);
    delete o;
}

// a run is its own records plus its per-lane parts, each over its own word pool, in the order flx_run_copy lists them
inline std::vector<const flx_run*> run_pieces(const flx_run* run) {
    std::vector<const flx_run*> pieces{run};
    for (auto const& p : run->parts) pieces.push_back(&p);
    return pieces;
}

// judge(i) for every i in [0, n), on up to eight threads (thread t takes i = t, t + threads, ..). judge returns false behind set_error:
// the first refusal in index order is the one reported, on the caller's thread (the message is the judging thread's own).
template <class F>
bool judge_in_parallel(size_t n, F&& judge) {
    std::vector<std::string> refusals(n);
    std::vector<char> refused(n, 0);
    auto one = [&](size_t i) {
        if (!judge(i)) { refused[i] = 1; refusals[i] = flx_last_error(); }
    };
    size_t const n_threads = std::min<size_t>(8, n);
    if (n_threads <= 1) for (size_t i = 0; i < n; ++i) one(i);
    else {
        std::vector<std::thread> threads;
        for (size_t t = 0; t < n_threads; ++t)
            threads.emplace_back([&, t] { for (size_t i = t; i < n; i += n_threads) one(i); });
        for (auto& t : threads) t.join();
    }
    for (size_t i = 0; i < n; ++i)
        if (refused[i]) { set_error(refusals[i]); return false; }
    return true;
}

// Where the letters of the reads come from (pileup, the error profile, the consensus): the caller's rank pool (forward sequences: a
// reverse complement is made here with the rank routine) or a batch's host copy (both orientations, flx_reads::pool).
struct Letters {
    const uint8_t* read_pool = nullptr;
    const uint64_t* read_offsets = nullptr;
    const flx_reads* batch = nullptr;
    uint64_t n_reads = 0;
    u64 length(u64 i) const { return batch ? batch->lens[i] : read_offsets[i + 1] - read_offsets[i]; }
    void oriented(u64 i, bool reverse, u8* out) const {
        u64 const len = length(i);
        if (batch) memcpy(out, batch->pool.data() + batch->pool_off[i] + (reverse ? len : 0), len);
        else if (reverse) reverse_complement(read_pool + read_offsets[i], len, out);
        else memcpy(out, read_pool + read_offsets[i], len);
    }
};

// the oriented sequences the jobs refer to (a job has read_index, reverse and seq_off), each once per orientation used, and every
// job's seq_off into them
template <class Job>
void stage_letters(std::vector<Job>& jobs, Letters const& src, std::vector<u8>& pool) {
    std::vector<u64> keys;
    keys.reserve(jobs.size());
    for (auto const& j : jobs) keys.push_back(j.read_index * 2 + j.reverse);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    std::vector<u64> off(keys.size() + 1, 0);
    for (size_t k = 0; k < keys.size(); ++k) off[k + 1] = off[k] + src.length(keys[k] >> 1);
    pool.resize(off.back());
    for (size_t k = 0; k < keys.size(); ++k) src.oriented(keys[k] >> 1, (keys[k] & 1) != 0, pool.data() + off[k]);
    for (auto& j : jobs) j.seq_off = off[(size_t)(std::lower_bound(keys.begin(), keys.end(), j.read_index * 2 + j.reverse) - keys.begin())];
}

// Coverage, pileup and the consensus: u32 planes over the unpadded concatenation of the sequences, differences until the object's finish.
struct PlaneObject : SideObject {
    static constexpr u64 ABSORB_CHUNK = 4ull << 20;    // entries per piece of an absorb (16 MB)
    std::vector<u64> starts;             // n_refs + 1
    u64 total = 0;
    DeviceBuffer acc, d_starts;          // acc_entries of u32, cleared; the starts as u32
    u64 acc_entries = 0;
    ScanDriver scan;                     // reserved for `total` elements
    DeviceBuffer chunk;                  // absorb: a piece of the other object's accumulator on this device
    PinnedBuffer pinned;                 // absorb: the same piece on its way through the host
    bool finished = false;
    u32 n_refs() const { return (u32)(starts.size() - 1); }
    u64 n_tiles() const { return ScanDriver::tiles(total); }

    // the common part of a create; counts: the per-tile count arrays that the object's finish scans
    int create(int dev, const char* profile_env, std::vector<u64>&& starts_, u64 entries, std::initializer_list<DeviceBuffer*> counts) {
        device = dev;
        FLX_HIP(hipSetDevice(device));                  // (a device below 0 is refused here: these objects have no host form)
        int rc = open(dev, profile_env);
        if (rc) return rc;
        starts = std::move(starts_);
        total = starts.back();
        acc_entries = entries;
        if ((rc = acc.ensure(entries * 4, true))) return rc;
        FLX_HIP(hipMemsetAsync(acc.ptr, 0, entries * 4, stream));
        std::vector<u32> starts32(starts.begin(), starts.end());
        if ((rc = d_starts.ensure(starts32.size() * 4, true))) return rc;
        FLX_HIP(hipMemcpyAsync(d_starts.ptr, starts32.data(), starts32.size() * 4, hipMemcpyHostToDevice, stream));
        if ((rc = scan.reserve(total))) return rc;
        for (DeviceBuffer* c : counts)
            if ((rc = c->ensure(n_tiles() * 4, true))) return rc;
        FLX_HIP(hipStreamSynchronize(stream));
        return FLX_OK;
    }
    // the accumulator all zero again, the stream idle
    int clear() {
        FLX_HIP(hipSetDevice(device));
        FLX_HIP(hipMemsetAsync(acc.ptr, 0, acc_entries * 4, stream));
        FLX_HIP(hipStreamSynchronize(stream));
        return FLX_OK;
    }
};

// into_ptr[0, n) += from_ptr[0, n), from `from`'s device to `into`'s in pieces through pinned memory. Both objects' locks are held.
inline int absorb_plane(PlaneObject* into, PlaneObject* from, u32* into_ptr, const u32* from_ptr, u64 n) {
    u64 const piece = std::min(n, PlaneObject::ABSORB_CHUNK);
    FLX_HIP(hipSetDevice(into->device));
    int rc;
    if ((rc = into->pinned.ensure(piece * 4)) || (rc = into->chunk.ensure(piece * 4, true))) return rc;
    for (u64 at = 0; at < n; at += piece) {
        u64 const m = std::min(piece, n - at);
        FLX_HIP(hipSetDevice(from->device));
        FLX_HIP(hipMemcpyAsync(into->pinned.ptr, from_ptr + at, m * 4, hipMemcpyDeviceToHost, from->stream));
        FLX_HIP(hipStreamSynchronize(from->stream));
        FLX_HIP(hipSetDevice(into->device));
        FLX_HIP(hipMemcpyAsync(into->chunk.ptr, into->pinned.ptr, m * 4, hipMemcpyHostToDevice, into->stream));
        FLX_LAUNCH("sum", ScanDevice::sum(into->stream, into_ptr + at, into->chunk.as<u32>(), m));
        FLX_HIP(hipStreamSynchronize(into->stream));    // (the piece's buffers are free again)
    }
    return FLX_OK;
}

// the copy calls of a PlaneObject work only behind its finish call
template <class T>
bool finished_for_copy(const T* c, const char* who, const char* finish_call) {
    if (!c) { set_error(std::string(who) + ": null argument"); return false; }
    std::lock_guard<std::mutex> g(const_cast<T*>(c)->mu);
    if (!c->finished) { set_error(std::string(who) + ": call " + finish_call + " first"); return false; }
    return true;
}

}  // namespace flx
