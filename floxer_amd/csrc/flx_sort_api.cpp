// flx_sort: the object behind the coordinate-order calls of the C ABI (include/floxer_amd.h). The rule and its checks: flx_sort.hpp; the
// kernels: flx_sort.hip. The object owns one stream, the key table (a SortKey and a SortMeta per record added, in adding order), the
// staging buffers of an add and the ping-pong buffers of a sort. Adds judge their records without the object's lock and take it for
// the staging and the launches only, so several host threads may add at once. With device -1 nothing of the device exists and the
// same calls keep the keys in host vectors and order them with std::sort (flx_sort_host's code). The host driver of the passes, which
// flx_sv shares: flx_sort_driver.hpp; the scan of a pass's table: flx_scan.hip; what the object shares with the other side objects:
// flx_object.hpp.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <numeric>
#include <set>

#include "flx_object.hpp"
#include "flx_sort_driver.hpp"

using namespace flx;

namespace {
constexpr u64 DEFAULT_INITIAL_CAPACITY = 1ull << 20;
}  // namespace

struct flx_sort : SideObject {           // mu: the table, staging, launches and `finished`; FLX_SORT_PROFILE
    u32 n_refs = 0;
    u64 initial_capacity = DEFAULT_INITIAL_CAPACITY;
    bool finished = false;
    u64 count = 0, capacity = 0;         // records added; records the table holds
    std::set<u64> first_ordinals;        // of the adds so far
    DeviceBuffer keys, meta;             // the table
    DeviceBuffer records, words;         // an add's staging
    RadixSorter sorter;                  // the sort's driver with its ping-pong buffers (an add's own records, or the whole table at finish)
    DeviceBuffer entries;                // the sorted entries, behind finish
    std::vector<SortKey> h_keys;         // the host form's table
    std::vector<SortMeta> h_meta;
    std::vector<flx_sort_entry> h_entries;
};

namespace {

struct Piece { const flx_record* records; u64 n; const u32* words; u64 n_words; };

// the order of keys[0, n) as indices, by the rule's comparison
void host_order(const SortKey* keys, u64 n, std::vector<u32>& order) {
    order.resize(n);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return sort_key_less(keys[a], keys[b]); });
}
flx_sort_entry entry_of(SortKey const& k, SortMeta const& m) {
    return flx_sort_entry{sort_key_ordinal(k), sort_key_reference(k), sort_key_position(k), m.end, m.flag};
}

// the table holds at least `need` records afterwards, its first `count` as before; a failure leaves it as it was
int grow(flx_sort* s, u64 need) {
    if (need <= s->capacity) return FLX_OK;
    u64 const cap = std::min<u64>(std::max<u64>({need, s->capacity * 2, s->initial_capacity}), SORT_MAX_RECORDS);
    DeviceBuffer keys, meta;
    int rc;
    if ((rc = keys.ensure(cap * sizeof(SortKey), true)) || (rc = meta.ensure(cap * sizeof(SortMeta), true))) return rc;
    if (s->count) {
        FLX_HIP(hipMemcpyAsync(keys.ptr, s->keys.ptr, s->count * sizeof(SortKey), hipMemcpyDeviceToDevice, s->stream));
        FLX_HIP(hipMemcpyAsync(meta.ptr, s->meta.ptr, s->count * sizeof(SortMeta), hipMemcpyDeviceToDevice, s->stream));
        FLX_HIP(hipStreamSynchronize(s->stream));
    }
    s->keys.take(keys);
    s->meta.take(meta);
    s->capacity = cap;
    return FLX_OK;
}

int add_pieces(flx_sort* s, std::vector<Piece> const& pieces, u64 first_ordinal, u32* out_order, const char* who) {
    auto const t0 = std::chrono::steady_clock::now();
    u64 total = 0;
    for (auto const& p : pieces) total += p.n;
    if (first_ordinal >= SORT_MAX_ORDINAL || total > SORT_MAX_ORDINAL - first_ordinal) { set_error(std::string(who) + ": an ordinal of 2^63 or more"); return FLX_ERR_INVALID; }
    // judged before anything is added, without the lock
    std::vector<SortKey> keys;
    std::vector<SortMeta> meta;
    {
        u64 at = 0;
        std::string error;
        for (auto const& p : pieces) {
            if (!sort_plan(s->n_refs, p.records, p.n, p.words, p.n_words, first_ordinal + at, nullptr, who, keys, meta, &error)) { set_error(error); return FLX_ERR_INVALID; }
            at += p.n;
        }
    }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->finished) { set_error(std::string(who) + ": the sort object is finished"); return FLX_ERR_INVALID; }
    if (total == 0) return FLX_OK;
    if (s->first_ordinals.count(first_ordinal)) { set_error(std::string(who) + ": first_ordinal " + std::to_string(first_ordinal) + " was added before"); return FLX_ERR_INVALID; }
    if (total > SORT_MAX_RECORDS - s->count) { set_error(std::string(who) + ": more than 2^32 - 1 records in one sort object"); return FLX_ERR_CAPACITY; }
    if (s->device < 0) {
        if (out_order) {
            std::vector<u32> order;
            host_order(keys.data(), total, order);
            memcpy(out_order, order.data(), total * 4);
        }
        s->h_keys.insert(s->h_keys.end(), keys.begin(), keys.end());
        s->h_meta.insert(s->h_meta.end(), meta.begin(), meta.end());
        s->count += total;
        s->first_ordinals.insert(first_ordinal);
        return FLX_OK;
    }
    FLX_HIP(hipSetDevice(s->device));
    int rc = grow(s, s->count + total);
    if (rc) return rc;
    u64 upload = 0, at = 0;
    float add_ms = 0, ms;
    for (auto const& p : pieces) {
        if (p.n == 0) continue;
        if ((rc = s->records.ensure(p.n * sizeof(flx_record))) || (rc = s->words.ensure(std::max<u64>(p.n_words, 1) * 4))) return rc;
        FLX_HIP(hipMemcpyAsync(s->records.ptr, p.records, p.n * sizeof(flx_record), hipMemcpyHostToDevice, s->stream));
        if (p.n_words) FLX_HIP(hipMemcpyAsync(s->words.ptr, p.words, p.n_words * 4, hipMemcpyHostToDevice, s->stream));
        upload += p.n * sizeof(flx_record) + p.n_words * 4;
        if ((rc = s->span_begin())) return rc;
        // (a piece has fewer than 2^32 records: the object's limit was checked above)
        FLX_LAUNCH("sort_keys_add", SortDevice::keys_add(s->stream, s->records.as<flx_record>(), (u32)p.n, s->words.as<u32>(), first_ordinal + at,
                                                       s->keys.as<SortKey>() + s->count + at, s->meta.as<SortMeta>() + s->count + at));
        if ((rc = s->span_end())) return rc;
        FLX_HIP(hipStreamSynchronize(s->stream));        // (the staging buffers are free for the next piece)
        if ((rc = s->span_ms(ms))) return rc;
        add_ms += ms;
        at += p.n;
    }
    u32 passes = 0;
    float sort_ms = 0;
    if (out_order) {
        if ((rc = s->sorter.keys_a.ensure(total * sizeof(SortKey))) || (rc = s->sorter.keys_b.ensure(total * sizeof(SortKey))) || (rc = s->sorter.pay_a.ensure(total * 4)) ||
            (rc = s->sorter.pay_b.ensure(total * 4)))
            return rc;
        if ((rc = s->span_begin())) return rc;
        FLX_HIP(hipMemcpyAsync(s->sorter.keys_a.ptr, s->keys.as<SortKey>() + s->count, total * sizeof(SortKey), hipMemcpyDeviceToDevice, s->stream));
        FLX_LAUNCH("sort_iota", SortDevice::iota(s->stream, s->sorter.pay_a.as<u32>(), total));
        SortKey* sorted_keys;
        u32* sorted_payload;
        if ((rc = s->sorter.sort(s->stream, s->sorter.keys_a.as<SortKey>(), s->sorter.keys_b.as<SortKey>(), s->sorter.pay_a.as<u32>(), s->sorter.pay_b.as<u32>(), total, &sorted_keys, &sorted_payload, &passes))) return rc;
        FLX_HIP(hipMemcpyAsync(out_order, sorted_payload, total * 4, hipMemcpyDeviceToHost, s->stream));
        if ((rc = s->span_end())) return rc;
        FLX_HIP(hipStreamSynchronize(s->stream));
        if ((rc = s->span_ms(sort_ms))) return rc;
    }
    s->count += total;
    s->first_ordinals.insert(first_ordinal);
    if (s->profile) {
        double const wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[flx sort] add: records %llu upload_bytes %llu sort_keys_add_ms %.3f order_passes %u order_ms %.3f order_download_bytes %llu wall_ms %.3f\n",
                (unsigned long long)total, (unsigned long long)upload, (double)add_ms, passes, (double)sort_ms, (unsigned long long)(out_order ? total * 4 : 0), wall);
    }
    return FLX_OK;
}

bool options_valid(const flx_sort_options* o) {
    if (!o) return true;
    for (uint32_t r : o->reserved) if (r) { set_error("flx_sort_options: the reserved fields must be 0"); return false; }
    if (o->tile_keys % SortDevice::THREADS != 0) { set_error("flx_sort_options: tile_keys must be a multiple of " + std::to_string(SortDevice::THREADS)); return false; }
    if (o->initial_capacity > SORT_MAX_RECORDS) { set_error("flx_sort_options: initial_capacity above 2^32 - 1"); return false; }
    return true;
}

}  // namespace

extern "C" int flx_sort_create(int hip_device, uint32_t n_refs, const flx_sort_options* o, flx_sort** out) {
    if (!out) { set_error("flx_sort_create: null argument"); return FLX_ERR_INVALID; }
    if (hip_device < -1) { set_error("flx_sort_create: a device below -1"); return FLX_ERR_INVALID; }
    if (!options_valid(o)) return FLX_ERR_INVALID;
    auto s = std::make_unique<flx_sort>();              // (an error below drops it: nothing stays allocated)
    s->n_refs = n_refs;
    if (o && o->initial_capacity) s->initial_capacity = o->initial_capacity;
    if (o && o->tile_keys) s->sorter.tile_keys = o->tile_keys;
    int const rc = s->open(hip_device, "FLX_SORT_PROFILE");
    if (rc) return rc;
    *out = s.release();
    return FLX_OK;
}
extern "C" void flx_sort_free(flx_sort* s) { free_object(s); }

extern "C" int flx_sort_add_records(flx_sort* s, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words, uint64_t first_ordinal,
                                    uint32_t* out_order) {
    if (!s || (n && !records)) { set_error("flx_sort_add_records: null argument"); return FLX_ERR_INVALID; }
    return add_pieces(s, {Piece{records, n, cigar_words, n_words}}, first_ordinal, out_order, "flx_sort_add_records");
}
extern "C" int flx_sort_add_run(flx_sort* s, const flx_run* run, uint64_t first_ordinal, uint32_t* out_order) {
    if (!s || !run) { set_error("flx_sort_add_run: null argument"); return FLX_ERR_INVALID; }
    std::vector<Piece> pieces;
    for (const flx_run* p : run_pieces(run)) pieces.push_back(Piece{p->records.data(), p->records.size(), p->cigars.data(), p->cigars.size()});
    return add_pieces(s, pieces, first_ordinal, out_order, "flx_sort_add_run");
}

extern "C" int flx_sort_finish(flx_sort* s) {
    if (!s) { set_error("flx_sort_finish: null argument"); return FLX_ERR_INVALID; }
    std::lock_guard<std::mutex> g(s->mu);
    if (s->finished) { set_error("flx_sort_finish: the sort object is finished"); return FLX_ERR_INVALID; }
    auto const t0 = std::chrono::steady_clock::now();
    u64 const n = s->count;
    if (s->device < 0) {
        std::vector<u32> order;
        host_order(s->h_keys.data(), n, order);
        s->h_entries.resize(n);
        for (u64 i = 0; i < n; ++i) s->h_entries[i] = entry_of(s->h_keys[order[i]], s->h_meta[order[i]]);
        s->finished = true;
        return FLX_OK;
    }
    u32 passes = 0;
    float ms = 0;
    if (n) {
        FLX_HIP(hipSetDevice(s->device));
        int rc;
        if ((rc = s->sorter.keys_b.ensure(n * sizeof(SortKey), true)) || (rc = s->sorter.pay_a.ensure(n * 4, true)) || (rc = s->sorter.pay_b.ensure(n * 4, true)) ||
            (rc = s->entries.ensure(n * sizeof(flx_sort_entry), true)))
            return rc;
        if ((rc = s->span_begin())) return rc;
        FLX_LAUNCH("sort_iota", SortDevice::iota(s->stream, s->sorter.pay_a.as<u32>(), n));
        SortKey* sorted_keys;
        u32* sorted_payload;
        // (the table itself is the first buffer: it is not read in adding order again)
        if ((rc = s->sorter.sort(s->stream, s->keys.as<SortKey>(), s->sorter.keys_b.as<SortKey>(), s->sorter.pay_a.as<u32>(), s->sorter.pay_b.as<u32>(), n, &sorted_keys, &sorted_payload, &passes))) return rc;
        FLX_LAUNCH("sort_entries", SortDevice::entries(s->stream, sorted_keys, sorted_payload, s->meta.as<SortMeta>(), n, s->entries.ptr));
        if ((rc = s->span_end())) return rc;
        FLX_HIP(hipStreamSynchronize(s->stream));
        if ((rc = s->span_ms(ms))) return rc;
        s->keys.release(); s->meta.release(); s->sorter.release(); s->records.release(); s->words.release();
        s->capacity = 0;
    }
    s->finished = true;
    if (s->profile) {
        double const wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[flx sort] finish: records %llu passes %u device_ms %.3f wall_ms %.3f\n", (unsigned long long)n, passes, (double)ms, wall);
    }
    return FLX_OK;
}

extern "C" uint64_t flx_sort_num_records(const flx_sort* s) {
    if (!s) return 0;
    std::lock_guard<std::mutex> g(const_cast<flx_sort*>(s)->mu);
    return s->count;
}
extern "C" int flx_sort_copy(const flx_sort* cs, uint64_t from, uint64_t to, flx_sort_entry* out) {
    if (!cs) { set_error("flx_sort_copy: null argument"); return FLX_ERR_INVALID; }
    flx_sort* const s = const_cast<flx_sort*>(cs);
    std::lock_guard<std::mutex> g(s->mu);
    if (!s->finished) { set_error("flx_sort_copy: call flx_sort_finish first"); return FLX_ERR_INVALID; }
    if (from > to || to > s->count) { set_error("flx_sort_copy: a stretch outside the entries"); return FLX_ERR_INVALID; }
    if (from == to) return FLX_OK;
    if (!out) { set_error("flx_sort_copy: null argument"); return FLX_ERR_INVALID; }
    if (s->device < 0) { memcpy(out, s->h_entries.data() + from, (to - from) * sizeof(flx_sort_entry)); return FLX_OK; }
    FLX_HIP(hipSetDevice(s->device));
    FLX_HIP(hipMemcpyAsync(out, s->entries.as<flx_sort_entry>() + from, (to - from) * sizeof(flx_sort_entry), hipMemcpyDeviceToHost, s->stream));
    FLX_HIP(hipStreamSynchronize(s->stream));
    return FLX_OK;
}

extern "C" int flx_sort_geometry(uint32_t out[4]) {
    if (!out) { set_error("flx_sort_geometry: null argument"); return FLX_ERR_INVALID; }
    out[0] = SortDevice::TILE_KEYS;
    out[1] = SORT_DIGIT_BITS;
    out[2] = (uint32_t)DEFAULT_INITIAL_CAPACITY;
    out[3] = ScanDevice::SCAN_TILE;
    return FLX_OK;
}

extern "C" int flx_sort_host(uint32_t n_refs, const flx_record* records, uint64_t n, const uint32_t* cigar_words, uint64_t n_words, const uint64_t* ordinals,
                             flx_sort_entry* out_sorted) {
    if (n && (!records || !ordinals || !out_sorted)) { set_error("flx_sort_host: null argument"); return FLX_ERR_INVALID; }
    if (n > SORT_MAX_RECORDS) { set_error("flx_sort_host: more than 2^32 - 1 records"); return FLX_ERR_CAPACITY; }
    std::vector<SortKey> keys;
    std::vector<SortMeta> meta;
    std::string error;
    if (!sort_plan(n_refs, records, n, cigar_words, n_words, 0, ordinals, "flx_sort_host", keys, meta, &error)) { set_error(error); return FLX_ERR_INVALID; }
    std::vector<u32> order;
    host_order(keys.data(), n, order);
    for (u64 i = 0; i < n; ++i) out_sorted[i] = entry_of(keys[order[i]], meta[order[i]]);
    return FLX_OK;
}

namespace {
const SortCalls sort_calls{flx_sort_create, flx_sort_free, flx_sort_add_records, flx_sort_finish, flx_sort_num_records, flx_sort_copy};
[[maybe_unused]] const bool sort_calls_registered = (flx::g_sort_calls = &sort_calls, true);
}  // namespace
